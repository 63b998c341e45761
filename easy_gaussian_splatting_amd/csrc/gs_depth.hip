// gs_depth.hip -- gsplat's depth render modes ("D", "ED", "RGB+D", "RGB+ED") for gfx950.  The depth of a (camera, Gaussian) is the
// projection's camera-space z; it rides the blend as one more colour channel (gs_blend_fwd / gs_blend_fwd_ch at Dc + 1 channels):
//   rec_depth_kernel      : depths[f] into lane j of the record's colour quad (floats 8..11) of the visible Gaussians
//   depth_grads_kernel    : v_z per (camera, Gaussian) = the sum of lane j of the colour quad of the Gaussian's gradient rows
//                           (quad_sums_wave, gs_common.h), pushed to v_means and -- on request -- to fp64 per-block partials of
//                           row 2 of v_viewmats
//   depth_cam_sum_kernel  : a camera's partials added in a fixed order onto v_viewmats[c, 2, :]
//   expected_depth_*      : the ED normalisation of the last channel, one thread per pixel, forward and backward
// The per-element arithmetic is gs_math.h's (depth_vjp_mean, depth_vjp_cam, expected_depth, expected_depth_vjp).
#include "gs_common.h"
#include "gs_math.h"

namespace gs {

constexpr int kDepthThreads = 256;

__device__ __forceinline__ float quad_lane(const float4 q, int j) { return j == 0 ? q.x : (j == 1 ? q.y : (j == 2 ? q.z : q.w)); }

__global__ __launch_bounds__(kDepthThreads) void rec_depth_kernel(int64_t CN, int lane, const float* __restrict__ depths,
                                                                  const int32_t* __restrict__ radii, float* __restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    if (f >= CN || radii[f] <= 0) return;
    const float z = depths[f];
    // (lane 0: depth alone -- the geometry-only projection left the quad unwritten and the blend reads three lanes of it)
    if (lane == 0) reinterpret_cast<float4*>(rec)[3 * f + 2] = make_float4(z, 0.f, 0.f, 0.f);
    else rec[GS_REC_FLOATS * f + 8 + lane] = z;
}

struct DepthGradArgs {
    int C, lane;
    int64_t N;
    const float *means, *viewmats;
    const int32_t *radii, *tiles_per_gauss, *cum_tiles, *row_base;
    const uint8_t* qmask;
    const float4* rows;     // [rows][3]: the colour quad is float4 2 of a row
    float* v_means;         // [N,3]  read, added to, written
    float* v_depths;        // [C,N]  optional
    double* cam_partials;   // [C][gridDim.x][4]  optional
    const int64_t* guard;
};

// v_z of (camera, Gaussian) f: lane a.lane of the sum of the colour quads of its gradient rows (0 for culled Gaussians and rows nobody
// took) -- the one gather of depth_grads_kernel and depth_grads_z_kernel.  Every lane of the wave calls it.
__device__ __forceinline__ float depth_row_vz(const DepthGradArgs& a, int64_t f, bool in_range, float4* item) {
    const bool vis = in_range && a.radii[f] > 0;
    const int cnt = vis ? a.tiles_per_gauss[f] : 0;
    const int base = vis ? a.cum_tiles[f] : 0;
    int r0 = 0, nr = 0;
    if (cnt > 0) { r0 = rows_before(a.row_base, a.qmask, base); nr = rows_before(a.row_base, a.qmask, base + cnt) - r0; }
    return quad_lane(quad_sums_wave(a.rows, nr, r0, item), a.lane);
}

// One thread per Gaussian n, the cameras in order (v_means accumulates in camera order, like gs_project_bwd's launches).
__global__ __launch_bounds__(kDepthThreads) void depth_grads_kernel(const DepthGradArgs a) {
    __shared__ float4 items[kDepthThreads / 64][64];
    __shared__ double wave_sums[kDepthThreads / 64][4];
    if (guard_tripped(a.guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    const bool in_range = n < a.N;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    float4* item = items[wave];
    float mean[3] = {0.f, 0.f, 0.f}, v_mean[3] = {0.f, 0.f, 0.f};
    if (in_range) {
        mean[0] = a.means[3 * n]; mean[1] = a.means[3 * n + 1]; mean[2] = a.means[3 * n + 2];
        v_mean[0] = a.v_means[3 * n]; v_mean[1] = a.v_means[3 * n + 1]; v_mean[2] = a.v_means[3 * n + 2];
    }
    for (int c = 0; c < a.C; ++c) {
        const int64_t f = (int64_t)c * a.N + n;
        const float v_z = depth_row_vz(a, f, in_range, item);
        const float* V = a.viewmats + 16 * c;
        const float row2[3] = {V[8], V[9], V[10]};
        depth_vjp_mean(v_z, row2, v_mean);
        if (a.v_depths && in_range) a.v_depths[f] = v_z;
        if (a.cam_partials) {   // (kernel argument: uniform)
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            depth_vjp_cam(v_z, mean, acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double t = wave_reduce_add(acc[i]);
                if (lane == 0) wave_sums[wave][i] = t;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < kDepthThreads / 64; ++w) t += wave_sums[w][threadIdx.x];
                a.cam_partials[((int64_t)c * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = t;
            }
            __syncthreads();
        }
    }
    if (in_range) { a.v_means[3 * n] = v_mean[0]; a.v_means[3 * n + 1] = v_mean[1]; a.v_means[3 * n + 2] = v_mean[2]; }
}

// The gather of depth_grads_kernel alone: v_depths[f] = v_z, the same depth_row_vz over the same rows (hence the same bits), no
// gradient touched -- what gs_project_bwd_adam_depth adds to the means gradient it forms in registers.
__global__ __launch_bounds__(kDepthThreads) void depth_grads_z_kernel(const DepthGradArgs a) {
    __shared__ float4 items[kDepthThreads / 64][64];
    if (guard_tripped(a.guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    const bool in_range = n < a.N;
    float4* item = items[threadIdx.x >> 6];
    for (int c = 0; c < a.C; ++c) {
        const int64_t f = (int64_t)c * a.N + n;
        const float v_z = depth_row_vz(a, f, in_range, item);
        if (in_range) a.v_depths[f] = v_z;
    }
}

// One block per camera: each of the 4 values is walked by 64 threads over the camera's partials at a stride of 64 blocks, and the
// 64 strided sums are added in order (cam_sum_kernel's scheme); the fp64 total is rounded once and added to v_viewmats[c, 2, :].
constexpr int kDepthSumChains = 64;
__global__ __launch_bounds__(4 * kDepthSumChains) void depth_cam_sum_kernel(const double* __restrict__ cam_partials, int n_blocks,
                                                                            float* __restrict__ v_viewmats,
                                                                            const int64_t* __restrict__ guard) {
    __shared__ double part[kDepthSumChains][4];
    if (guard_tripped(guard)) return;
    const int c = blockIdx.x, term = threadIdx.x & 3, j = threadIdx.x >> 2;
    const double* src = cam_partials + (int64_t)c * n_blocks * 4 + term;
    double t = 0.0;
    for (int b = j; b < n_blocks; b += kDepthSumChains) t += src[(int64_t)b * 4];
    part[j][term] = t;
    __syncthreads();
    if (threadIdx.x < 4) {
        double sum = 0.0;
#pragma unroll 8
        for (int k = 0; k < kDepthSumChains; ++k) sum += part[k][term];
        v_viewmats[16 * c + 8 + term] += (float)sum;
    }
}

// ---- expected depth: one thread per pixel, CH channels of which the last is the depth ----
template <int CH> struct Pix { float v[CH]; };
template <int CH>
__device__ __forceinline__ Pix<CH> load_pix(const float* __restrict__ p, int64_t i) {
    Pix<CH> r;
    if constexpr (CH == 4) { const float4 q = reinterpret_cast<const float4*>(p)[i]; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; }
    else if constexpr (CH == 2) { const float2 q = reinterpret_cast<const float2*>(p)[i]; r.v[0] = q.x; r.v[1] = q.y; }
    else {
#pragma unroll
        for (int k = 0; k < CH; ++k) r.v[k] = p[CH * i + k];
    }
    return r;
}
template <int CH>
__device__ __forceinline__ void store_pix(float* __restrict__ p, int64_t i, const Pix<CH>& r) {
    if constexpr (CH == 4) reinterpret_cast<float4*>(p)[i] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else if constexpr (CH == 2) reinterpret_cast<float2*>(p)[i] = make_float2(r.v[0], r.v[1]);
    else {
#pragma unroll
        for (int k = 0; k < CH; ++k) p[CH * i + k] = r.v[k];
    }
}

template <int CH>
__global__ __launch_bounds__(kDepthThreads) void expected_depth_fwd_kernel(int64_t n_pixels, const float* __restrict__ acc,
                                                                           const float* __restrict__ alphas, float* __restrict__ out,
                                                                           const int64_t* __restrict__ guard) {
    if (guard_tripped(guard)) return;
    const int64_t i = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    if (i >= n_pixels) return;
    Pix<CH> p = load_pix<CH>(acc, i);
    p.v[CH - 1] = expected_depth(p.v[CH - 1], alphas[i]);
    store_pix<CH>(out, i, p);
}

template <int CH>
__global__ __launch_bounds__(kDepthThreads) void expected_depth_bwd_kernel(int64_t n_pixels, const float* __restrict__ acc,
                                                                           const float* __restrict__ alphas, const float* __restrict__ v_out,
                                                                           const float* __restrict__ v_alphas_in, float* __restrict__ v_colors,
                                                                           float* __restrict__ v_alphas, const int64_t* __restrict__ guard) {
    if (guard_tripped(guard)) return;
    const int64_t i = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    if (i >= n_pixels) return;
    Pix<CH> v = load_pix<CH>(v_out, i);
    float v_acc, v_alpha;
    expected_depth_vjp(v.v[CH - 1], acc[CH * i + CH - 1], alphas[i], v_acc, v_alpha);
    v.v[CH - 1] = v_acc;
    store_pix<CH>(v_colors, i, v);
    v_alphas[i] = (v_alphas_in ? v_alphas_in[i] : 0.f) + v_alpha;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_rec_depth(void* stream, int C, int64_t N, int lane, const float* depths, const int32_t* radii, float* rec) {
    GS_REQUIRE(lane >= 0 && lane <= 3, "lane must be 0, 1, 2 or 3");
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(current_rounds().phase == 0, "depth render modes are one-round only");
    const int64_t CN = (int64_t)C * N;
    if (CN == 0) return GS_OK;   // (empty tensors have no address)
    GS_REQUIRE(depths && radii && rec, "null pointer");
    GS_REQUIRE(((uintptr_t)rec & 15) == 0, "rec must be 16-byte aligned");
    hipLaunchKernelGGL(rec_depth_kernel, dim3((unsigned)((CN + kDepthThreads - 1) / kDepthThreads)), dim3(kDepthThreads), 0,
                       (hipStream_t)stream, CN, lane, depths, radii, rec);
    GS_LAUNCH_CHECK("rec_depth_kernel");
    return GS_OK;
}

extern "C" size_t gs_depth_partials_doubles(int C, int64_t N) {
    if (C < 1 || N < 0) return 0;
    return (size_t)C * (size_t)((N + kDepthThreads - 1) / kDepthThreads) * 4;
}

extern "C" int gs_depth_grads(void* stream, int C, int64_t N, int lane, const float* means, const float* viewmats,
                              const int32_t* radii, const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows,
                              const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_depths,
                              double* cam_partials, float* v_viewmats) {
    GS_REQUIRE(lane >= 0 && lane <= 3, "lane must be 0, 1, 2 or 3");
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(current_rounds().phase == 0, "the rows of depth rounds are two ranges: depth gradients are one-round only");
    if (N == 0) return GS_OK;   // (empty tensors have no address; nothing to add to v_viewmats)
    GS_REQUIRE(means && viewmats && radii && tiles_per_gauss && cum_tiles && rows && row_base && qmask && v_means, "null pointer");
    GS_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)qmask & 15) == 0, "rows / qmask 16-byte aligned");
    GS_REQUIRE((v_viewmats == nullptr) == (cam_partials == nullptr) && ((uintptr_t)cam_partials & 7) == 0,
               "v_viewmats and cam_partials (8-byte aligned) come together");
    DepthGradArgs a;
    a.C = C; a.lane = lane; a.N = N; a.means = means; a.viewmats = viewmats;
    a.radii = radii; a.tiles_per_gauss = tiles_per_gauss; a.cum_tiles = cum_tiles; a.row_base = row_base; a.qmask = qmask;
    a.rows = reinterpret_cast<const float4*>(rows); a.v_means = v_means; a.v_depths = v_depths; a.cam_partials = cam_partials;
    a.guard = current_guard().info;
    const int n_blocks = (int)((N + kDepthThreads - 1) / kDepthThreads);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_grads_kernel, dim3((unsigned)n_blocks), dim3(kDepthThreads), 0, st, a);
    GS_LAUNCH_CHECK("depth_grads_kernel");
    if (cam_partials) {
        hipLaunchKernelGGL(depth_cam_sum_kernel, dim3((unsigned)C), dim3(4 * kDepthSumChains), 0, st, (const double*)cam_partials, n_blocks,
                           v_viewmats, a.guard);
        GS_LAUNCH_CHECK("depth_cam_sum_kernel");
    }
    return GS_OK;
}

extern "C" int gs_depth_grads_z(void* stream, int C, int64_t N, int lane, const int32_t* radii, const int32_t* tiles_per_gauss,
                                const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_depths) {
    GS_REQUIRE(lane >= 0 && lane <= 3, "lane must be 0, 1, 2 or 3");
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(current_rounds().phase == 0, "the rows of depth rounds are two ranges: depth gradients are one-round only");
    if (N == 0) return GS_OK;
    GS_REQUIRE(radii && tiles_per_gauss && cum_tiles && rows && row_base && qmask && v_depths, "null pointer");
    GS_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)qmask & 15) == 0, "rows / qmask 16-byte aligned");
    DepthGradArgs a = {};
    a.C = C; a.lane = lane; a.N = N; a.radii = radii; a.tiles_per_gauss = tiles_per_gauss; a.cum_tiles = cum_tiles; a.row_base = row_base;
    a.qmask = qmask; a.rows = reinterpret_cast<const float4*>(rows); a.v_depths = v_depths; a.guard = current_guard().info;
    hipLaunchKernelGGL(depth_grads_z_kernel, dim3((unsigned)((N + kDepthThreads - 1) / kDepthThreads)), dim3(kDepthThreads), 0,
                       (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_grads_z_kernel");
    return GS_OK;
}

static int expected_depth_args(int64_t n_pixels, int channels, const void* a, const void* b, const void* c) {
    GS_REQUIRE(channels >= 1 && channels <= 4, "channels must be 1, 2, 3 or 4");
    GS_REQUIRE(n_pixels >= 0, "n_pixels>=0");
    const uintptr_t align = channels == 4 ? 15 : (channels == 2 ? 7 : 3);
    GS_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & align) == 0, "images must be aligned to a pixel of 2 or 4 channels");
    return GS_OK;
}

#define GS_ED_CH(KERNEL, ...)                                                                                              \
    switch (channels) {                                                                                                    \
        case 1: hipLaunchKernelGGL((KERNEL<1>), grid, dim3(kDepthThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;    \
        case 2: hipLaunchKernelGGL((KERNEL<2>), grid, dim3(kDepthThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;    \
        case 3: hipLaunchKernelGGL((KERNEL<3>), grid, dim3(kDepthThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;    \
        default: hipLaunchKernelGGL((KERNEL<4>), grid, dim3(kDepthThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
    }

extern "C" int gs_expected_depth_fwd(void* stream, int64_t n_pixels, int channels, const float* acc_colors, const float* alphas,
                                     float* out_colors) {
    GS_REQUIRE(acc_colors && alphas && out_colors, "null pointer");
    if (int rc = expected_depth_args(n_pixels, channels, acc_colors, out_colors, nullptr)) return rc;
    if (n_pixels == 0) return GS_OK;
    const dim3 grid((unsigned)((n_pixels + kDepthThreads - 1) / kDepthThreads));
    const int64_t* guard = current_guard().info;
    GS_ED_CH(expected_depth_fwd_kernel, n_pixels, acc_colors, alphas, out_colors, guard)
    GS_LAUNCH_CHECK("expected_depth_fwd_kernel");
    return GS_OK;
}

extern "C" int gs_expected_depth_bwd(void* stream, int64_t n_pixels, int channels, const float* acc_colors, const float* alphas,
                                     const float* v_out, const float* v_alphas_in, float* v_colors, float* v_alphas) {
    GS_REQUIRE(acc_colors && alphas && v_out && v_colors && v_alphas, "null pointer");
    if (int rc = expected_depth_args(n_pixels, channels, acc_colors, v_out, v_colors)) return rc;
    if (n_pixels == 0) return GS_OK;
    const dim3 grid((unsigned)((n_pixels + kDepthThreads - 1) / kDepthThreads));
    const int64_t* guard = current_guard().info;
    GS_ED_CH(expected_depth_bwd_kernel, n_pixels, acc_colors, alphas, v_out, v_alphas_in, v_colors, v_alphas, guard)
    GS_LAUNCH_CHECK("expected_depth_bwd_kernel");
    return GS_OK;
}
#undef GS_ED_CH
