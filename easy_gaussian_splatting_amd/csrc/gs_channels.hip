// gs_channels.hip -- colour features of 1 .. 4 channels (non-SH colours; gs_blend_fwd_ch / gs_blend_bwd_ch) for gfx950:
//   rec_colors_kernel     : the colour quad of the blend record (floats 8..11, zero above the channel count) for the Gaussians a
//                           geometry-only gs_project_fwd (stage 1) found visible
//   channel_grads_kernel  : the per-Gaussian channel gradients, summed from the colour quad of the gradient rows gs_blend_bwd_ch left
//                           (floats 8..11; quad_sums_wave of gs_common.h, shared with gs_depth.hip) -- the geometry gradients come
//                           from gs_project_bwd, which sums floats 0..10 only
#include "gs_common.h"

namespace gs {

constexpr int kChThreads = 256;

__global__ __launch_bounds__(kChThreads) void rec_colors_kernel(int64_t CN, int64_t N, int D, const float* __restrict__ colors,
                                                                int per_cam, const int32_t* __restrict__ radii, float4* __restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * kChThreads + threadIdx.x;
    if (f >= CN || radii[f] <= 0) return;
    const float* src = colors + (int64_t)D * (per_cam ? f : f % N);
    float c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = i < D ? src[i] : 0.f;
    rec[3 * f + 2] = make_float4(c[0], c[1], c[2], c[3]);
}

struct ChanGradArgs {
    int C, D, per_cam;
    int64_t N;
    const int32_t *radii, *tiles_per_gauss, *cum_tiles, *row_base;
    const uint8_t* qmask;
    const float4* rows;   // [rows][3]: the colour quad is float4 2 of a row
    float* v_colors;      // [N, D] or [C, N, D]
    const int64_t* guard;
};

__device__ __forceinline__ void store_channels(float* d, int D, const float4 v) {
    d[0] = v.x;
    if (D > 1) d[1] = v.y;
    if (D > 2) d[2] = v.z;
    if (D > 3) d[3] = v.w;
}

// One thread per Gaussian n; the cameras in order (colours shared by the cameras: their sums added in camera order, like
// gs_project_bwd's accumulation).
__global__ __launch_bounds__(kChThreads) void channel_grads_kernel(const ChanGradArgs a) {
    __shared__ float4 items[kChThreads / 64][64];
    if (guard_tripped(a.guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kChThreads + threadIdx.x;
    const bool in_range = n < a.N;
    float4* item = items[threadIdx.x >> 6];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < a.C; ++c) {
        const int64_t f = (int64_t)c * a.N + n;
        const bool vis = in_range && a.radii[f] > 0;
        const int cnt = vis ? a.tiles_per_gauss[f] : 0;
        const int base = vis ? a.cum_tiles[f] : 0;
        int r0 = 0, nr = 0;
        if (cnt > 0) { r0 = rows_before(a.row_base, a.qmask, base); nr = rows_before(a.row_base, a.qmask, base + cnt) - r0; }
        const float4 s = quad_sums_wave(a.rows, nr, r0, item);
        if (a.per_cam) {
            if (in_range) store_channels(a.v_colors + (int64_t)a.D * f, a.D, s);
        } else {
            acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
        }
    }
    if (!a.per_cam && in_range) store_channels(a.v_colors + (int64_t)a.D * n, a.D, acc);
}

}  // namespace gs

using namespace gs;

extern "C" int gs_rec_colors(void* stream, int C, int64_t N, int channels, const float* colors, int colors_per_camera,
                             const int32_t* radii, float* rec) {
    GS_REQUIRE(channels >= 1 && channels <= 4, "channels must be 1, 2, 3 or 4");
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(colors && radii && rec, "null pointer");
    GS_REQUIRE(((uintptr_t)rec & 15) == 0, "rec must be 16-byte aligned");
    const int64_t CN = (int64_t)C * N;
    if (CN == 0) return GS_OK;
    hipLaunchKernelGGL(rec_colors_kernel, dim3((unsigned)((CN + kChThreads - 1) / kChThreads)), dim3(kChThreads), 0,
                       (hipStream_t)stream, CN, N, channels, colors, colors_per_camera ? 1 : 0, radii, reinterpret_cast<float4*>(rec));
    GS_LAUNCH_CHECK("rec_colors_kernel");
    return GS_OK;
}

extern "C" int gs_channel_grads(void* stream, int C, int64_t N, int channels, int colors_per_camera, const int32_t* radii,
                                const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                                const uint8_t* qmask, float* v_colors) {
    GS_REQUIRE(channels >= 1 && channels <= 4, "channels must be 1, 2, 3 or 4");
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(radii && tiles_per_gauss && cum_tiles && rows && row_base && qmask && v_colors, "null pointer");
    GS_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)qmask & 15) == 0, "rows / qmask 16-byte aligned");
    GS_REQUIRE(current_rounds().phase == 0, "the rows of depth rounds are two ranges: channel gradients are one-round only");
    if (N == 0) return GS_OK;
    ChanGradArgs a;
    a.C = C; a.D = channels; a.per_cam = colors_per_camera ? 1 : 0; a.N = N;
    a.radii = radii; a.tiles_per_gauss = tiles_per_gauss; a.cum_tiles = cum_tiles; a.row_base = row_base; a.qmask = qmask;
    a.rows = reinterpret_cast<const float4*>(rows); a.v_colors = v_colors;
    a.guard = current_guard().info;
    hipLaunchKernelGGL(channel_grads_kernel, dim3((unsigned)((N + kChThreads - 1) / kChThreads)), dim3(kChThreads), 0,
                       (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("channel_grads_kernel");
    return GS_OK;
}
