// gs_normals.hip -- the normal-consistency regulariser for gfx950 (normals.py).  Every value is the function
// gs_normals.h states, bit for bit; the loss value is the header's terms summed in fp64 in a fixed order.
//
//   gauss_normals_fwd_kernel : one thread per Gaussian; the C cameras are read from device memory (uniform loads); normals [C][N][3]
//   gauss_normals_bwd_kernel : one thread per Gaussian; the gradient of the world normal summed over the cameras in order, then
//                              through the quaternion once: v_quats [N][4], no atomics
//   normal_loss_fwd_kernel   : one block per 64 x 8 tile, one thread per pixel.  The usable depths (normal_depth_ok of the render's
//                              4th channel and the alpha) of the tile and a halo of 1 go to LDS; a thread forms its centre from
//                              five LDS words, adds its terms of sum(w e), sum(w) in fp64 and, when asked, stores the depth normal.
//                              Lanes (xor butterfly), the block's waves in order, a per-block pair of partials.
//   normal_loss_finish_kernel: the partials in block order, value and 1 / sum(w) rounded to fp32 once into the record
//   normal_loss_bwd_kernel   : one block per 64 x 8 tile, gather form.  Usable depths of the tile and a halo of 2 to LDS; every
//                              centre of the tile and of a halo of 1 is formed once and what it sends to its four neighbours' depths
//                              goes to LDS (float4); a thread then writes its pixel's whole v_render4: its own centre's v_Nb and the
//                              sum of what the four centres around it sent.  Every pixel is written, no atomics.
// A wave is one row of 64 pixels, so every LDS access of a wave is a run of 64 consecutive words whatever the row length (66, 68):
// ds_read_b32 and ds_write_b32 bank 32-lane halves modulo 32, and 32 consecutive words never meet.
#include "gs_common.h"
#include "gs_normals.h"

namespace gs {

constexpr int kNmTw = GS_NORMAL_TILE_W, kNmTh = GS_NORMAL_TILE_H, kNmThreads = kNmTw * kNmTh;
static_assert(kNmTw == kWave, "a wave is one row of the tile");

__global__ __launch_bounds__(256) void gauss_normals_fwd_kernel(int64_t N, int C, const float* __restrict__ means,
                                                                const float* __restrict__ quats, const float* __restrict__ scales,
                                                                const float* __restrict__ viewmats, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    gauss_normals_fwd(N, C, i, means, quats, scales, viewmats, normals);
}

__global__ __launch_bounds__(256) void gauss_normals_bwd_kernel(int64_t N, int C, const float* __restrict__ means,
                                                                const float* __restrict__ quats, const float* __restrict__ scales,
                                                                const float* __restrict__ viewmats, const float* __restrict__ v_normals,
                                                                float* __restrict__ v_quats) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    gauss_normals_bwd(N, C, i, means, quats, scales, viewmats, v_normals, v_quats);
}

struct NormalLossArgs {
    int H, W, tiles_x, blocks;
    const float* K;         // device float[9]
    float min_alpha;
    int detach_depth;
    const float* render4;   // [H][W][4]: the blended normal and the expected depth
    const float* alphas;    // [H][W]
    const float* mask;      // [H][W] or null
    float* rec;             // {value, 1 / sum(w)}
    double* partials;
    float* depth_normals;   // [H][W][3] or null
    const float* v_loss;
    float* v_render4;       // [H][W][4]
};

// the usable depth of pixel (x, y), 0 outside the frame
__device__ __forceinline__ float nm_load_depth(const NormalLossArgs& a, int x, int y) {
    if (x < 0 || y < 0 || x >= a.W || y >= a.H) return 0.f;
    const int p = y * a.W + x;   // (H * W * 4 < 2^31)
    return normal_depth_ok(a.render4[4 * p + 3], a.alphas[p], a.min_alpha);
}

// the depths of the tile at (x0, y0) and a halo of R into lds[(kNmTh + 2R)][(kNmTw + 2R)]
template <int R>
__device__ __forceinline__ void nm_fill_depths(const NormalLossArgs& a, int x0, int y0, float* lds) {
    constexpr int RW = kNmTw + 2 * R, RH = kNmTh + 2 * R;
    for (int i = threadIdx.x; i < RW * RH; i += kNmThreads) {
        const int ly = i / RW, lx = i - ly * RW;
        lds[i] = nm_load_depth(a, x0 + lx - R, y0 + ly - R);
    }
}

// the centre at (x, y) from a depth tile of halo R whose cell (lx, ly) it is; false when it is not valid
template <int R>
__device__ __forceinline__ bool nm_centre(const NormalLossArgs& a, const NormalCam& cam, const float* lds, int lx, int ly, int x, int y,
                                          NormalCentre& c) {
    constexpr int RW = kNmTw + 2 * R;
    if (x < 1 || y < 1 || x > a.W - 2 || y > a.H - 2) return false;
    const float* d = lds + ly * RW + lx;
    return normal_centre(cam, x, y, d[0], d[-1], d[1], d[-RW], d[RW], c);
}

__device__ __forceinline__ double nm_wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kNmThreads) void normal_loss_fwd_kernel(const NormalLossArgs a) {
    __shared__ float depth[(kNmTh + 2) * (kNmTw + 2)];
    __shared__ double wsum[kNmTh][2];
    const int tx = threadIdx.x & (kNmTw - 1), ty = threadIdx.x >> 6;
    const int by = (int)blockIdx.x / a.tiles_x, bx = (int)blockIdx.x - by * a.tiles_x;
    const int x0 = bx * kNmTw, y0 = by * kNmTh, x = x0 + tx, y = y0 + ty;
    const NormalCam cam = normal_cam(a.K);
    nm_fill_depths<1>(a, x0, y0, depth);
    __syncthreads();
    double acc[2] = {0.0, 0.0};
    if (x < a.W && y < a.H) {
        const int p = y * a.W + x;
        NormalCentre c;
        const bool valid = nm_centre<1>(a, cam, depth, tx + 1, ty + 1, x, y, c);
        if (valid) {
            const float w = normal_loss_weight(a.mask != nullptr ? a.mask[p] : 0.f);
            if (w != 0.f) {
                const float4 r = reinterpret_cast<const float4*>(a.render4)[p];
                const float nb[3] = {r.x, r.y, r.z};
                normal_loss_accumulate(acc, c, nb, w);
            }
        }
        if (a.depth_normals != nullptr) {
            float* o = a.depth_normals + 3 * (int64_t)p;
            o[0] = valid ? c.n[0] : 0.f; o[1] = valid ? c.n[1] : 0.f; o[2] = valid ? c.n[2] : 0.f;
        }
    }
    if (a.partials == nullptr) return;   // (block-uniform: the depth normals alone)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double t = nm_wave_sum_f64(acc[i]);
        if (lane_id() == 0) wsum[ty][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = wsum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kNmTh; ++w) t += wsum[w][threadIdx.x];
        a.partials[2 * (int64_t)blockIdx.x + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(2 * kWave) void normal_loss_finish_kernel(const NormalLossArgs a) {
    __shared__ double sums[2];
    const int k = threadIdx.x >> 6;   // which of the two sums
    double t = 0.0;
    for (int blk = lane_id(); blk < a.blocks; blk += kWave) t += a.partials[2 * (int64_t)blk + k];
    t = nm_wave_sum_f64(t);
    if (lane_id() == 0) sums[k] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        float value, inv_w;
        normal_loss_finish(sums[0], sums[1], value, inv_w);
        a.rec[GS_NORMAL_REC_VALUE] = value;
        a.rec[GS_NORMAL_REC_INV_W] = inv_w;
    }
}

__global__ __launch_bounds__(kNmThreads) void normal_loss_bwd_kernel(const NormalLossArgs a) {
    constexpr int SW = kNmTw + 2, SH = kNmTh + 2;   // the centres: the tile and a halo of 1
    __shared__ float depth[(kNmTh + 4) * (kNmTw + 4)];
    __shared__ float4 sent[SH * SW];
    const int tx = threadIdx.x & (kNmTw - 1), ty = threadIdx.x >> 6;
    const int by = (int)blockIdx.x / a.tiles_x, bx = (int)blockIdx.x - by * a.tiles_x;
    const int x0 = bx * kNmTw, y0 = by * kNmTh;
    const NormalCam cam = normal_cam(a.K);
    const float scale = fp_opaque(a.v_loss[0] * a.rec[GS_NORMAL_REC_INV_W]);
    nm_fill_depths<2>(a, x0, y0, depth);
    __syncthreads();
    float v_nb[3] = {0.f, 0.f, 0.f};
    // pass 0: a thread's own centre, (tx, ty) of the tile; pass 1: the ring of SW * SH - 512 = 148 centres around the tile
    for (int pass = 0; pass < 2; ++pass) {
        int lx, ly;   // the cell of `sent`
        if (pass == 0) {
            lx = tx + 1; ly = ty + 1;
        } else {
            const int r = threadIdx.x;
            if (r >= 2 * SW + 2 * kNmTh) break;
            if (r < SW) { lx = r; ly = 0; }
            else if (r < 2 * SW) { lx = r - SW; ly = SH - 1; }
            else if (r < 2 * SW + kNmTh) { lx = 0; ly = 1 + (r - 2 * SW); }
            else { lx = SW - 1; ly = 1 + (r - 2 * SW - kNmTh); }
        }
        const int x = x0 + lx - 1, y = y0 + ly - 1;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        NormalCentre c;
        if (nm_centre<2>(a, cam, depth, lx + 1, ly + 1, x, y, c)) {   // (valid: interior, so inside the frame)
            const int p = y * a.W + x;
            const float w = normal_loss_weight(a.mask != nullptr ? a.mask[p] : 0.f);
            if (w != 0.f) {
                const float4 r = reinterpret_cast<const float4*>(a.render4)[p];
                const float nb[3] = {r.x, r.y, r.z};
                float vn[3], send[4];
                normal_centre_vjp(cam, x, y, c, nb, -(scale * w), vn, send);
                if (pass == 0) { v_nb[0] = vn[0]; v_nb[1] = vn[1]; v_nb[2] = vn[2]; }
                if (!a.detach_depth) s = make_float4(send[0], send[1], send[2], send[3]);
            }
        }
        sent[ly * SW + lx] = s;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x < a.W && y < a.H) {
        const float4* m = sent + (ty + 1) * SW + (tx + 1);
        // the centre above sends its "down" (.y), the one below its "up" (.x), the one to the left its "right" (.w), to the right its "left" (.z)
        const float vd = normal_depth_gather(m[-SW].y, m[SW].x, m[-1].w, m[1].z);
        reinterpret_cast<float4*>(a.v_render4)[y * a.W + x] = make_float4(v_nb[0], v_nb[1], v_nb[2], vd);
    }
}

static bool nm_frame_ok(int height, int width) { return height > 0 && width > 0 && (int64_t)height * width * 4 < (1ll << 31); }
static NormalLossArgs nm_args(int height, int width) {
    NormalLossArgs a = {};
    a.H = height; a.W = width;
    a.tiles_x = (width + kNmTw - 1) / kNmTw;
    a.blocks = a.tiles_x * ((height + kNmTh - 1) / kNmTh);
    return a;
}

}  // namespace gs

using namespace gs;

static inline bool nm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define GS_NM_GAUSS_ARGS()                                                                                             \
    GS_REQUIRE(N >= 0 && N < (1ll << 31) && C >= 1 && (int64_t)C * N * 3 < (1ll << 40), "0 <= N < 2^31, C >= 1");       \
    if (N == 0) return GS_OK;                                                                                          \
    GS_REQUIRE(means && quats && scales && viewmats, "null pointer")

extern "C" int gs_gauss_normals_fwd(void* stream, int64_t N, int C, const float* means, const float* quats, const float* scales,
                                    const float* viewmats, float* normals) {
    GS_NM_GAUSS_ARGS();
    GS_REQUIRE(normals != nullptr, "null pointer");
    hipLaunchKernelGGL(gauss_normals_fwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, C, means, quats,
                       scales, viewmats, normals);
    GS_LAUNCH_CHECK("gauss_normals_fwd_kernel");
    return GS_OK;
}

extern "C" int gs_gauss_normals_bwd(void* stream, int64_t N, int C, const float* means, const float* quats, const float* scales,
                                    const float* viewmats, const float* v_normals, float* v_quats) {
    GS_NM_GAUSS_ARGS();
    GS_REQUIRE(v_normals != nullptr && v_quats != nullptr, "null pointer");
    hipLaunchKernelGGL(gauss_normals_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, C, means, quats,
                       scales, viewmats, v_normals, v_quats);
    GS_LAUNCH_CHECK("gauss_normals_bwd_kernel");
    return GS_OK;
}

extern "C" size_t gs_normal_loss_partials_doubles(int height, int width) {
    if (!nm_frame_ok(height, width)) return 0;
    return 2 * (size_t)nm_args(height, width).blocks;
}

#define GS_NM_FRAME_MSG "height > 0, width > 0 and height * width * 4 < 2^31"

extern "C" int gs_normal_loss_fwd(void* stream, int height, int width, const float* K_dev, float min_alpha, const float* render4,
                                  const float* alphas, const float* mask, float* rec_dev, double* partials, float* depth_normals) {
    GS_REQUIRE(nm_frame_ok(height, width), GS_NM_FRAME_MSG);
    GS_REQUIRE(min_alpha == min_alpha, "min_alpha is NaN");
    GS_REQUIRE(K_dev && render4 && alphas, "null pointer");
    GS_REQUIRE((rec_dev != nullptr) == (partials != nullptr), "rec_dev and partials come together");
    GS_REQUIRE(rec_dev != nullptr || depth_normals != nullptr, "nothing to compute: no record and no depth-normal image");
    GS_REQUIRE(nm_aligned16(render4) && ((uintptr_t)alphas & 3) == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)rec_dev & 3) == 0 &&
                   ((uintptr_t)partials & 7) == 0 && ((uintptr_t)depth_normals & 3) == 0,
               "render4 16-byte, partials 8-byte, the others 4-byte aligned");
    GS_REQUIRE((const void*)depth_normals != (const void*)render4, "an output aliases an input");
    NormalLossArgs a = nm_args(height, width);
    a.K = K_dev; a.min_alpha = min_alpha; a.render4 = render4; a.alphas = alphas; a.mask = mask; a.rec = rec_dev; a.partials = partials;
    a.depth_normals = depth_normals;
    hipLaunchKernelGGL(normal_loss_fwd_kernel, dim3(a.blocks), dim3(kNmThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("normal_loss_fwd_kernel");
    if (rec_dev != nullptr) {
        hipLaunchKernelGGL(normal_loss_finish_kernel, dim3(1), dim3(2 * kWave), 0, (hipStream_t)stream, a);
        GS_LAUNCH_CHECK("normal_loss_finish_kernel");
    }
    return GS_OK;
}

extern "C" int gs_normal_loss_bwd(void* stream, int height, int width, const float* K_dev, float min_alpha, int detach_depth,
                                  const float* render4, const float* alphas, const float* mask, const float* rec_dev, const float* v_loss,
                                  float* v_render4) {
    GS_REQUIRE(nm_frame_ok(height, width), GS_NM_FRAME_MSG);
    GS_REQUIRE(min_alpha == min_alpha, "min_alpha is NaN");
    GS_REQUIRE(detach_depth == 0 || detach_depth == 1, "detach_depth is 0 or 1");
    GS_REQUIRE(K_dev && render4 && alphas && rec_dev && v_loss && v_render4, "null pointer");
    GS_REQUIRE(nm_aligned16(render4) && nm_aligned16(v_render4) && ((uintptr_t)alphas & 3) == 0 && ((uintptr_t)mask & 3) == 0 &&
                   ((uintptr_t)rec_dev & 3) == 0 && ((uintptr_t)v_loss & 3) == 0,
               "render4 and v_render4 16-byte, the others 4-byte aligned");
    GS_REQUIRE((const void*)v_render4 != (const void*)render4, "an output aliases an input");
    NormalLossArgs a = nm_args(height, width);
    a.K = K_dev; a.min_alpha = min_alpha; a.detach_depth = detach_depth; a.render4 = render4; a.alphas = alphas; a.mask = mask;
    a.rec = const_cast<float*>(rec_dev); a.v_loss = v_loss; a.v_render4 = v_render4;
    hipLaunchKernelGGL(normal_loss_bwd_kernel, dim3(a.blocks), dim3(kNmThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("normal_loss_bwd_kernel");
    return GS_OK;
}
