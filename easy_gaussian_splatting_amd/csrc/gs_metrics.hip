// gs_metrics.hip -- the two image metrics an evaluation needs, for gfx950: the mean squared error (torchmetrics
// PeakSignalNoiseRatio(data_range=1.0) before the logarithm) and the mean SSIM (StructuralSimilarityIndexMeasure(data_range=1.0))
// of one view, as the reference's eval.py:45-55 forms them after the mask composite.  Forward only: no derivative maps, no map
// store, a workspace of the per-block partial pairs alone.
//
//   image_metrics_kernel  : l1_ssim_fwd_kernel of gs_loss.hip (the tuned design: one block per 32x32 tile + 5-pixel halo in
//                           loss_tile's XCD order, whole 12-byte pixel loads, a channel at a time in LDS, four moment maps through
//                           register sliding windows, literal taps) without its derivative arithmetic and its 36 B per pixel of map
//                           stores, with a sum of squared differences beside the SSIM sum.  The two separable passes are the loss
//                           kernel's own lines: that kernel's body is held to the code it compiled to before this file existed, so
//                           they are restated here rather than factored out of it.
//   metrics_reduce_kernel : single block, fixed-order sum of the per-block pairs in double; divides and writes {mse, ssim}.
// No atomics: the same inputs give the same bits.
// clamp_input clamps with fminf(fmaxf(r, 0), 1), as the loss kernel does: a NaN in the render becomes 0 (torch.clamp would hand
// it on), so a diverged render evaluates to a finite figure on this path and to NaN in plain torch.
#include "gs_loss_tile.h"
#include "gs_math.h"

namespace gs {

struct MetricsArgs {
    int H, W;
    int clamp_input;                   // render is the un-clamped image: clamp to [0,1] on load
    const float *render, *gt, *mask;   // [H,W,3], [H,W,3], [H,W] or null
    float* partial;                    // [nblocks][2] (sum of squared differences, ssim sum)
};

template <bool MASK>
__global__ __launch_bounds__(256) void image_metrics_kernel(const MetricsArgs a) {
    constexpr float kWin[11] = GS_WIN_TAPS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sx = lds;                         // [kLR][kLRP] render (composited), one channel
    float* sy = sx + kLR * kLRP;             // [kLR][kLRP] ground truth
    float* hp = sy + kLR * kLRP;             // [4][kLR][kHP] horizontal sums
    __shared__ float red[2][4];
    int x0, y0;
    if (!loss_tile(a, x0, y0)) {   // (a block past the end of its XCD's run: the reduction sums every block's pair)
        if (threadIdx.x == 0) { a.partial[2 * blockIdx.x] = 0.f; a.partial[2 * blockIdx.x + 1] = 0.f; }
        return;
    }
    const int tid = threadIdx.x;
    const unsigned row_bytes = 12u * (unsigned)a.W;
    // ---- staging role: thread = one staged column x 7 rows (coordinates clamped: every address lies inside the image; clamped
    // values only feed discarded outputs).  A block-uniform base + a 32-bit byte offset per lane (the entry point bounds H * W).
    constexpr int kPer = kLR / 6;   // 7 rows per thread
    float rv[kPer][3], gv[kPer][3], mv[MASK ? kPer : 1];
    if (tid < kLR * 6) {
        const int rg = tid / kLR, col = tid - rg * kLR;
        const int cx = clampi(x0 - kHalo + col, 0, a.W - 1), ytop = y0 - kHalo + rg;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const unsigned cy = (unsigned)clampi(ytop + 6 * i, 0, a.H - 1);
            const unsigned o = __umul24(cy, row_bytes) + 12u * (unsigned)cx;
            const F3 g3 = ld3_off(a.gt, o), r3 = ld3_off(a.render, o);
            gv[i][0] = g3.x; gv[i][1] = g3.y; gv[i][2] = g3.z;
            rv[i][0] = r3.x; rv[i][1] = r3.y; rv[i][2] = r3.z;
            if (MASK) mv[i] = ld_off(a.mask, __umul24(cy, 4u * (unsigned)a.W) + 4u * (unsigned)cx);
        }
    }
    float sq = 0.f, ssim_sum = 0.f;
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        // (the thread's roles are re-derived from an opaque copy of its index every round, as in the loss kernel: hoisted out of
        //  the loop their addresses and predicates cost registers)
        int t = tid;
        asm volatile("" : "+v"(t));
        const bool st_on = t < kLR * 6;
        const int rg = t / kLR, col = t - rg * kLR;
        if (st_on) {
            const int gx = x0 - kHalo + col;
            const bool col_own = col >= kHalo && col < kHalo + kLT && gx < a.W;
            float* dx = sx + rg * kLRP + col;
            float* dy = sy + rg * kLRP + col;
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int row = rg + 6 * i, gy = y0 - kHalo + row;
                const float g = gv[i][0];
                float r = rv[i][0];
                if (a.clamp_input) r = fminf(fmaxf(r, 0.f), 1.f);
                if (MASK) r = mv[i] * g + (1.f - mv[i]) * r;
                dx[6 * i * kLRP] = r;
                dy[6 * i * kLRP] = g;
                if (col_own && row >= kHalo && row < kHalo + kLT && gy < a.H) { const float d = r - g; sq = fmaf(d, d, sq); }
                gv[i][0] = gv[i][1]; gv[i][1] = gv[i][2];   // the next channel moves up (a rolled loop cannot index registers)
                rv[i][0] = rv[i][1]; rv[i][1] = rv[i][2];
            }
        }
        __syncthreads();
        {
            // horizontal pass: 16 + 16 LDS reads feed 6 x 4 outputs; FOUR moment maps (x, y, x^2 + y^2, xy)
            const int row = col, c0 = min(kHOut * rg, kLT - kHOut);
            if (st_on) {
                float* h = hp + row * kHP + c0;
                float xv[kHWin], yv[kHWin];
#pragma unroll
                for (int i = 0; i < kHWin; ++i) { xv[i] = sx[row * kLRP + c0 + i]; yv[i] = sy[row * kLRP + c0 + i]; }
#pragma unroll
                for (int j = 0; j < kHOut; ++j) {
                    float m0 = kWin[0] * xv[j], m1 = kWin[0] * yv[j], m2 = kWin[0] * fmaf(xv[j], xv[j], yv[j] * yv[j]),
                          m3 = kWin[0] * (xv[j] * yv[j]);
#pragma unroll
                    for (int kk = 1; kk < 11; ++kk) {
                        const float w = kWin[kk], x = xv[j + kk], y = yv[j + kk];
                        m0 = fmaf(w, x, m0); m1 = fmaf(w, y, m1); m2 = fmaf(w, fmaf(x, x, y * y), m2); m3 = fmaf(w, x * y, m3);
                    }
                    h[j] = m0; h[kLR * kHP + j] = m1; h[2 * kLR * kHP + j] = m2; h[3 * kLR * kHP + j] = m3;
                }
            }
        }
        __syncthreads();
        // vertical pass + SSIM: one thread = one column x 4 output rows (14 LDS reads per map)
        {
            const int q = t / kLT, vcol = t - q * kLT, r0 = 4 * q;
            float mom[4][4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                float hv[14];
#pragma unroll
                for (int i = 0; i < 14; ++i) hv[i] = hp[mi * kLR * kHP + (r0 + i) * kHP + vcol];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float acc = kWin[0] * hv[j];
#pragma unroll
                    for (int kk = 1; kk < 11; ++kk) acc = fmaf(kWin[kk], hv[j + kk], acc);
                    mom[mi][j] = acc;
                }
            }
            const int gx = x0 + vcol;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gy = y0 + r0 + j;
                if (gy >= kHalo && gy < a.H - kHalo && gx >= kHalo && gx < a.W - kHalo)   // the interior: the window lies inside the image
                    ssim_sum += ssim_from_moments(mom[0][j], mom[1][j], mom[2][j], mom[3][j]);
            }
        }
        // (no barrier here, unlike the loss kernel: the next channel's staging writes sx / sy, last read in front of the barrier
        //  above, and hp is written again only behind the barrier that follows the staging)
    }
    sq = wave_reduce_add(sq);
    ssim_sum = wave_reduce_add(ssim_sum);
    if (lane_id() == 0) { red[0][tid >> 6] = sq; red[1][tid >> 6] = ssim_sum; }
    __syncthreads();
    if (tid == 0) {
        a.partial[2 * blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        a.partial[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// out[0] = mse over all H W 3 elements, out[1] = mean SSIM over the (H - 10) x (W - 10) interior of the three channels
__global__ __launch_bounds__(256) void metrics_reduce_kernel(int nblocks, const float* __restrict__ partial, int H, int W,
                                                             float* __restrict__ out) {
    __shared__ double red[2][4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { s0 += partial[2 * i]; s1 += partial[2 * i + 1]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); }
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double cnt = (double)(H - 2 * kHalo) * (double)(W - 2 * kHalo) * 3.0;
        out[0] = (float)((red[0][0] + red[0][1] + red[0][2] + red[0][3]) / ((double)H * W * 3.0));
        out[1] = (float)((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / cnt);
    }
}

}  // namespace gs

using namespace gs;

// one (squared error, ssim) pair per LAUNCHED block: the grid is the tile count rounded up to the eight XCD runs
extern "C" size_t gs_metrics_workspace_floats(int height, int width) {
    if (height <= 0 || width <= 0) return 0;
    const size_t nt = (size_t)((width + kLT - 1) / kLT) * ((height + kLT - 1) / kLT);
    return 2 * 8 * ((nt + 7) / 8);
}

extern "C" int gs_image_metrics(void* stream, int height, int width, const float* render, const float* gt, const float* mask,
                                int clamp_input, float* workspace, float* out2) {
    GS_REQUIRE(height > 2 * kHalo && width > 2 * kHalo, "image must be larger than the 11x11 window");
    GS_REQUIRE((int64_t)height * width <= kLossMaxPixels && width <= kLossMaxWidth && height <= (1 << 24),
               "image too large for the metrics kernel's 32-bit byte offsets (H * W <= 2^28, W <= 2^20, H <= 2^24: row indices go through 24-bit multiplies)");
    GS_REQUIRE(render && gt && workspace && out2, "null pointer");
    MetricsArgs a;
    a.H = height; a.W = width; a.clamp_input = clamp_input != 0; a.render = render; a.gt = gt; a.mask = mask; a.partial = workspace;
    const int blocks = (int)loss_grid(loss_tile_count(height, width)).x;
    const size_t lds = sizeof(float) * (2 * kLR * kLRP + 4 * kLR * kHP);
    hipStream_t st = (hipStream_t)stream;
    if (mask) hipLaunchKernelGGL(image_metrics_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(image_metrics_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, st, a);
    GS_LAUNCH_CHECK("image_metrics_kernel");
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3(1), dim3(256), 0, st, blocks, a.partial, height, width, out2);
    GS_LAUNCH_CHECK("metrics_reduce_kernel");
    return GS_OK;
}
