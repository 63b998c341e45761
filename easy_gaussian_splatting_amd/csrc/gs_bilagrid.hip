// gs_bilagrid.hip -- per-view bilateral grids of colour affines (include/gs_raster.h "Per-view bilateral grids"; DESIGN.md "Bilateral
// grids in the captured step"): the math is gs_bilagrid.h, shared with the host tests.
//   bilagrid_step_inputs_kernel  {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), view, 0} of the step about to run into a device record
//   bilagrid_apply_kernel        out = the slice of the view's slab applied to the render: a streaming pass, 24 B per pixel
//   bilagrid_scatter_kernel      the slice's adjoint without atomics: a block owns (spatial cell, chunk of its pixels, luminance node)
//                                and sums its pixels' 4 corners x 12 coefficients in fp64 -- thread, wave, block --, one partial each
//   bilagrid_nodes_kernel        per node and coefficient the at most 4 cells x chunks partials in a fixed order, rounded to fp32 once
//   bilagrid_vjp_kernel          v <- M^T v + w v_luma in place: a streaming pass, 36 B per pixel
//   bilagrid_tv_kernel           tv_weight d tv / d grids (+ the view's slab) for every node and the value's per-block fp64 partials
//   bilagrid_tv_finish           the partials in block order, the value, tv_weight * tv onto the loss total
//   bilagrid_adam_kernel         DENSE Adam over every element of every view, guarded
// The image kernels are shaped along the slab's SPATIAL cells: the pixels of cell (cx, cy) are a rectangle (gs_bilagrid.h
// bilagrid_axis_first), and a block that serves pixels of one cell needs 2 x 2 x L x 12 nodes -- 3 KB of LDS at L = 16 -- instead
// of the view's slab (96 KB at the defaults).  A cell is split into `chunks` blocks of 256 threads striding over its pixels.
#include "gs_common.h"
#include "gs_bilagrid.h"

namespace gs {

constexpr int kBgThreads = 256;
// Pixels a block takes of a full cell.  A block's fixed work -- its rectangle, the 48-value reduction, the partial store -- is
// worth several hundred pixels, so a big launch takes 8192 per block (32 per thread: -51 us on the bench frame's backward against
// 2048); a launch that would then have fewer than kBgFewBlocks blocks keeps 2048, to have blocks at all.
constexpr int kBgChunkPixels = 8192;
constexpr int kBgChunkPixelsSmall = 2048;
constexpr int kBgFewBlocks = 1024;
constexpr int kBgMaxChunks = 64;
constexpr int kBgMaxL = GS_BILAGRID_MAX_L;
constexpr int kBgTvBlocks = GS_BILAGRID_TV_DOUBLES;

struct BilagridStepRec { float v[GS_BILAGRID_REC_FLOATS]; };
struct BgShape { int H, W, Wg, Hg, L, n_views; };

__global__ void bilagrid_step_inputs_kernel(const BilagridStepRec r, float* __restrict__ rec) {
    const unsigned t = threadIdx.x;
    if (t < (unsigned)GS_BILAGRID_REC_FLOATS) rec[t] = r.v[t];
}

__device__ __forceinline__ int bilagrid_view(const float* rec, int view) {
    return rec ? __float_as_int(rec[GS_BILAGRID_REC_VIEW]) : view;
}

// chunks per cell for a frame: the largest cell is at most ceil(W / (Wg - 1)) + 1 by ceil(H / (Hg - 1)) + 1 pixels
static inline int bilagrid_chunks(const BgShape& s) {
    const int64_t wc = (s.W + s.Wg - 2) / (s.Wg - 1) + 1, hc = (s.H + s.Hg - 2) / (s.Hg - 1) + 1;
    int64_t c = (wc * hc + kBgChunkPixels - 1) / kBgChunkPixels;
    if ((int64_t)(s.Wg - 1) * (s.Hg - 1) * s.L * c < kBgFewBlocks) c = (wc * hc + kBgChunkPixelsSmall - 1) / kBgChunkPixelsSmall;
    return (int)(c < 1 ? 1 : (c > kBgMaxChunks ? kBgMaxChunks : c));
}

// The block's cell (blockIdx.x) and its pixel rectangle [x0, x0 + wc) x [y0, y0 + hc)
struct BgRect { int cx, cy, x0, y0, wc, hc; };
__device__ __forceinline__ BgRect bilagrid_rect(const BgShape& s) {
    BgRect r;
    r.cx = (int)blockIdx.x % (s.Wg - 1);
    r.cy = (int)blockIdx.x / (s.Wg - 1);
    r.x0 = bilagrid_axis_first(r.cx, s.W, s.Wg);
    r.y0 = bilagrid_axis_first(r.cy, s.H, s.Hg);
    r.wc = bilagrid_axis_first(r.cx + 1, s.W, s.Wg) - r.x0;
    r.hc = bilagrid_axis_first(r.cy + 1, s.H, s.Hg) - r.y0;
    return r;
}

// A thread's walk over its block's pixels of the rectangle, pixel i = blockIdx.y * 256 + thread, then every gridDim.y * 256-th: (x, y)
// inside the rectangle kept by carrying, one division per thread in front of the loop instead of one per pixel.
struct BgWalk {
    int i, x, y, dx, dy, step;
    __device__ __forceinline__ BgWalk(const BgRect& r) {
        step = (int)gridDim.y * kBgThreads;
        i = (int)blockIdx.y * kBgThreads + (int)threadIdx.x;
        const int wc = r.wc > 0 ? r.wc : 1;
        y = i / wc; x = i - y * wc;
        dy = step / wc; dx = step - dy * wc;
    }
    __device__ __forceinline__ void next(const BgRect& r) {
        i += step; x += dx; y += dy;
        if (x >= r.wc) { x -= r.wc; ++y; }
    }
};

// The cell's 2 x 2 x L x 12 nodes into LDS as nodes[z][corner (y, x)][k]
__device__ __forceinline__ void bilagrid_stage(const BgShape& s, const BgRect& r, const float* __restrict__ slab, float4* nodes4) {
    float* nodes = reinterpret_cast<float*>(nodes4);
    const int n = 48 * s.L;
    for (int e = threadIdx.x; e < n; e += kBgThreads) {
        const int k = e % 12, sc = (e / 12) & 3, z = e / 48;
        nodes[e] = slab[(((int64_t)k * s.L + z) * s.Hg + (r.cy + (sc >> 1))) * s.Wg + (r.cx + (sc & 1))];
    }
    __syncthreads();
}

// M (and, BWD, D = M_z1 - M_z0) of a pixel from the staged nodes: four channels at a time, a 16-byte LDS read per corner
template <bool BWD>
__device__ __forceinline__ void bilagrid_slice(const float4* nodes4, const BilagridCell& c, float M[12], float D[12]) {
    const float4* lo = nodes4 + 12 * c.iz;   // [z][corner][3 float4]
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float4 n4[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) n4[i] = lo[3 * i + q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float n[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) n[i] = j == 0 ? n4[i].x : (j == 1 ? n4[i].y : (j == 2 ? n4[i].z : n4[i].w));
            float m0, m1;
            M[4 * q + j] = bilagrid_slice1(n, c.tx, c.ty, c.tz, m0, m1);
            if (BWD) D[4 * q + j] = m1 - m0;
        }
    }
}

__global__ __launch_bounds__(kBgThreads) void bilagrid_apply_kernel(const BgShape s, const float* __restrict__ rec, int view_arg,
                                                                     const float* __restrict__ grids, const float* __restrict__ render,
                                                                     float* __restrict__ out) {
    __shared__ float4 nodes[12 * kBgMaxL];
    const int view = bilagrid_view(rec, view_arg);
    if ((unsigned)view >= (unsigned)s.n_views) return;   // (the entries refuse such a view: never taken)
    const BgRect r = bilagrid_rect(s);
    const int n_pix = r.wc * r.hc;
    if ((int)blockIdx.y * kBgThreads >= n_pix) return;   // (block-uniform, in front of the barrier)
    bilagrid_stage(s, r, grids + (int64_t)view * 12 * s.L * s.Hg * s.Wg, nodes);
    for (BgWalk w(r); w.i < n_pix; w.next(r)) {
        const int x = r.x0 + w.x, y = r.y0 + w.y;
        const int64_t p = 3 * ((int64_t)y * s.W + x);
        const float c0 = render[p], c1 = render[p + 1], c2 = render[p + 2];
        const BilagridCell c = bilagrid_cell(x, y, s.W, s.H, s.Wg, s.Hg, s.L, bilagrid_luma(c0, c1, c2));
        float M[12];
        bilagrid_slice<false>(nodes, c, M, nullptr);
        bilagrid_apply(M, c0, c1, c2, out[p], out[p + 1], out[p + 2]);
    }
}

__global__ __launch_bounds__(kBgThreads) void bilagrid_vjp_kernel(const BgShape s, const float* __restrict__ rec, int view_arg,
                                                                   const float* __restrict__ grids, const float* __restrict__ render,
                                                                   float* __restrict__ v_image) {
    __shared__ float4 nodes[12 * kBgMaxL];
    const int view = bilagrid_view(rec, view_arg);
    if ((unsigned)view >= (unsigned)s.n_views) return;
    const BgRect r = bilagrid_rect(s);
    const int n_pix = r.wc * r.hc;
    if ((int)blockIdx.y * kBgThreads >= n_pix) return;
    bilagrid_stage(s, r, grids + (int64_t)view * 12 * s.L * s.Hg * s.Wg, nodes);
    for (BgWalk w(r); w.i < n_pix; w.next(r)) {
        const int x = r.x0 + w.x, y = r.y0 + w.y;
        const int64_t p = 3 * ((int64_t)y * s.W + x);
        const float c0 = render[p], c1 = render[p + 1], c2 = render[p + 2];
        const float v0 = v_image[p], v1 = v_image[p + 1], v2 = v_image[p + 2];
        const BilagridCell c = bilagrid_cell(x, y, s.W, s.H, s.Wg, s.Hg, s.L, bilagrid_luma(c0, c1, c2));
        float M[12], D[12];
        bilagrid_slice<true>(nodes, c, M, D);
        bilagrid_vjp(M, D, c.zin, s.L, c0, c1, c2, v0, v1, v2, v_image[p], v_image[p + 1], v_image[p + 2]);
    }
}

// The wave's sums of 48 doubles per lane with 51 exchanges instead of 288: four halving steps (lane bit d decides which half of the
// values a lane keeps and which it hands to lane ^ d: 48 -> 24 -> 12 -> 6 -> 3), then a butterfly over the last two bits.  On exit
// lanes with (lane & 3) == 0 hold in acc[0..2] the sums of values 3 * (lane >> 2) .. + 2.  A fixed order: reproducible.
__device__ __forceinline__ void wave_reduce48(double acc[48]) {
    const int lane = lane_id();
    int n = 48;
#pragma unroll
    for (int d = 32; d >= 4; d >>= 1) {
        n >>= 1;
        const bool up = (lane & d) != 0;
#pragma unroll
        for (int i = 0; i < n; ++i) {
            const double send = up ? acc[i] : acc[i + n], keep = up ? acc[i + n] : acc[i];
            acc[i] = keep + __shfl_xor(send, d, 64);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        acc[i] += __shfl_xor(acc[i], 2, 64);
        acc[i] += __shfl_xor(acc[i], 1, 64);
    }
}

// grid (cells, chunks, L): partials[((cell * chunks + chunk) * L + z) * 48 + 12 * corner + k], every entry written (zeros where a
// block has no pixel)
__global__ __launch_bounds__(kBgThreads) void bilagrid_scatter_kernel(const BgShape s, const float* __restrict__ render,
                                                                       const float* __restrict__ v_image, double* __restrict__ partials) {
    __shared__ double wsum[kBgThreads / kWave][48];
    const BgRect r = bilagrid_rect(s);
    const int n_pix = r.wc * r.hc, z = blockIdx.z;
    double acc[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) acc[i] = 0.0;
    for (BgWalk w(r); w.i < n_pix; w.next(r)) {
        const int x = r.x0 + w.x, y = r.y0 + w.y;
        const int64_t p = 3 * ((int64_t)y * s.W + x);
        const float c0 = render[p], c1 = render[p + 1], c2 = render[p + 2];
        BilagridCell c;
        bilagrid_cell_z(bilagrid_luma(c0, c1, c2), s.L, c);
        if (c.iz != z && c.iz + 1 != z) continue;   // the pixel's cell does not touch this luminance node
        bilagrid_cell_xy(x, y, s.W, s.H, s.Wg, s.Hg, c);
        double wx[2], wy[2], wz[2], a[12];
        bilagrid_axis_weights(c.tx, wx); bilagrid_axis_weights(c.ty, wy); bilagrid_axis_weights(c.tz, wz);
        bilagrid_products(v_image[p], v_image[p + 1], v_image[p + 2], c0, c1, c2, a);
        bilagrid_accumulate(acc, wz[z - c.iz], wy, wx, a);
    }
    wave_reduce48(acc);
    const int wave = threadIdx.x >> 6, lane = lane_id();
    if ((lane & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) wsum[wave][3 * (lane >> 2) + i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < 48) {
        double t = wsum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBgThreads / kWave; ++w) t += wsum[w][threadIdx.x];
        partials[(((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * s.L + z) * 48 + threadIdx.x] = t;
    }
}

// v_slab[k][z][y][x] = the partials of the cells (cy, cx) in {y - 1, y} x {x - 1, x} that exist, cy then cx ascending, each cell's
// chunks in order, one rounding to fp32
__global__ __launch_bounds__(kBgThreads) void bilagrid_nodes_kernel(const BgShape s, int chunks, const double* __restrict__ partials,
                                                                     float* __restrict__ v_slab) {
    const int total = 12 * s.L * s.Hg * s.Wg, e = blockIdx.x * kBgThreads + threadIdx.x;
    if (e >= total) return;
    const int k = e % 12, x = (e / 12) % s.Wg, y = (e / (12 * s.Wg)) % s.Hg, z = e / (12 * s.Wg * s.Hg);   // (k fastest: 96-byte runs of a partial)
    double t = 0.0;
    for (int cy = y - 1; cy <= y; ++cy) {
        if (cy < 0 || cy > s.Hg - 2) continue;
        for (int cx = x - 1; cx <= x; ++cx) {
            if (cx < 0 || cx > s.Wg - 2) continue;
            const int sc = 2 * (y - cy) + (x - cx);
            const int64_t cell = (int64_t)cy * (s.Wg - 1) + cx;
            for (int ch = 0; ch < chunks; ++ch) t += partials[((cell * chunks + ch) * s.L + z) * 48 + 12 * sc + k];
        }
    }
    v_slab[((k * s.L + z) * s.Hg + y) * s.Wg + x] = (float)t;
}

// a block's sum, always in the same order: a fixed butterfly inside each wave, then the waves in order (thread 0's)
__device__ __forceinline__ double bilagrid_block_sum(double v, double* lds) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBgThreads / kWave; ++w) t += lds[w];
    return t;
}

struct BgTvArgs {
    BgShape s;
    const float* grids;
    float tv_weight;
    const float* rec;
    int view;
    const float* v_slab;   // or nullptr: the total-variation gradient alone
    float* v_grids;        // or nullptr: the value alone
    double* partial;       // [kBgTvBlocks]
    float *loss3, *tv_out;
    const int64_t* guard;
};

__global__ __launch_bounds__(kBgThreads) void bilagrid_tv_kernel(const BgTvArgs a) {
    __shared__ double lds[kBgThreads / kWave];
    if (guard_tripped(a.guard)) return;
    const BgShape& s = a.s;
    const int view = a.v_slab ? bilagrid_view(a.rec, a.view) : -1;
    // (n_views * slab < 2^31, the entries' contract: 32-bit index arithmetic, three divisions per element)
    const unsigned plane = (unsigned)(s.Hg * s.Wg), slab = 12u * (unsigned)s.L * plane, total = slab * (unsigned)s.n_views;
    const unsigned strides[3] = {plane, (unsigned)s.Wg, 1u};
    const int extent[3] = {s.L, s.Hg, s.Wg};
    double inv_cnt[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) inv_cnt[ax] = 1.0 / ((double)s.n_views * (double)(slab / extent[ax] * (extent[ax] - 1)));
    double value = 0.0;
    for (unsigned e = blockIdx.x * kBgThreads + threadIdx.x; e < total; e += gridDim.x * kBgThreads) {
        const unsigned row = e / (unsigned)s.Wg, lev = row / (unsigned)s.Hg, chan = lev / (unsigned)s.L;   // chan = view * 12 + k
        const int at[3] = {(int)(lev - chan * (unsigned)s.L), (int)(row - lev * (unsigned)s.Hg), (int)(e - row * (unsigned)s.Wg)};
        const unsigned e_view = chan / 12u, in_slab = e - e_view * slab;
        const float g = a.grids[e];
        float gm[3], gp[3];
        bool has_m[3], has_p[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            has_m[ax] = at[ax] > 0; has_p[ax] = at[ax] < extent[ax] - 1;
            gm[ax] = has_m[ax] ? a.grids[e - strides[ax]] : 0.f;
            gp[ax] = has_p[ax] ? a.grids[e + strides[ax]] : 0.f;
        }
        double v, d;
        bilagrid_tv_node(g, gm, gp, has_m, has_p, inv_cnt, v, d);
        value += v;
        if (a.v_grids) {   // the gradient rounded on its own, then the slab's added: autograd's accumulation of the two parts
            const float tvg = (float)((double)a.tv_weight * d);
            a.v_grids[e] = tvg + ((int)e_view == view ? a.v_slab[in_slab] : 0.f);
        }
    }
    const double t = bilagrid_block_sum(value, lds);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(kBgThreads) void bilagrid_tv_finish(const BgTvArgs a, int blocks) {
    __shared__ double lds[kBgThreads / kWave];
    if (guard_tripped(a.guard)) return;
    double t = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kBgThreads) t += a.partial[b];
    const double sum = bilagrid_block_sum(t, lds);
    if (threadIdx.x == 0) {
        const float tv = (float)sum;
        if (a.tv_out) a.tv_out[0] = tv;
        // the eager total: total + tv_weight * tv, the product rounded on its own
        if (a.loss3) a.loss3[2] = a.loss3[2] + fp_opaque(a.tv_weight * tv);
    }
}

__global__ __launch_bounds__(kBgThreads) void bilagrid_adam_kernel(int64_t numel, const float* __restrict__ rec, float* __restrict__ grids,
                                                                    float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                                    const float* __restrict__ v_grids, float b1, float b2, float eps,
                                                                    const int64_t* guard) {
    if (guard_tripped(guard)) return;
    const float ss = rec[GS_BILAGRID_REC_SS], isbc2 = rec[GS_BILAGRID_REC_ISBC2];
    const int64_t quads = numel >> 2, stride = (int64_t)gridDim.x * kBgThreads;   // (numel is a multiple of 12)
    float4* __restrict__ p4 = reinterpret_cast<float4*>(grids);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(exp_avg);
    float4* __restrict__ s4 = reinterpret_cast<float4*>(exp_avg_sq);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(v_grids);
    for (int64_t q = (int64_t)blockIdx.x * kBgThreads + threadIdx.x; q < quads; q += stride) {
        float4 p = p4[q], m = m4[q], v = s4[q];
        const float4 g = g4[q];
        bilagrid_adam1(p.x, g.x, m.x, v.x, b1, b2, eps, isbc2, ss);
        bilagrid_adam1(p.y, g.y, m.y, v.y, b1, b2, eps, isbc2, ss);
        bilagrid_adam1(p.z, g.z, m.z, v.z, b1, b2, eps, isbc2, ss);
        bilagrid_adam1(p.w, g.w, m.w, v.w, b1, b2, eps, isbc2, ss);
        p4[q] = p; m4[q] = m; s4[q] = v;
    }
}

}  // namespace gs

using namespace gs;

#define GS_BG_GRID_ARGS()                                                                                                             \
    GS_REQUIRE(grid_x >= 2 && grid_x <= GS_BILAGRID_MAX_XY && grid_y >= 2 && grid_y <= GS_BILAGRID_MAX_XY, "2 <= grid_x, grid_y <= 64"); \
    GS_REQUIRE(grid_l >= 2 && grid_l <= GS_BILAGRID_MAX_L, "2 <= grid_l <= 16");                                                     \
    GS_REQUIRE(n_views >= 1 && n_views <= GS_BILAGRID_MAX_VIEWS, "1 <= n_views <= GS_BILAGRID_MAX_VIEWS");                          \
    GS_REQUIRE((int64_t)n_views * 12 * grid_l * grid_y * grid_x < ((int64_t)1 << 31), "n_views * 12 * grid_l * grid_y * grid_x < 2^31")
#define GS_BG_IMAGE_ARGS()                                                                                                            \
    GS_REQUIRE(height > 0 && width > 0 && (int64_t)height * width < ((int64_t)1 << 31) / 3, "height, width > 0, 3 * height * width < 2^31"); \
    GS_BG_GRID_ARGS();                                                                                                                \
    GS_REQUIRE(rec_dev != nullptr || (view >= 0 && view < n_views), "without a record: 0 <= view < n_views")

extern "C" int gs_bilagrid_step_inputs(void* stream, int view, int n_views, float lr, float beta1, float beta2, int64_t step, float* rec_dev) {
    GS_REQUIRE(n_views >= 1 && n_views <= GS_BILAGRID_MAX_VIEWS && view >= 0 && view < n_views, "0 <= view < n_views <= GS_BILAGRID_MAX_VIEWS");
    GS_REQUIRE(step >= 1, "step counts from 1");
    GS_REQUIRE(rec_dev != nullptr && ((uintptr_t)rec_dev & 15) == 0, "rec_dev: non-null, 16-byte aligned");
    GS_REQUIRE(lr == lr && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "lr is NaN, or a beta outside [0, 1)");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    BilagridStepRec r = {};
    r.v[GS_BILAGRID_REC_SS] = (float)((double)lr / bc1);   // (gs_step_inputs' host arithmetic)
    r.v[GS_BILAGRID_REC_ISBC2] = (float)(1.0 / sqrt(bc2));
    memcpy(&r.v[GS_BILAGRID_REC_VIEW], &view, sizeof(int));
    hipLaunchKernelGGL(bilagrid_step_inputs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, r, rec_dev);
    GS_LAUNCH_CHECK("bilagrid_step_inputs_kernel");
    return GS_OK;
}

extern "C" int gs_bilagrid_apply(void* stream, int height, int width, int n_views, int grid_x, int grid_y, int grid_l, const float* rec_dev,
                                 int view, const float* grids, const float* render, float* out) {
    GS_BG_IMAGE_ARGS();
    GS_REQUIRE(grids && render && out && render != out, "null pointer, or out aliases render");
    GS_REQUIRE((((uintptr_t)render | (uintptr_t)out | (uintptr_t)grids) & 15) == 0, "images and grids must be 16-byte aligned");
    const BgShape s = {height, width, grid_x, grid_y, grid_l, n_views};
    const dim3 grid((unsigned)((grid_x - 1) * (grid_y - 1)), (unsigned)bilagrid_chunks(s));
    hipLaunchKernelGGL(bilagrid_apply_kernel, grid, dim3(kBgThreads), 0, (hipStream_t)stream, s, rec_dev, view, grids, render, out);
    GS_LAUNCH_CHECK("bilagrid_apply_kernel");
    return GS_OK;
}

extern "C" size_t gs_bilagrid_partials_doubles(int height, int width, int grid_x, int grid_y, int grid_l) {
    if (height <= 0 || width <= 0 || grid_x < 2 || grid_x > GS_BILAGRID_MAX_XY || grid_y < 2 || grid_y > GS_BILAGRID_MAX_XY || grid_l < 2 ||
        grid_l > GS_BILAGRID_MAX_L)
        return 0;
    const BgShape s = {height, width, grid_x, grid_y, grid_l, 1};
    return (size_t)(grid_x - 1) * (grid_y - 1) * bilagrid_chunks(s) * grid_l * 48;
}

extern "C" int gs_bilagrid_bwd(void* stream, int height, int width, int n_views, int grid_x, int grid_y, int grid_l, const float* rec_dev,
                               int view, const float* grids, const float* render, float* v_image, double* partials, float* v_slab) {
    GS_BG_IMAGE_ARGS();
    GS_REQUIRE(grids && render && v_image && partials && v_slab && render != v_image, "null pointer, or v_image aliases render");
    GS_REQUIRE((((uintptr_t)render | (uintptr_t)v_image | (uintptr_t)grids | (uintptr_t)v_slab) & 15) == 0 && ((uintptr_t)partials & 7) == 0,
               "images, grids and v_slab must be 16-byte aligned");
    const BgShape s = {height, width, grid_x, grid_y, grid_l, n_views};
    const int cells = (grid_x - 1) * (grid_y - 1), chunks = bilagrid_chunks(s), nodes = 12 * grid_l * grid_y * grid_x;
    hipLaunchKernelGGL(bilagrid_scatter_kernel, dim3((unsigned)cells, (unsigned)chunks, (unsigned)grid_l), dim3(kBgThreads), 0,
                       (hipStream_t)stream, s, render, v_image, partials);
    GS_LAUNCH_CHECK("bilagrid_scatter_kernel");
    hipLaunchKernelGGL(bilagrid_nodes_kernel, dim3((unsigned)((nodes + kBgThreads - 1) / kBgThreads)), dim3(kBgThreads), 0, (hipStream_t)stream,
                       s, chunks, partials, v_slab);
    GS_LAUNCH_CHECK("bilagrid_nodes_kernel");
    hipLaunchKernelGGL(bilagrid_vjp_kernel, dim3((unsigned)cells, (unsigned)chunks), dim3(kBgThreads), 0, (hipStream_t)stream, s, rec_dev, view,
                       grids, render, v_image);
    GS_LAUNCH_CHECK("bilagrid_vjp_kernel");
    return GS_OK;
}

extern "C" int gs_bilagrid_tv(void* stream, int n_views, int grid_x, int grid_y, int grid_l, const float* grids, float tv_weight,
                              const float* rec_dev, int view, const float* v_slab, float* loss3, float* tv_out, float* v_grids,
                              double* tv_ws) {
    GS_BG_GRID_ARGS();
    GS_REQUIRE(grids && tv_ws && ((uintptr_t)tv_ws & 7) == 0, "null pointer: grids, tv_ws");
    GS_REQUIRE(tv_weight == tv_weight, "tv_weight is NaN");
    GS_REQUIRE(v_slab == nullptr || (v_grids != nullptr && (rec_dev != nullptr || (view >= 0 && view < n_views))),
               "v_slab needs v_grids and a view: the record's, or 0 <= view < n_views");
    BgTvArgs a = {{0, 0, grid_x, grid_y, grid_l, n_views}, grids, tv_weight, rec_dev, view, v_slab, v_grids, tv_ws, loss3, tv_out,
                  current_guard().info};
    const int64_t total = (int64_t)n_views * 12 * grid_l * grid_y * grid_x, want = (total + kBgThreads - 1) / kBgThreads;
    const int blocks = (int)(want > kBgTvBlocks ? kBgTvBlocks : want);
    hipLaunchKernelGGL(bilagrid_tv_kernel, dim3((unsigned)blocks), dim3(kBgThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("bilagrid_tv_kernel");
    hipLaunchKernelGGL(bilagrid_tv_finish, dim3(1), dim3(kBgThreads), 0, (hipStream_t)stream, a, blocks);
    GS_LAUNCH_CHECK("bilagrid_tv_finish");
    return GS_OK;
}

extern "C" int gs_bilagrid_adam(void* stream, int64_t numel, const float* rec_dev, float* grids, float* exp_avg, float* exp_avg_sq,
                                const float* v_grids, float beta1, float beta2, float eps) {
    GS_REQUIRE(numel >= 12 && numel % 12 == 0 && numel < ((int64_t)1 << 31), "numel: a multiple of 12 in [12, 2^31)");
    GS_REQUIRE(rec_dev && grids && exp_avg && exp_avg_sq && v_grids, "null pointer");
    GS_REQUIRE((((uintptr_t)grids | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)v_grids) & 15) == 0, "buffers must be 16-byte aligned");
    const int64_t blocks = ((numel >> 2) + kBgThreads - 1) / kBgThreads;
    hipLaunchKernelGGL(bilagrid_adam_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(kBgThreads), 0, (hipStream_t)stream, numel,
                       rec_dev, grids, exp_avg, exp_avg_sq, v_grids, beta1, beta2, eps, current_guard().info);
    GS_LAUNCH_CHECK("bilagrid_adam_kernel");
    return GS_OK;
}
