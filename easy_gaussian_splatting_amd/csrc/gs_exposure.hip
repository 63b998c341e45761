// gs_exposure.hip -- per-view exposure compensation (include/gs_raster.h "Per-view exposure compensation"; DESIGN.md "Exposure in the
// captured step"): the math is gs_exposure.h, shared with the host tests.
//   exposure_step_inputs_kernel  {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), view, 0} of the step about to run into a device record
//   exposure_apply_kernel        out = A render + b for the view's row of the table: a streaming pass, 24 B per pixel
//   exposure_bwd_kernel          v <- A^T v in place and the 12 sums {v_i render_j, v_i} in fp64: 36 B per pixel, per-block partials
//   exposure_sums_kernel         the partials in block order, rounded to fp32 once
//   exposure_adam_kernel         DENSE Adam over all n_views x 12 entries -- the sums on the view's row, 0 on every other --, guarded
// The image kernels: 256-thread blocks, a thread takes 4 pixels = 12 floats = three 16-byte accesses per image (48 B per thread keeps
// every access 16-byte aligned), grid-stride from a capped block count; the H*W % 4 pixels left over are block 0's first threads'.
#include "gs_common.h"
#include "gs_exposure.h"

namespace gs {

constexpr int kExpThreads = 256;
constexpr int kExpMaxBlocks = 1024;   // 4 blocks on each of 256 CUs; a frame beyond 1 M pixels strides
constexpr int kExpSumWaves = 12;      // exposure_sums_kernel: a wave per sum

struct ExposureStepRec { float v[GS_EXPOSURE_REC_FLOATS]; };

__global__ void exposure_step_inputs_kernel(const ExposureStepRec r, float* __restrict__ rec) {
    const unsigned t = threadIdx.x;
    if (t < (unsigned)GS_EXPOSURE_REC_FLOATS) rec[t] = r.v[t];
}

__device__ __forceinline__ int exposure_view(const float* rec, int view) {
    return rec ? __float_as_int(rec[GS_EXPOSURE_REC_VIEW]) : view;
}

static inline int exposure_blocks(int64_t n_pix) {
    const int64_t quads = n_pix >> 2, blocks = (quads + kExpThreads - 1) / kExpThreads;
    return (int)(blocks < 1 ? 1 : (blocks > kExpMaxBlocks ? kExpMaxBlocks : blocks));
}

__global__ __launch_bounds__(kExpThreads) void exposure_apply_kernel(int64_t n_pix, int n_views, const float* __restrict__ rec, int view_arg,
                                                                      const float* __restrict__ table, const float* __restrict__ render,
                                                                      float* __restrict__ out) {
    const int view = exposure_view(rec, view_arg);
    if ((unsigned)view >= (unsigned)n_views) return;   // (the entries refuse such a view: never taken)
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = table[12 * (int64_t)view + i];
    const int64_t quads = n_pix >> 2, stride = (int64_t)gridDim.x * kExpThreads;
    const float4* __restrict__ in4 = reinterpret_cast<const float4*>(render);
    float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
    for (int64_t q = (int64_t)blockIdx.x * kExpThreads + threadIdx.x; q < quads; q += stride) {
        const float4 a = in4[3 * q], b = in4[3 * q + 1], c = in4[3 * q + 2];
        float4 oa, ob, oc;
        exposure_apply(T, a.x, a.y, a.z, oa.x, oa.y, oa.z);
        exposure_apply(T, a.w, b.x, b.y, oa.w, ob.x, ob.y);
        exposure_apply(T, b.z, b.w, c.x, ob.z, ob.w, oc.x);
        exposure_apply(T, c.y, c.z, c.w, oc.y, oc.z, oc.w);
        out4[3 * q] = oa; out4[3 * q + 1] = ob; out4[3 * q + 2] = oc;
    }
    const int64_t p = 4 * quads + threadIdx.x;   // the tail: fewer than 4 pixels
    if (blockIdx.x == 0 && p < n_pix)
        exposure_apply(T, render[3 * p], render[3 * p + 1], render[3 * p + 2], out[3 * p], out[3 * p + 1], out[3 * p + 2]);
}

__device__ __forceinline__ double wave_reduce_add_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kExpThreads) void exposure_bwd_kernel(int64_t n_pix, int n_views, const float* __restrict__ rec, int view_arg,
                                                                    const float* __restrict__ table, const float* __restrict__ render,
                                                                    float* __restrict__ v_image, double* __restrict__ partials) {
    __shared__ double wsum[kExpThreads / kWave][12];
    const int view = exposure_view(rec, view_arg);
    if ((unsigned)view >= (unsigned)n_views) return;
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = table[12 * (int64_t)view + i];
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    const int64_t quads = n_pix >> 2, stride = (int64_t)gridDim.x * kExpThreads;
    const float4* __restrict__ in4 = reinterpret_cast<const float4*>(render);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v_image);
    for (int64_t q = (int64_t)blockIdx.x * kExpThreads + threadIdx.x; q < quads; q += stride) {
        const float4 a = in4[3 * q], b = in4[3 * q + 1], c = in4[3 * q + 2];
        const float4 va = v4[3 * q], vb = v4[3 * q + 1], vc = v4[3 * q + 2];
        float4 da, db, dc;
        exposure_accumulate(acc, va.x, va.y, va.z, a.x, a.y, a.z);
        exposure_vjp(T, va.x, va.y, va.z, da.x, da.y, da.z);
        exposure_accumulate(acc, va.w, vb.x, vb.y, a.w, b.x, b.y);
        exposure_vjp(T, va.w, vb.x, vb.y, da.w, db.x, db.y);
        exposure_accumulate(acc, vb.z, vb.w, vc.x, b.z, b.w, c.x);
        exposure_vjp(T, vb.z, vb.w, vc.x, db.z, db.w, dc.x);
        exposure_accumulate(acc, vc.y, vc.z, vc.w, c.y, c.z, c.w);
        exposure_vjp(T, vc.y, vc.z, vc.w, dc.y, dc.z, dc.w);
        v4[3 * q] = da; v4[3 * q + 1] = db; v4[3 * q + 2] = dc;
    }
    const int64_t p = 4 * quads + threadIdx.x;
    if (blockIdx.x == 0 && p < n_pix) {
        const float v0 = v_image[3 * p], v1 = v_image[3 * p + 1], v2 = v_image[3 * p + 2];
        exposure_accumulate(acc, v0, v1, v2, render[3 * p], render[3 * p + 1], render[3 * p + 2]);
        exposure_vjp(T, v0, v1, v2, v_image[3 * p], v_image[3 * p + 1], v_image[3 * p + 2]);
    }
    // lanes (xor butterfly), then the block's waves in order, then -- exposure_sums_kernel -- the blocks in order
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const double s = wave_reduce_add_f64(acc[i]);
        if (lane_id() == 0) wsum[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double s = wsum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kExpThreads / kWave; ++w) s += wsum[w][threadIdx.x];
        partials[12 * (int64_t)blockIdx.x + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kExpSumWaves * kWave) void exposure_sums_kernel(int n_blocks, const double* __restrict__ partials,
                                                                              float* __restrict__ v_affine12) {
    const int k = threadIdx.x >> 6;   // which of the 12 sums
    double s = 0.0;
    for (int blk = lane_id(); blk < n_blocks; blk += kWave) s += partials[12 * (int64_t)blk + k];
    s = wave_reduce_add_f64(s);
    if (lane_id() == 0) v_affine12[k] = (float)s;
}

__global__ __launch_bounds__(kExpThreads) void exposure_adam_kernel(int n_views, const float* __restrict__ rec, float* __restrict__ table,
                                                                     float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                                     const float* __restrict__ v_affine12, float b1, float b2, float eps,
                                                                     const int64_t* guard) {
    if (guard_tripped(guard)) return;
    const int view = exposure_view(rec, 0);
    if ((unsigned)view >= (unsigned)n_views) return;
    const float ss = rec[GS_EXPOSURE_REC_SS], isbc2 = rec[GS_EXPOSURE_REC_ISBC2];
    const int64_t total = 12 * (int64_t)n_views, stride = (int64_t)gridDim.x * kExpThreads;
    for (int64_t e = (int64_t)blockIdx.x * kExpThreads + threadIdx.x; e < total; e += stride) {
        const int64_t row = e / 12;
        const float g = row == view ? v_affine12[e - 12 * row] : 0.f;
        float p = table[e], m = exp_avg[e], v = exp_avg_sq[e];
        exposure_adam1(p, g, m, v, b1, b2, eps, isbc2, ss);
        table[e] = p; exp_avg[e] = m; exp_avg_sq[e] = v;
    }
}

}  // namespace gs

using namespace gs;

#define GS_EXP_IMAGE_ARGS(n_views)                                                                                                  \
    GS_REQUIRE(height > 0 && width > 0, "height > 0 and width > 0");                                                                \
    GS_REQUIRE(n_views >= 1 && n_views <= GS_EXPOSURE_MAX_VIEWS, "1 <= n_views <= GS_EXPOSURE_MAX_VIEWS");                          \
    GS_REQUIRE(rec_dev != nullptr || (view >= 0 && view < n_views), "without a record: 0 <= view < n_views")

extern "C" int gs_exposure_step_inputs(void* stream, int view, int n_views, float lr, float beta1, float beta2, int64_t step, float* rec_dev) {
    GS_REQUIRE(n_views >= 1 && n_views <= GS_EXPOSURE_MAX_VIEWS && view >= 0 && view < n_views, "0 <= view < n_views <= GS_EXPOSURE_MAX_VIEWS");
    GS_REQUIRE(step >= 1, "step counts from 1");
    GS_REQUIRE(rec_dev != nullptr && ((uintptr_t)rec_dev & 15) == 0, "rec_dev: non-null, 16-byte aligned");
    GS_REQUIRE(lr == lr && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "lr is NaN, or a beta outside [0, 1)");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    ExposureStepRec r = {};
    r.v[GS_EXPOSURE_REC_SS] = (float)((double)lr / bc1);   // (gs_step_inputs' host arithmetic)
    r.v[GS_EXPOSURE_REC_ISBC2] = (float)(1.0 / sqrt(bc2));
    memcpy(&r.v[GS_EXPOSURE_REC_VIEW], &view, sizeof(int));
    hipLaunchKernelGGL(exposure_step_inputs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, r, rec_dev);
    GS_LAUNCH_CHECK("exposure_step_inputs_kernel");
    return GS_OK;
}

extern "C" int gs_exposure_apply(void* stream, int height, int width, int n_views, const float* rec_dev, int view, const float* table,
                                 const float* render, float* out) {
    GS_EXP_IMAGE_ARGS(n_views);
    GS_REQUIRE(table && render && out && render != out, "null pointer, or out aliases render");
    GS_REQUIRE((((uintptr_t)render | (uintptr_t)out) & 15) == 0, "images must be 16-byte aligned");
    const int64_t n_pix = (int64_t)height * width;
    hipLaunchKernelGGL(exposure_apply_kernel, dim3(exposure_blocks(n_pix)), dim3(kExpThreads), 0, (hipStream_t)stream, n_pix, n_views, rec_dev,
                       view, table, render, out);
    GS_LAUNCH_CHECK("exposure_apply_kernel");
    return GS_OK;
}

extern "C" size_t gs_exposure_partials_doubles(int height, int width) {
    if (height <= 0 || width <= 0) return 0;
    return 12 * (size_t)exposure_blocks((int64_t)height * width);
}

extern "C" int gs_exposure_bwd(void* stream, int height, int width, int n_views, const float* rec_dev, int view, const float* table,
                               const float* render, float* v_image, double* partials, float* v_affine12) {
    GS_EXP_IMAGE_ARGS(n_views);
    GS_REQUIRE(table && render && v_image && partials && v_affine12 && render != v_image, "null pointer, or v_image aliases render");
    GS_REQUIRE((((uintptr_t)render | (uintptr_t)v_image) & 15) == 0 && ((uintptr_t)partials & 7) == 0, "images must be 16-byte aligned");
    const int64_t n_pix = (int64_t)height * width;
    const int blocks = exposure_blocks(n_pix);
    hipLaunchKernelGGL(exposure_bwd_kernel, dim3(blocks), dim3(kExpThreads), 0, (hipStream_t)stream, n_pix, n_views, rec_dev, view, table,
                       render, v_image, partials);
    GS_LAUNCH_CHECK("exposure_bwd_kernel");
    hipLaunchKernelGGL(exposure_sums_kernel, dim3(1), dim3(kExpSumWaves * kWave), 0, (hipStream_t)stream, blocks, partials, v_affine12);
    GS_LAUNCH_CHECK("exposure_sums_kernel");
    return GS_OK;
}

extern "C" int gs_exposure_adam(void* stream, int n_views, const float* rec_dev, float* table, float* exp_avg, float* exp_avg_sq,
                                const float* v_affine12, float beta1, float beta2, float eps) {
    GS_REQUIRE(n_views >= 1 && n_views <= GS_EXPOSURE_MAX_VIEWS, "1 <= n_views <= GS_EXPOSURE_MAX_VIEWS");
    GS_REQUIRE(rec_dev && table && exp_avg && exp_avg_sq && v_affine12, "null pointer");
    const int64_t blocks = (12 * (int64_t)n_views + kExpThreads - 1) / kExpThreads;
    hipLaunchKernelGGL(exposure_adam_kernel, dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(kExpThreads), 0, (hipStream_t)stream, n_views,
                       rec_dev, table, exp_avg, exp_avg_sq, v_affine12, beta1, beta2, eps, current_guard().info);
    GS_LAUNCH_CHECK("exposure_adam_kernel");
    return GS_OK;
}
