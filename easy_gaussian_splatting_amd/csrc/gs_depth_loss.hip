// gs_depth_loss.hip -- depth supervision (include/gs_raster.h "Depth supervision"; DESIGN.md "Depth supervision in the captured
// step"): the math is gs_depth_loss.h, shared with the host tests, and gs_math.h's expected_depth / expected_depth_vjp.
//   depth_step_inputs_kernel   {lambda_depth, mode, the target's address} of the step about to run into a device record: one wave,
//                              four lanes write; in front of the step's guarded sequence, so it does not look at the guard
//   depth_loss_fwd_kernel      <SPLIT>: the [H,W,4] blend into the [H,W,3] image and the expected-depth map, and the pixels' terms
//                              of sum(w |e|) and sum(w) in fp64 as per-block partials: 40 B per pixel (24 read, 16 written; 4 more
//                              with a mask); <!SPLIT>: the terms alone, from a depth map (the eager form)
//   depth_loss_finish_kernel   (behind the image loss's forward, which writes loss3) the partials in block order, value and
//                              1 / sum(w) rounded to fp32 once into the record, loss3[2] += lambda_depth * value
//   depth_loss_bwd_kernel      <JOIN>: v_render [H,W,3] and the depth term's gradient through expected_depth_vjp into
//                              v_colors [H,W,4] and v_alphas [H,W]: 60 B per pixel (40 read, 20 written); <!JOIN>: the gradient of the depth map alone
// The image kernels are gs_exposure.hip's: 256-thread blocks, a thread takes 4 pixels with 16-byte accesses, grid-stride from a
// capped block count; the H*W % 4 pixels left over are block 0's first threads'.  No atomics anywhere.
#include "gs_common.h"
#include "gs_math.h"
#include "gs_depth_loss.h"

namespace gs {

constexpr int kDlThreads = 256;
constexpr int kDlMaxBlocks = 1024;   // 4 blocks on each of 256 CUs; a frame beyond 1 M pixels strides

struct DepthStepRec { float v[4]; };   // the words gs_depth_step_inputs owns: lambda, mode, the address (two words)

__global__ void depth_step_inputs_kernel(const DepthStepRec r, float* __restrict__ rec) {
    const unsigned t = threadIdx.x;
    if (t < 4u) rec[t] = r.v[t];
}

static inline int depth_loss_blocks(int64_t n_pix) {
    const int64_t quads = n_pix >> 2, blocks = (quads + kDlThreads - 1) / kDlThreads;
    return (int)(blocks < 1 ? 1 : (blocks > kDlMaxBlocks ? kDlMaxBlocks : blocks));
}

struct DepthLossArgs {
    int64_t n_pix;
    float* rec;                 // value and 1 / sum(w) live here; staged: lambda, mode and the target's address too
    int staged;                 // {lambda, mode, target} come from the record (gs_depth_step_inputs), not from the three below
    float lambda;
    int mode;
    const float* target;        // [H,W]
    const float* mask;          // [H,W] or nullptr
    const int64_t* img_slots;   // {gt, mask} addresses of the step (gs_step_inputs) or nullptr: the mask is slot 1
    const float* colors4;       // [H,W,4] the blend: {r, g, b, accumulated depth}
    const float* alphas;        // [H,W]
    float* image3;              // [H,W,3]
    float* depth;               // [H,W]  written (SPLIT / never by the backward), read otherwise
    const float* v_render;      // [H,W,3]
    const float* v_loss;        // the upstream gradient of the value, one float on the device
    float* v_colors4;           // [H,W,4]
    float* v_out;               // v_alphas [H,W] (JOIN) or v_depth [H,W]
    double* partials;
    float* loss3;
    int blocks;
    const int64_t* guard;
};

struct DepthLossView { int mode; float lambda; const float* target; const float* mask; };

__device__ __forceinline__ DepthLossView depth_loss_view(const DepthLossArgs& a) {
    DepthLossView v;
    v.mode = a.mode; v.lambda = a.lambda; v.target = a.target;
    if (a.staged) {
        v.lambda = a.rec[GS_DEPTH_REC_LAMBDA];
        v.mode = __float_as_int(a.rec[GS_DEPTH_REC_MODE]);
        v.target = reinterpret_cast<const float*>(*reinterpret_cast<const uint64_t*>(a.rec + GS_DEPTH_REC_TARGET));
    }
    v.mask = a.img_slots ? reinterpret_cast<const float*>(a.img_slots[1]) : a.mask;
    return v;
}

__device__ __forceinline__ float4 mask_quad(const float* __restrict__ mask, int64_t q) {   // (4-byte aligned: scalar loads)
    if (mask == nullptr) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(mask[4 * q], mask[4 * q + 1], mask[4 * q + 2], mask[4 * q + 3]);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool SPLIT>
__global__ __launch_bounds__(kDlThreads) void depth_loss_fwd_kernel(const DepthLossArgs a) {
    __shared__ double wsum[kDlThreads / kWave][2];
    if (guard_tripped(a.guard)) return;
    const DepthLossView s = depth_loss_view(a);
    double acc[2] = {0.0, 0.0};
    const int64_t quads = a.n_pix >> 2, stride = (int64_t)gridDim.x * kDlThreads;
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(s.target);
    for (int64_t q = (int64_t)blockIdx.x * kDlThreads + threadIdx.x; q < quads; q += stride) {
        const float4 t = t4[q], m = mask_quad(s.mask, q);
        float4 d;
        if (SPLIT) {
            const float4* __restrict__ c4 = reinterpret_cast<const float4*>(a.colors4);
            const float4 c0 = c4[4 * q], c1 = c4[4 * q + 1], c2 = c4[4 * q + 2], c3 = c4[4 * q + 3];
            const float4 al = reinterpret_cast<const float4*>(a.alphas)[q];
            d = make_float4(expected_depth(c0.w, al.x), expected_depth(c1.w, al.y), expected_depth(c2.w, al.z), expected_depth(c3.w, al.w));
            float4* __restrict__ o4 = reinterpret_cast<float4*>(a.image3);
            o4[3 * q] = make_float4(c0.x, c0.y, c0.z, c1.x);
            o4[3 * q + 1] = make_float4(c1.y, c1.z, c2.x, c2.y);
            o4[3 * q + 2] = make_float4(c2.z, c3.x, c3.y, c3.z);
            reinterpret_cast<float4*>(a.depth)[q] = d;
        } else {
            d = reinterpret_cast<const float4*>(a.depth)[q];
        }
        depth_loss_accumulate(acc, s.mode, d.x, t.x, m.x);
        depth_loss_accumulate(acc, s.mode, d.y, t.y, m.y);
        depth_loss_accumulate(acc, s.mode, d.z, t.z, m.z);
        depth_loss_accumulate(acc, s.mode, d.w, t.w, m.w);
    }
    const int64_t p = 4 * quads + threadIdx.x;   // the tail: fewer than 4 pixels
    if (blockIdx.x == 0 && p < a.n_pix) {
        float d;
        if (SPLIT) {
            d = expected_depth(a.colors4[4 * p + 3], a.alphas[p]);
            a.image3[3 * p] = a.colors4[4 * p]; a.image3[3 * p + 1] = a.colors4[4 * p + 1]; a.image3[3 * p + 2] = a.colors4[4 * p + 2];
            a.depth[p] = d;
        } else {
            d = a.depth[p];
        }
        depth_loss_accumulate(acc, s.mode, d, s.target[p], s.mask ? s.mask[p] : 0.f);
    }
    // lanes (xor butterfly), then the block's waves in order, then -- depth_loss_finish_kernel -- the blocks in order
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double t = wave_sum_f64(acc[i]);
        if (lane_id() == 0) wsum[wave][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = wsum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kDlThreads / kWave; ++w) t += wsum[w][threadIdx.x];
        a.partials[2 * (int64_t)blockIdx.x + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(2 * kWave) void depth_loss_finish_kernel(const DepthLossArgs a) {
    __shared__ double sums[2];
    if (guard_tripped(a.guard)) return;
    const int k = threadIdx.x >> 6;   // which of the two sums
    double t = 0.0;
    for (int blk = lane_id(); blk < a.blocks; blk += kWave) t += a.partials[2 * (int64_t)blk + k];
    t = wave_sum_f64(t);
    if (lane_id() == 0) sums[k] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        float value, inv_w;
        depth_loss_finish(sums[0], sums[1], value, inv_w);
        a.rec[GS_DEPTH_REC_VALUE] = value;
        a.rec[GS_DEPTH_REC_INV_W] = inv_w;
        // the eager total: total + lambda * value, the product rounded on its own (as gs_scale_reg enters it)
        if (a.loss3 != nullptr) a.loss3[2] = a.loss3[2] + fp_opaque(depth_loss_view(a).lambda * value);
    }
}

template <bool JOIN>
__global__ __launch_bounds__(kDlThreads) void depth_loss_bwd_kernel(const DepthLossArgs a) {
    if (guard_tripped(a.guard)) return;
    const DepthLossView s = depth_loss_view(a);
    // the upstream gradient of the value (the step: lambda_depth) times 1 / sum(w), rounded once
    const float scale = fp_opaque((JOIN ? s.lambda : a.v_loss[0]) * a.rec[GS_DEPTH_REC_INV_W]);
    const int64_t quads = a.n_pix >> 2, stride = (int64_t)gridDim.x * kDlThreads;
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(s.target);
    const float4* __restrict__ d4 = reinterpret_cast<const float4*>(a.depth);
    for (int64_t q = (int64_t)blockIdx.x * kDlThreads + threadIdx.x; q < quads; q += stride) {
        const float4 t = t4[q], m = mask_quad(s.mask, q), d = d4[q];
        const float4 g = make_float4(depth_loss_grad(s.mode, d.x, t.x, m.x, scale), depth_loss_grad(s.mode, d.y, t.y, m.y, scale),
                                     depth_loss_grad(s.mode, d.z, t.z, m.z, scale), depth_loss_grad(s.mode, d.w, t.w, m.w, scale));
        if (JOIN) {
            const float4* __restrict__ c4 = reinterpret_cast<const float4*>(a.colors4);
            const float4* __restrict__ v4 = reinterpret_cast<const float4*>(a.v_render);
            const float4 al = reinterpret_cast<const float4*>(a.alphas)[q];
            const float4 va = v4[3 * q], vb = v4[3 * q + 1], vc = v4[3 * q + 2];
            float4 vz, val;
            expected_depth_vjp(g.x, c4[4 * q].w, al.x, vz.x, val.x);
            expected_depth_vjp(g.y, c4[4 * q + 1].w, al.y, vz.y, val.y);
            expected_depth_vjp(g.z, c4[4 * q + 2].w, al.z, vz.z, val.z);
            expected_depth_vjp(g.w, c4[4 * q + 3].w, al.w, vz.w, val.w);
            float4* __restrict__ o4 = reinterpret_cast<float4*>(a.v_colors4);
            o4[4 * q] = make_float4(va.x, va.y, va.z, vz.x);
            o4[4 * q + 1] = make_float4(va.w, vb.x, vb.y, vz.y);
            o4[4 * q + 2] = make_float4(vb.z, vb.w, vc.x, vz.z);
            o4[4 * q + 3] = make_float4(vc.y, vc.z, vc.w, vz.w);
            reinterpret_cast<float4*>(a.v_out)[q] = val;
        } else {
            reinterpret_cast<float4*>(a.v_out)[q] = g;
        }
    }
    const int64_t p = 4 * quads + threadIdx.x;
    if (blockIdx.x == 0 && p < a.n_pix) {
        const float g = depth_loss_grad(s.mode, a.depth[p], s.target[p], s.mask ? s.mask[p] : 0.f, scale);
        if (JOIN) {
            float vz, val;
            expected_depth_vjp(g, a.colors4[4 * p + 3], a.alphas[p], vz, val);
            a.v_colors4[4 * p] = a.v_render[3 * p]; a.v_colors4[4 * p + 1] = a.v_render[3 * p + 1];
            a.v_colors4[4 * p + 2] = a.v_render[3 * p + 2]; a.v_colors4[4 * p + 3] = vz;
            a.v_out[p] = val;
        } else {
            a.v_out[p] = g;
        }
    }
}

}  // namespace gs

using namespace gs;

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define GS_DL_COMMON_ARGS()                                                                                                          \
    GS_REQUIRE(height > 0 && width > 0, "height > 0 and width > 0");                                                                 \
    GS_REQUIRE(rec_dev != nullptr && aligned16(rec_dev), "rec_dev: non-null, 16-byte aligned");                                      \
    GS_REQUIRE(target == nullptr || (mode == GS_DEPTH_MODE_DEPTH || mode == GS_DEPTH_MODE_DISPARITY), "mode: GS_DEPTH_MODE_*");      \
    GS_REQUIRE(aligned16(target) && ((uintptr_t)mask & 3) == 0, "target 16-byte, mask 4-byte aligned")

extern "C" int gs_depth_step_inputs(void* stream, float lambda_depth, int mode, const float* target, float* rec_dev) {
    GS_REQUIRE(lambda_depth == lambda_depth, "lambda_depth is NaN");
    GS_REQUIRE(mode == GS_DEPTH_MODE_DEPTH || mode == GS_DEPTH_MODE_DISPARITY, "mode: GS_DEPTH_MODE_DEPTH or GS_DEPTH_MODE_DISPARITY");
    GS_REQUIRE(target != nullptr && aligned16(target), "target: non-null, 16-byte aligned");
    GS_REQUIRE(rec_dev != nullptr && aligned16(rec_dev), "rec_dev: non-null, 16-byte aligned");
    DepthStepRec r = {};
    const uint64_t addr = (uint64_t)(uintptr_t)target;
    r.v[GS_DEPTH_REC_LAMBDA] = lambda_depth;
    memcpy(&r.v[GS_DEPTH_REC_MODE], &mode, sizeof(int));
    memcpy(&r.v[GS_DEPTH_REC_TARGET], &addr, sizeof(uint64_t));
    hipLaunchKernelGGL(depth_step_inputs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, r, rec_dev);
    GS_LAUNCH_CHECK("depth_step_inputs_kernel");
    return GS_OK;
}

extern "C" size_t gs_depth_loss_partials_doubles(int height, int width) {
    if (height <= 0 || width <= 0) return 0;
    return 2 * (size_t)depth_loss_blocks((int64_t)height * width);
}

static DepthLossArgs depth_loss_args(int height, int width, float* rec_dev, float lambda_depth, int mode, const float* target,
                                     const float* mask, const int64_t* img_slots) {
    DepthLossArgs a = {};
    a.n_pix = (int64_t)height * width; a.rec = rec_dev; a.lambda = lambda_depth; a.mode = mode; a.target = target; a.mask = mask;
    a.staged = target == nullptr; a.img_slots = img_slots; a.blocks = depth_loss_blocks(a.n_pix); a.guard = current_guard().info;
    return a;
}

extern "C" int gs_depth_loss_split(void* stream, int height, int width, float* rec_dev, float lambda_depth, int mode, const float* target,
                                   const float* mask, const int64_t* img_slots, const float* colors4, const float* alphas, float* image3,
                                   float* depth, double* partials) {
    GS_DL_COMMON_ARGS();
    GS_REQUIRE(colors4 && alphas && image3 && depth && partials, "null pointer");
    GS_REQUIRE(aligned16(colors4) && aligned16(alphas) && aligned16(image3) && aligned16(depth) && ((uintptr_t)partials & 7) == 0,
               "images must be 16-byte aligned");
    GS_REQUIRE((const void*)image3 != (const void*)colors4 && (const void*)depth != (const void*)alphas, "an output aliases an input");
    DepthLossArgs a = depth_loss_args(height, width, rec_dev, lambda_depth, mode, target, mask, img_slots);
    a.colors4 = colors4; a.alphas = alphas; a.image3 = image3; a.depth = depth; a.partials = partials;
    hipLaunchKernelGGL(depth_loss_fwd_kernel<true>, dim3(a.blocks), dim3(kDlThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_loss_fwd_kernel (split)");
    return GS_OK;
}

extern "C" int gs_depth_loss_finish(void* stream, int height, int width, float* rec_dev, float lambda_depth, int staged,
                                    const double* partials, float* loss3) {
    GS_REQUIRE(height > 0 && width > 0, "height > 0 and width > 0");
    GS_REQUIRE(rec_dev != nullptr && aligned16(rec_dev), "rec_dev: non-null, 16-byte aligned");
    GS_REQUIRE(partials != nullptr && ((uintptr_t)partials & 7) == 0 && ((uintptr_t)loss3 & 3) == 0, "partials: non-null, 8-byte aligned; loss3 4-byte");
    GS_REQUIRE(staged == 0 || staged == 1, "staged is 0 or 1");
    GS_REQUIRE(staged || lambda_depth == lambda_depth, "lambda_depth is NaN");
    DepthLossArgs a = depth_loss_args(height, width, rec_dev, lambda_depth, 0, nullptr, nullptr, nullptr);
    a.staged = staged; a.partials = const_cast<double*>(partials); a.loss3 = loss3;
    hipLaunchKernelGGL(depth_loss_finish_kernel, dim3(1), dim3(2 * kWave), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_loss_finish_kernel");
    return GS_OK;
}

extern "C" int gs_depth_loss_fwd(void* stream, int height, int width, float* rec_dev, int mode, const float* target, const float* mask,
                                 const float* depth, double* partials) {
    GS_DL_COMMON_ARGS();
    GS_REQUIRE(target && depth && partials, "null pointer");
    GS_REQUIRE(aligned16(depth) && ((uintptr_t)partials & 7) == 0, "depth must be 16-byte, partials 8-byte aligned");
    DepthLossArgs a = depth_loss_args(height, width, rec_dev, 0.f, mode, target, mask, nullptr);
    a.depth = const_cast<float*>(depth); a.partials = partials;
    hipLaunchKernelGGL(depth_loss_fwd_kernel<false>, dim3(a.blocks), dim3(kDlThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_loss_fwd_kernel");
    hipLaunchKernelGGL(depth_loss_finish_kernel, dim3(1), dim3(2 * kWave), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_loss_finish_kernel");
    return GS_OK;
}

extern "C" int gs_depth_loss_join(void* stream, int height, int width, const float* rec_dev, float lambda_depth, int mode,
                                  const float* target, const float* mask, const int64_t* img_slots, const float* colors4,
                                  const float* alphas, const float* depth, const float* v_render, float* v_colors4, float* v_alphas) {
    GS_DL_COMMON_ARGS();
    GS_REQUIRE(colors4 && alphas && depth && v_render && v_colors4 && v_alphas, "null pointer");
    GS_REQUIRE(aligned16(colors4) && aligned16(alphas) && aligned16(depth) && aligned16(v_render) && aligned16(v_colors4) && aligned16(v_alphas),
               "images must be 16-byte aligned");
    GS_REQUIRE((const void*)v_colors4 != (const void*)v_render && (const void*)v_colors4 != (const void*)colors4 &&
               (const void*)v_alphas != (const void*)alphas && (const void*)v_alphas != (const void*)depth, "an output aliases an input");
    DepthLossArgs a = depth_loss_args(height, width, const_cast<float*>(rec_dev), lambda_depth, mode, target, mask, img_slots);
    a.colors4 = colors4; a.alphas = alphas; a.depth = const_cast<float*>(depth); a.v_render = v_render; a.v_colors4 = v_colors4; a.v_out = v_alphas;
    hipLaunchKernelGGL(depth_loss_bwd_kernel<true>, dim3(a.blocks), dim3(kDlThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_loss_bwd_kernel (join)");
    return GS_OK;
}

extern "C" int gs_depth_loss_bwd(void* stream, int height, int width, const float* rec_dev, int mode, const float* target, const float* mask,
                                 const float* depth, const float* v_loss, float* v_depth) {
    GS_DL_COMMON_ARGS();
    GS_REQUIRE(target && depth && v_loss && v_depth, "null pointer");
    GS_REQUIRE(aligned16(depth) && aligned16(v_depth) && ((uintptr_t)v_loss & 3) == 0, "depth and v_depth must be 16-byte aligned");
    DepthLossArgs a = depth_loss_args(height, width, const_cast<float*>(rec_dev), 0.f, mode, target, mask, nullptr);
    a.depth = const_cast<float*>(depth); a.v_loss = v_loss; a.v_out = v_depth;
    hipLaunchKernelGGL(depth_loss_bwd_kernel<false>, dim3(a.blocks), dim3(kDlThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("depth_loss_bwd_kernel");
    return GS_OK;
}
