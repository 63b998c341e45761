// gs_pose.hip -- pose refinement inside the captured train step (include/gs_raster.h "Pose refinement in the captured step";
// DESIGN.md "Poses in the captured step"): the math is gs_pose.h, fp64, shared with the host tests.
//   pose_step_inputs_kernel  {raw w2c, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), view} of the step about to run into a device
//                            record (values travel as kernel arguments)
//   pose_compose_kernel      viewmats[0] = [[exp([omega]x), tau], [0, 1]] @ w2c for the record's view, in front of the projection
//   pose_adam_kernel         behind cam_sum_kernel: the chain from the view matrix' gradient to the 6-vector (v_delta), then DENSE
//                            Adam over all n_views x 6 corrections -- v_delta on the view's row, 0 on every other --, under the guard
#include "gs_common.h"
#include "gs_pose.h"

namespace gs {

struct PoseStepRec { float v[GS_POSE_REC_FLOATS]; int has_w2c; };

__global__ void pose_step_inputs_kernel(const PoseStepRec r, const float* __restrict__ w2c_src, float* __restrict__ rec) {
    const unsigned t = threadIdx.x;
    if (t < 16u) {
        if (w2c_src) rec[t] = w2c_src[t];
        else if (r.has_w2c) rec[t] = r.v[t];
    } else if (t < (unsigned)GS_POSE_REC_FLOATS) {
        rec[t] = r.v[t];
    }
}

__device__ __forceinline__ int pose_view(const float* rec) { return __float_as_int(rec[GS_POSE_REC_VIEW]); }

__global__ void pose_compose_kernel(int n_views, const float* __restrict__ rec, const float* __restrict__ deltas,
                                    float* __restrict__ viewmat) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int view = pose_view(rec);
    if ((unsigned)view >= (unsigned)n_views) return;   // (gs_pose_step_inputs refuses such a record: never taken)
    float d[6], w[16], out[16];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = deltas[6 * (int64_t)view + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = rec[i];
    pose_compose(d, w, out);
#pragma unroll
    for (int i = 0; i < 16; ++i) viewmat[i] = out[i];
}

constexpr int kPoseAdamThreads = 256;

__global__ __launch_bounds__(kPoseAdamThreads) void pose_adam_kernel(int n_views, const float* __restrict__ rec, float* deltas,
                                                                     float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                                     const float* __restrict__ v_viewmats, const float* __restrict__ v_campos,
                                                                     float* __restrict__ v_delta_out, float b1, float b2, float eps,
                                                                     const int64_t* guard) {
    __shared__ float g6[6];
    if (guard_tripped(guard)) return;
    const int view = pose_view(rec);
    if ((unsigned)view >= (unsigned)n_views) return;
    if (threadIdx.x == 0) {   // (the view's row is read here, before any thread writes it: the barrier below)
        double d[6], vA[9], vt[3], vc[3], vd[6];
        float w[16];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = (double)deltas[6 * (int64_t)view + i];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = rec[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) vA[3 * i + j] = (double)v_viewmats[4 * i + j];
            vt[i] = (double)v_viewmats[4 * i + 3];
            vc[i] = (double)v_campos[i];
        }
        pose_vjp(d, w, vA, vt, vc, vd);
#pragma unroll
        for (int i = 0; i < 6; ++i) { g6[i] = (float)vd[i]; v_delta_out[i] = (float)vd[i]; }
    }
    __syncthreads();
    const float ss = rec[GS_POSE_REC_SS], isbc2 = rec[GS_POSE_REC_ISBC2];
    const int total = 6 * n_views;
    for (int e = threadIdx.x; e < total; e += kPoseAdamThreads) {
        const int row = e / 6, k = e - 6 * row;
        const float g = row == view ? g6[k] : 0.f;
        float p = deltas[e], m = exp_avg[e], v = exp_avg_sq[e];
        adam1(p, g, m, v, b1, b2, eps, isbc2, ss);
        deltas[e] = p; exp_avg[e] = m; exp_avg_sq[e] = v;
    }
}

}  // namespace gs

using namespace gs;

extern "C" int gs_pose_step_inputs(void* stream, int view, int n_views, const float* w2c_dev, const float* w2c_host, float lr,
                                   float beta1, float beta2, int64_t step, float* rec_dev) {
    GS_REQUIRE(n_views >= 1 && n_views <= GS_POSE_MAX_VIEWS && view >= 0 && view < n_views, "0 <= view < n_views <= GS_POSE_MAX_VIEWS");
    GS_REQUIRE(step >= 1, "step counts from 1");
    GS_REQUIRE(!(w2c_dev && w2c_host), "the raw view matrix: a device pointer or host values, not both");
    GS_REQUIRE(rec_dev != nullptr && ((uintptr_t)rec_dev & 15) == 0, "rec_dev: non-null, 16-byte aligned");
    GS_REQUIRE(lr == lr && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "lr is NaN, or a beta outside [0, 1)");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    PoseStepRec r = {};
    if (w2c_host) { memcpy(r.v, w2c_host, 16 * sizeof(float)); r.has_w2c = 1; }
    r.v[GS_POSE_REC_SS] = (float)((double)lr / bc1);   // (gs_step_inputs' host arithmetic)
    r.v[GS_POSE_REC_ISBC2] = (float)(1.0 / sqrt(bc2));
    memcpy(&r.v[GS_POSE_REC_VIEW], &view, sizeof(int));
    // values travel as kernel arguments (copied at launch): no host buffer that a later call could overwrite
    hipLaunchKernelGGL(pose_step_inputs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, r, w2c_dev, rec_dev);
    GS_LAUNCH_CHECK("pose_step_inputs_kernel");
    return GS_OK;
}

extern "C" int gs_pose_compose(void* stream, int n_views, const float* rec_dev, const float* deltas, float* viewmat_out) {
    GS_REQUIRE(n_views >= 1 && n_views <= GS_POSE_MAX_VIEWS, "1 <= n_views <= GS_POSE_MAX_VIEWS");
    GS_REQUIRE(rec_dev && deltas && viewmat_out, "null pointer");
    hipLaunchKernelGGL(pose_compose_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, n_views, rec_dev, deltas, viewmat_out);
    GS_LAUNCH_CHECK("pose_compose_kernel");
    return GS_OK;
}

extern "C" int gs_pose_adam(void* stream, int n_views, const float* rec_dev, float* deltas, float* exp_avg, float* exp_avg_sq,
                            const float* v_viewmats, const float* v_campos, float* v_delta, float beta1, float beta2, float eps) {
    GS_REQUIRE(n_views >= 1 && n_views <= GS_POSE_MAX_VIEWS, "1 <= n_views <= GS_POSE_MAX_VIEWS");
    GS_REQUIRE(rec_dev && deltas && exp_avg && exp_avg_sq && v_viewmats && v_campos && v_delta, "null pointer");
    hipLaunchKernelGGL(pose_adam_kernel, dim3(1), dim3(kPoseAdamThreads), 0, (hipStream_t)stream, n_views, rec_dev, deltas, exp_avg,
                       exp_avg_sq, v_viewmats, v_campos, v_delta, beta1, beta2, eps, current_guard().info);
    GS_LAUNCH_CHECK("pose_adam_kernel");
    return GS_OK;
}
