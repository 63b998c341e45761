// gs_scale_reg.hip -- the scale-ratio regulariser of the reference's GaussianModel (use_scale_regularization) for gfx950:
//   scale_reg_kernel   : per Gaussian the term max(max_k s_k / min_k s_k, R) - R (gs_common.h scale_reg_term), summed per block in
//                        fp64 in a fixed order; optionally its gradient added to v_log_scales
//   scale_reg_finish   : one block sums the block partials in a fixed order, writes reg = sum / N and adds lambda * reg to the
//                        loss total
// No float atomics anywhere: two runs of the same inputs give the same bits (replays of a captured step included).
// The fused form -- the gradient added to v_scale inside the projection backward + Adam -- is project_bwd_kernel<D, true, false,
// true> (gs_project.hip); this pass then runs for the value only, in front of it, on the parameters before the update.
//
// The budget regulariser of mcmc.MCMCStrategy (a mean(opacity) + b mean(scale), gs_mcmc_reg) follows the same contract with the
// same two-stage fixed-order sum:
//   budget_reg_kernel  : per Gaussian o and s_0 + s_1 + s_2 in fp64 (gs_common.h budget_reg_term), two block partials; optionally
//                        the gradients added to v_logit_opacities / v_log_scales
//   budget_reg_finish  : reg = a sum_o / N + b sum_s / (3 N), rounded once, added to the loss total
// Its fused form is project_bwd_budget_kernel.
#include "gs_common.h"

namespace gs {

constexpr int kRegThreads = 256;
constexpr int kRegFinishThreads = 1024;

struct ScaleRegArgs {
    int64_t N;
    const float* log_scales;   // [N, 3]
    float R, g, lam;           // the free ratio, the upstream gradient of one term (lambda * (1 / N)), lambda
    float* v_log_scales;       // [N, 3] or nullptr
    double* partial;           // [blocks]
    float* reg;                // reg[0] = the regulariser's value
    float* loss3;              // {l1, 1 - ssim, total} or nullptr
    int64_t blocks;
    const int64_t* guard;
};

// a block's sum, always in the same order: a fixed butterfly inside each wave, then the waves in order
template <int THREADS>
__device__ __forceinline__ double block_sum_fixed(double v, double* lds) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        for (int w = 0; w < THREADS / 64; ++w) s += lds[w];
    }
    return s;   // (thread 0's)
}

template <bool GRAD>
__global__ __launch_bounds__(kRegThreads) void scale_reg_kernel(const ScaleRegArgs a) {
    __shared__ double lds[kRegThreads / 64];
    if (guard_tripped(a.guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kRegThreads + threadIdx.x;
    double t = 0.0;
    if (n < a.N) {
        const float* l = a.log_scales + 3 * n;
        float gl[3];
        t = (double)scale_reg_term(l[0], l[1], l[2], a.R, a.g, gl);
        if (GRAD) {
            float* v = a.v_log_scales + 3 * n;
            v[0] = fp_opaque(v[0]) + gl[0]; v[1] = fp_opaque(v[1]) + gl[1]; v[2] = fp_opaque(v[2]) + gl[2];
        }
    }
    const double s = block_sum_fixed<kRegThreads>(t, lds);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kRegFinishThreads) void scale_reg_finish(const ScaleRegArgs a) {
    __shared__ double lds[kRegFinishThreads / 64];
    if (guard_tripped(a.guard)) return;
    double t = 0.0;
    for (int64_t b = threadIdx.x; b < a.blocks; b += kRegFinishThreads) t += a.partial[b];
    const double s = block_sum_fixed<kRegFinishThreads>(t, lds);
    if (threadIdx.x == 0) {
        const float reg = (float)(s / (double)a.N);
        a.reg[0] = reg;
        // the eager total: total + lambda * reg, the product rounded on its own
        if (a.loss3 != nullptr) a.loss3[2] = a.loss3[2] + fp_opaque(a.lam * reg);
    }
}

struct BudgetRegArgs {
    int64_t N;
    const float *logit, *log_scales;   // [N], [N, 3]
    double a, b;
    float ga, gb;                      // fl32(a / N), fl32(b / (3 N)): the upstream gradient of one opacity, of one scale
    float *v_logit, *v_log_scales;     // [N], [N, 3], each may be nullptr
    double* partial;                   // [2 blocks]: the opacities' sums, then the scales'
    float* reg;
    float* loss3;
    int64_t blocks;
    const int64_t* guard;
};

__global__ __launch_bounds__(kRegThreads) void budget_reg_kernel(const BudgetRegArgs a) {
    __shared__ double lds_o[kRegThreads / 64], lds_s[kRegThreads / 64];
    if (guard_tripped(a.guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kRegThreads + threadIdx.x;
    double to = 0.0, ts = 0.0;
    if (n < a.N) {
        const float* l = a.log_scales + 3 * n;
        double s[3];
        float go, gl[3];
        budget_reg_term(a.logit[n], l[0], l[1], l[2], a.ga, a.gb, &to, s, &go, gl);
        ts = (s[0] + s[1]) + s[2];
        if (a.v_logit != nullptr) a.v_logit[n] = fp_opaque(a.v_logit[n]) + go;
        if (a.v_log_scales != nullptr) {
            float* v = a.v_log_scales + 3 * n;
            v[0] = fp_opaque(v[0]) + gl[0]; v[1] = fp_opaque(v[1]) + gl[1]; v[2] = fp_opaque(v[2]) + gl[2];
        }
    }
    const double so = block_sum_fixed<kRegThreads>(to, lds_o);
    const double ss = block_sum_fixed<kRegThreads>(ts, lds_s);
    if (threadIdx.x == 0) { a.partial[blockIdx.x] = so; a.partial[a.blocks + blockIdx.x] = ss; }
}

__global__ __launch_bounds__(kRegFinishThreads) void budget_reg_finish(const BudgetRegArgs a) {
    __shared__ double lds_o[kRegFinishThreads / 64], lds_s[kRegFinishThreads / 64];
    if (guard_tripped(a.guard)) return;
    double to = 0.0, ts = 0.0;
    for (int64_t b = threadIdx.x; b < a.blocks; b += kRegFinishThreads) { to += a.partial[b]; ts += a.partial[a.blocks + b]; }
    const double so = block_sum_fixed<kRegFinishThreads>(to, lds_o);
    const double ss = block_sum_fixed<kRegFinishThreads>(ts, lds_s);
    if (threadIdx.x == 0) {
        const float reg = (float)(a.a * (so / (double)a.N) + a.b * (ss / (3.0 * (double)a.N)));
        a.reg[0] = reg;
        if (a.loss3 != nullptr) a.loss3[2] = a.loss3[2] + reg;
    }
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_scale_reg_workspace_floats(int64_t N) {
    if (N <= 0) return 2;
    return 2 + 2 * (size_t)((N + kRegThreads - 1) / kRegThreads);
}

extern "C" int gs_scale_reg(void* stream, int64_t N, const float* log_scales, float max_ratio, float lambda, float* loss3,
                            float* reg_ws, float* v_log_scales) {
    GS_REQUIRE(N >= 0, "N >= 0");
    GS_REQUIRE(log_scales && reg_ws, "null pointer (log_scales, reg_ws)");
    GS_REQUIRE(((uintptr_t)reg_ws & 15) == 0, "reg_ws must be 16-byte aligned");
    GS_REQUIRE(((uintptr_t)log_scales & 3) == 0 && ((uintptr_t)loss3 & 3) == 0 && ((uintptr_t)v_log_scales & 3) == 0,
               "log_scales / loss3 / v_log_scales must be 4-byte aligned");
    if (N == 0) return GS_OK;
    ScaleRegArgs a;
    a.N = N; a.log_scales = log_scales; a.R = max_ratio; a.g = scale_reg_upstream(lambda, N); a.lam = lambda;
    a.v_log_scales = v_log_scales;
    a.partial = reinterpret_cast<double*>(reg_ws + 2);
    a.reg = reg_ws; a.loss3 = loss3;
    a.blocks = (N + kRegThreads - 1) / kRegThreads;
    a.guard = current_guard().info;
    hipStream_t st = (hipStream_t)stream;
    if (v_log_scales) hipLaunchKernelGGL(scale_reg_kernel<true>, dim3((unsigned)a.blocks), dim3(kRegThreads), 0, st, a);
    else hipLaunchKernelGGL(scale_reg_kernel<false>, dim3((unsigned)a.blocks), dim3(kRegThreads), 0, st, a);
    GS_LAUNCH_CHECK("scale_reg_kernel");
    hipLaunchKernelGGL(scale_reg_finish, dim3(1), dim3(kRegFinishThreads), 0, st, a);
    GS_LAUNCH_CHECK("scale_reg_finish");
    return GS_OK;
}

extern "C" size_t gs_mcmc_reg_workspace_floats(int64_t N) {
    if (N <= 0) return 2;
    return 2 + 4 * (size_t)((N + kRegThreads - 1) / kRegThreads);
}

extern "C" int gs_mcmc_reg(void* stream, int64_t N, const float* logit_opacities, const float* log_scales, double a, double b,
                           float* loss3, float* reg_ws, float* v_logit_opacities, float* v_log_scales) {
    GS_REQUIRE(N >= 0, "N >= 0");
    GS_REQUIRE(logit_opacities && log_scales && reg_ws, "null pointer (logit_opacities, log_scales, reg_ws)");
    GS_REQUIRE(a == a && b == b, "a or b is NaN");
    GS_REQUIRE(((uintptr_t)reg_ws & 15) == 0, "reg_ws must be 16-byte aligned");
    GS_REQUIRE(((uintptr_t)logit_opacities & 3) == 0 && ((uintptr_t)log_scales & 3) == 0 && ((uintptr_t)loss3 & 3) == 0 &&
               ((uintptr_t)v_logit_opacities & 3) == 0 && ((uintptr_t)v_log_scales & 3) == 0, "float arrays must be 4-byte aligned");
    if (N == 0) return GS_OK;
    BudgetRegArgs r;
    r.N = N; r.logit = logit_opacities; r.log_scales = log_scales; r.a = a; r.b = b;
    r.ga = budget_reg_upstream(a, N); r.gb = budget_reg_upstream(b, 3 * N);
    r.v_logit = v_logit_opacities; r.v_log_scales = v_log_scales;
    r.partial = reinterpret_cast<double*>(reg_ws + 2);
    r.reg = reg_ws; r.loss3 = loss3;
    r.blocks = (N + kRegThreads - 1) / kRegThreads;
    r.guard = current_guard().info;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(budget_reg_kernel, dim3((unsigned)r.blocks), dim3(kRegThreads), 0, st, r);
    GS_LAUNCH_CHECK("budget_reg_kernel");
    hipLaunchKernelGGL(budget_reg_finish, dim3(1), dim3(kRegFinishThreads), 0, st, r);
    GS_LAUNCH_CHECK("budget_reg_finish");
    return GS_OK;
}
