// gs_exposure.h -- the per-pixel math of exposure.ExposureTable (gs_exposure.hip; DESIGN.md "Exposure in the captured step"): a view's
// 3x4 colour affine T = [A | b], row-major, applied to one pixel, its transpose applied to one pixel's gradient, the pixel's terms of
// the 12 gradient sums, and the Adam update of one table entry.  Plain C++ that compiles for the device and for the host alike:
// tests/test_exposure_host.py builds it with the host compiler (tests/hostmath/exposuremath.cpp) and holds it to fp64 numpy.
// Every multiply-add is spelled fmaf: the order below is the order on both sides, whatever the compiler would contract.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD static inline
#endif

namespace gs {

// out_i = fma(A_i2, c_2, fma(A_i1, c_1, fma(A_i0, c_0, b_i))): three roundings per channel.  At [I | 0]: fma(1, c_i, 0) = c_i and
// every other term adds a zero -- the input comes back exactly (a -0 as +0).
GS_HD void exposure_apply(const float T[12], float c0, float c1, float c2, float& o0, float& o1, float& o2) {
    o0 = fmaf(T[2], c2, fmaf(T[1], c1, fmaf(T[0], c0, T[3])));
    o1 = fmaf(T[6], c2, fmaf(T[5], c1, fmaf(T[4], c0, T[7])));
    o2 = fmaf(T[10], c2, fmaf(T[9], c1, fmaf(T[8], c0, T[11])));
}

// (A^T v)_j = fma(A_2j, v_2, fma(A_1j, v_1, A_0j * v_0)): the forward's discipline, three roundings per channel
GS_HD void exposure_vjp(const float T[12], float v0, float v1, float v2, float& d0, float& d1, float& d2) {
    d0 = fmaf(T[8], v2, fmaf(T[4], v1, T[0] * v0));
    d1 = fmaf(T[9], v2, fmaf(T[5], v1, T[1] * v0));
    d2 = fmaf(T[10], v2, fmaf(T[6], v1, T[2] * v0));
}

// acc[3][4] += {v_i c_j, v_i}: the product of two fp32 numbers is exact in fp64 (48 bits of significand), so only the sums round
GS_HD void exposure_accumulate(double acc[12], float v0, float v1, float v2, float c0, float c1, float c2) {
    const double dv0 = (double)v0, dv1 = (double)v1, dv2 = (double)v2, dc0 = (double)c0, dc1 = (double)c1, dc2 = (double)c2;
    acc[0] += dv0 * dc0; acc[1] += dv0 * dc1; acc[2] += dv0 * dc2; acc[3] += dv0;
    acc[4] += dv1 * dc0; acc[5] += dv1 * dc1; acc[6] += dv1 * dc2; acc[7] += dv1;
    acc[8] += dv2 * dc0; acc[9] += dv2 * dc1; acc[10] += dv2 * dc2; acc[11] += dv2;
}

// One Adam update, adam1() of gs_common.h with its contractions written out (tests/adam_ref.py "The bounds"):
// isbc2 = 1 / sqrt(1 - beta2^t), ss = lr / (1 - beta1^t), both formed on the host from (double)beta.
GS_HD void exposure_adam1(float& p, float g, float& m, float& v, float b1, float b2, float eps, float isbc2, float ss) {
    m = fmaf(b1, m, (1.f - b1) * g);
    v = fmaf(b2, v, ((1.f - b2) * g) * g);
    const float denom = fmaf(sqrtf(v), isbc2, eps);
    p = fmaf(-ss, m / denom, p);
}

}  // namespace gs
