// gs_depth_loss.h -- the per-pixel math of the depth loss (gs_depth_loss.hip; include/gs_raster.h "Depth supervision"; DESIGN.md
// "Depth supervision in the captured step"): whether a target pixel is a measurement, its weight under the step's mask, the error in
// depth or in disparity, the pixel's terms of the two sums, the value from the sums, and the gradient with respect to the predicted
// depth.  Plain C++ that compiles for the device and for the host alike: tests/test_depth_loss_host.py builds it with the host
// compiler (tests/hostmath/depthlossmath.cpp) and holds it to fp64 numpy.  No multiply feeds an add in fp32 here, so there is
// nothing for a compiler to contract: the device and the host round alike.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD static inline
#endif

#define GS_DEPTH_LOSS_DEPTH 0       /* e = d - t            (include/gs_raster.h: GS_DEPTH_MODE_DEPTH) */
#define GS_DEPTH_LOSS_DISPARITY 1   /* e = disp(d) - 1 / t  (GS_DEPTH_MODE_DISPARITY) */

namespace gs {

// A measurement: t > 0 and finite.  A NaN fails the first comparison, +inf the second; zero and negatives mean "none".
GS_HD bool depth_loss_valid(float t) { return t > 0.f && t <= 3.402823466e+38f; }

// w = valid * (1 - m): the mask convention of LossComputer (m = 1 excludes the pixel); one rounding
GS_HD float depth_loss_weight(float t, float m) { return depth_loss_valid(t) ? 1.f - m : 0.f; }

GS_HD float depth_loss_disp(float d) { return d > 0.f ? 1.f / d : 0.f; }

// The error of a VALID pixel (the caller has asked depth_loss_valid: 1 / t is finite and positive): one or three roundings
GS_HD float depth_loss_error(int mode, float d, float t) {
    return mode == GS_DEPTH_LOSS_DISPARITY ? depth_loss_disp(d) - 1.f / t : d - t;
}

// acc += {w |e|, w}: the product of two fp32 numbers is exact in fp64, so only the sums round.  A pixel of weight 0 adds nothing,
// whatever its error holds (an invalid target never reaches the subtraction).
GS_HD void depth_loss_accumulate(double acc[2], int mode, float d, float t, float m) {
    const float w = depth_loss_weight(t, m);
    if (w == 0.f) return;
    acc[0] += (double)w * (double)fabsf(depth_loss_error(mode, d, t));
    acc[1] += (double)w;
}

// value = sum(w |e|) / sum(w) and 1 / sum(w), each formed in fp64 and rounded to fp32 once; exactly {0, 0} when nothing counts
GS_HD void depth_loss_finish(double sum_we, double sum_w, float& value, float& inv_w) {
    const bool any = sum_w > 0.0;
    value = any ? (float)(sum_we / sum_w) : 0.f;
    inv_w = any ? (float)(1.0 / sum_w) : 0.f;
}

// d value / d d times `scale` (the upstream gradient times 1 / sum(w)): scale * w * sign(e) * {depth: 1; disparity: d > 0 ? -1 / d^2 : 0},
// sign(0) = 0; left to right, every product rounded.  0 for a pixel that does not count -- never a NaN.
GS_HD float depth_loss_grad(int mode, float d, float t, float m, float scale) {
    const float w = depth_loss_weight(t, m);
    if (w == 0.f) return 0.f;
    const float e = depth_loss_error(mode, d, t);
    const float sgn = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
    if (sgn == 0.f) return 0.f;
    float g = (scale * w) * sgn;
    if (mode == GS_DEPTH_LOSS_DISPARITY) g = d > 0.f ? -((g / d) / d) : 0.f;
    return g;
}

}  // namespace gs
