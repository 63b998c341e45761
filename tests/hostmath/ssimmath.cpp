// Host (g++) build of the evaluation metrics' per-pixel arithmetic of easy_gaussian_splatting_amd/csrc/gs_math.h
// (ssim_from_moments), driven as gs_metrics.hip drives it.  TEST-ONLY (tests/test_eval_host.py); it is never loaded by the
// product package.
#include "../../easy_gaussian_splatting_amd/csrc/gs_math.h"

extern "C" {

// out[i] = SSIM of window i from its four moments {mu_x, mu_y, E[xx] + E[yy], E[xy]}
int sm_ssim_from_moments(int n, const float* mu_x, const float* mu_y, const float* ess, const float* exy, float* out) {
    for (int i = 0; i < n; ++i) out[i] = gs::ssim_from_moments(mu_x[i], mu_y[i], ess[i], exy[i]);
    return 0;
}

}  // extern "C"
