// Host build of csrc/gs_pose.h for tests/test_pose_host.py: the device's own text, driven over chosen arguments.
#include "../../easy_gaussian_splatting_amd/csrc/gs_pose.h"

extern "C" {
void pm_compose(const float* delta, const float* w2c, float* viewmat) { gs::pose_compose(delta, w2c, viewmat); }
// (fp64 in, fp64 out: the view matrix is not rounded here, so the test's autograd sees the same function)
void pm_vjp(const double* delta, const double* w2c, const double* v_A, const double* v_t, const double* v_campos, double* v_delta) {
    gs::pose_vjp(delta, w2c, v_A, v_t, v_campos, v_delta);
}
void pm_coeffs(double theta2, double* abc) { gs::pose_coeffs(theta2, abc[0], abc[1], abc[2]); }
}
