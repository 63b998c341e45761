// Host build of csrc/gs_exposure.h for tests/test_exposure_host.py: the device's own text, driven over whole images.
#include "../../easy_gaussian_splatting_amd/csrc/gs_exposure.h"

extern "C" {
// out[n][3] = T applied to img[n][3]
void em_apply(const float* T, const float* img, int64_t n, float* out) {
    for (int64_t p = 0; p < n; ++p) gs::exposure_apply(T, img[3 * p], img[3 * p + 1], img[3 * p + 2], out[3 * p], out[3 * p + 1], out[3 * p + 2]);
}
// out[n][3] = A^T v[n][3]
void em_vjp(const float* T, const float* v, int64_t n, float* out) {
    for (int64_t p = 0; p < n; ++p) gs::exposure_vjp(T, v[3 * p], v[3 * p + 1], v[3 * p + 2], out[3 * p], out[3 * p + 1], out[3 * p + 2]);
}
// sums[3][4]: the pixels' terms accumulated in fp64 in pixel order, rounded to fp32 once
void em_sums(const float* v, const float* img, int64_t n, float* sums) {
    double acc[12] = {0};
    for (int64_t p = 0; p < n; ++p) gs::exposure_accumulate(acc, v[3 * p], v[3 * p + 1], v[3 * p + 2], img[3 * p], img[3 * p + 1], img[3 * p + 2]);
    for (int i = 0; i < 12; ++i) sums[i] = (float)acc[i];
}
void em_adam(float* p, const float* g, float* m, float* v, int64_t n, float b1, float b2, float eps, float isbc2, float ss) {
    for (int64_t i = 0; i < n; ++i) gs::exposure_adam1(p[i], g[i], m[i], v[i], b1, b2, eps, isbc2, ss);
}
}
