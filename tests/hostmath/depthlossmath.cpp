// Host build of csrc/gs_depth_loss.h for tests/test_depth_loss_host.py: the device's own text, driven over whole frames.
#include "../../easy_gaussian_splatting_amd/csrc/gs_depth_loss.h"

extern "C" {
// out[2] = {value, 1 / sum(w)}: the pixels' terms accumulated in fp64 in pixel order, finished as the one-block launch does; mask may be null
void dl_value(int mode, const float* d, const float* t, const float* m, int64_t n, float* out) {
    double acc[2] = {0.0, 0.0};
    for (int64_t p = 0; p < n; ++p) gs::depth_loss_accumulate(acc, mode, d[p], t[p], m ? m[p] : 0.f);
    gs::depth_loss_finish(acc[0], acc[1], out[0], out[1]);
}
// g[n] = scale * w sign(e) * {1; d > 0 ? -1 / d^2 : 0}
void dl_grad(int mode, const float* d, const float* t, const float* m, int64_t n, float scale, float* g) {
    for (int64_t p = 0; p < n; ++p) g[p] = gs::depth_loss_grad(mode, d[p], t[p], m ? m[p] : 0.f, scale);
}
// valid[n] = 1 where t is a measurement
void dl_valid(const float* t, int64_t n, int* valid) {
    for (int64_t p = 0; p < n; ++p) valid[p] = gs::depth_loss_valid(t[p]) ? 1 : 0;
}
}
