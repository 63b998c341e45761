// Host (g++) build of the depth render modes' arithmetic of easy_gaussian_splatting_amd/csrc/gs_math.h (depth_vjp_mean,
// depth_vjp_cam, expected_depth, expected_depth_vjp), driven as gs_depth.hip drives it.  TEST-ONLY (tests/test_depth_host.py); it is
// never loaded by the product package.
#include "../../easy_gaussian_splatting_amd/csrc/gs_math.h"
#include <cstring>

extern "C" {

// v_means[N,3] += sum_c v_z[c,n] viewmats[c][2][0:3] (camera order); cam_sums[C][4] = {sum_n v_z mean, sum_n v_z} in double.
int dm_depth_grads(int C, int N, const float* means, const float* viewmats, const float* v_z, float* v_means, double* cam_sums) {
    std::memset(cam_sums, 0, sizeof(double) * 4 * C);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c) {
            const float* V = viewmats + 16 * c;
            const float row2[3] = {V[8], V[9], V[10]};
            gs::depth_vjp_mean(v_z[(long)c * N + n], row2, v_means + 3 * n);
            gs::depth_vjp_cam(v_z[(long)c * N + n], means + 3 * n, cam_sums + 4 * c);
        }
    return 0;
}

int dm_expected_depth(int n, const float* acc, const float* alpha, const float* v_out, float* out, float* v_acc, float* v_alpha) {
    for (int i = 0; i < n; ++i) {
        out[i] = gs::expected_depth(acc[i], alpha[i]);
        gs::expected_depth_vjp(v_out[i], acc[i], alpha[i], v_acc[i], v_alpha[i]);
    }
    return 0;
}

}  // extern "C"
