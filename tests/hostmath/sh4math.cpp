// Host (g++) build of the SH functions of easy_gaussian_splatting_amd/csrc/gs_math.h, sized for degree 4 (K up to 25).
// TEST-ONLY (tests/test_sh4_host.py): hostmath.cpp stages a Gaussian's SH gradient in a 48-float row, which cannot take
// K = 25.  Every entry point loops over n independent directions / Gaussians; it is never loaded by the product package.
#include "../../easy_gaussian_splatting_amd/csrc/gs_math.h"

extern "C" {

// Y[n][25]: the basis up to `degree` (entries above (degree+1)^2 are left as they were)
void sh4_basis(int degree, int n, const float* dirs, float* Y) {
    for (int i = 0; i < n; ++i) gs::sh_basis(degree, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], Y + 25 * i);
}

// g[n][3] = sum_k d[n][k] dY_k/du, u treated as three free variables
void sh4_dir_grad(int degree, int n, const float* d, const float* dirs, float* g) {
    for (int i = 0; i < n; ++i)
        gs::sh_dir_grad(degree, d + 25 * i, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], g[3 * i], g[3 * i + 1], g[3 * i + 2]);
}

// G[n][12] from sh[n][K][3]
void sh4_dir_jacobian(int degree, int K, int n, const float* sh, const float* dirs, float* G) {
    for (int i = 0; i < n; ++i)
        gs::sh_dir_jacobian(degree, sh + 3 * (long)K * i, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], G + 12 * i);
}

// rgb[n][3] from sh[n][K][3]
void sh4_to_rgb(int degree, int K, int n, const float* sh, const float* dirs, float* rgb) {
    for (int i = 0; i < n; ++i)
        gs::sh_to_rgb(degree, sh + 3 * (long)K * i, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], rgb + 3 * i);
}

// v_sh[n][K][3] (coefficients below (degree+1)^2; the rest zero) and v_mean[n][3] (direction term only) of sh_vjp
// (use_jac = 0, from the coefficients) or sh_vjp_jac (use_jac = 1, from G[n][12])
void sh4_vjp(int degree, int K, int n, const float* sh, const float* G, const float* rgb, const float* v_rgb,
             const float* dirs, const float* dnorm, float* v_sh, float* v_mean, int use_jac) {
    for (int i = 0; i < n; ++i) {
        float row[3 * 25] = {0.f};
        float vm[3] = {0.f, 0.f, 0.f};
        const float x = dirs[3 * i], y = dirs[3 * i + 1], z = dirs[3 * i + 2];
        if (use_jac) gs::sh_vjp_jac(degree, G + 12 * i, rgb + 3 * i, v_rgb + 3 * i, x, y, z, dnorm[i], row, vm);
        else gs::sh_vjp(degree, sh + 3 * (long)K * i, rgb + 3 * i, v_rgb + 3 * i, x, y, z, dnorm[i], row, vm, false);
        const int ka3 = 3 * (degree + 1) * (degree + 1);
        for (int o = 0; o < 3 * K; ++o) v_sh[3 * (long)K * i + o] = o < ka3 ? row[o] : 0.f;
        v_mean[3 * i] = vm[0]; v_mean[3 * i + 1] = vm[1]; v_mean[3 * i + 2] = vm[2];
    }
}

}  // extern "C"
