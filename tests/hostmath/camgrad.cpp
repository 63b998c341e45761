// Host (g++) build of the camera-gradient functions of easy_gaussian_splatting_amd/csrc/gs_math.h (project_vjp_cam, sh_dir_term,
// sh_dir_term_jac), summed per camera in double as the gfx950 reduction does.  TEST-ONLY (tests/test_camgrad_host.py); it is
// never loaded by the product package.
#include "../../easy_gaussian_splatting_amd/csrc/gs_math.h"
#include <cstring>
#include <initializer_list>

extern "C" {

// cam_sums[C][16] = {v_A[9] (row-major), v_t[3], v_campos[3], 0} over the Gaussians with radii > 0 of each camera.
// v_*_cam: the geometry gradients project_vjp_cam leaves, v_*_ref: those of project_vjp (both accumulated over the cameras from
// zero, so that the caller can compare them bit for bit).  counts[0] += Gaussians whose Jacobian took the FOV clamp;
// counts[1] += Gaussians whose direction term differs in any bit from what sh_vjp / sh_vjp_jac add to a zero v_mean.
int cg_camera_grads(int C, int N, int K, int degree, const float* means, const float* quats, const float* scales,
                    const float* shs, const float* viewmats, const float* Ks, int W, int H, float eps2d, float near_p,
                    float far_p, const int32_t* radii, const float* colors, const float* v_means2d, const float* v_conics,
                    const float* v_colors, int use_jac, double* cam_sums, float* v_means_cam, float* v_quats_cam,
                    float* v_scales_cam, float* v_means_ref, float* v_quats_ref, float* v_scales_ref, int64_t* counts) {
    if (N <= 0) return 0;
    std::memset(cam_sums, 0, sizeof(double) * 16 * C);
    for (float* b : {v_means_cam, v_scales_cam, v_means_ref, v_scales_ref}) std::memset(b, 0, sizeof(float) * 3 * N);
    for (float* b : {v_quats_cam, v_quats_ref}) std::memset(b, 0, sizeof(float) * 4 * N);
    for (int c = 0; c < C; ++c) {
        gs::Camera cam;
        gs::make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, cam);
        double* out = cam_sums + 16 * c;
        for (int n = 0; n < N; ++n) {
            const long f = (long)c * N + n;
            if (radii[f] <= 0) continue;
            gs::ProjChain p;
            if (!gs::project_chain<gs::preal>(means + 3 * n, quats + 4 * n, scales + 3 * n, cam, eps2d, near_p, far_p, p)) continue;
            if (p.clampx != 0 || p.clampy != 0) counts[0] += 1;
            if (degree >= 0) {
                float ux, uy, uz, term[3], G[12], row[3 * gs::kMaxShCoeffs], vm[3] = {0.f, 0.f, 0.f};
                const float dn = gs::view_dir(means + 3 * n, cam, ux, uy, uz);
                const float* sh = shs + (long)n * K * 3;
                if (use_jac) {
                    if (degree >= 1) gs::sh_dir_jacobian(degree, sh, ux, uy, uz, G);
                    gs::sh_dir_term_jac(degree, G, colors + 3 * f, v_colors + 3 * f, ux, uy, uz, dn, term);
                    gs::sh_vjp_jac(degree, G, colors + 3 * f, v_colors + 3 * f, ux, uy, uz, dn, row, vm);
                } else {
                    gs::sh_dir_term(degree, sh + 3, colors + 3 * f, v_colors + 3 * f, ux, uy, uz, dn, term);
                    gs::sh_vjp(degree, sh, colors + 3 * f, v_colors + 3 * f, ux, uy, uz, dn, row, vm, false);
                }
                if (!(term[0] == vm[0] && term[1] == vm[1] && term[2] == vm[2])) counts[1] += 1;   // (0 + -0 = +0: compared as values)
                for (int i = 0; i < 3; ++i) out[12 + i] -= (double)term[i];
            }
            gs::preal vA[9], vt[3];
            gs::project_vjp_cam<gs::preal>(means + 3 * n, scales + 3 * n, cam, p, v_means2d[2 * f], v_means2d[2 * f + 1], v_conics[3 * f],
                                           v_conics[3 * f + 1], v_conics[3 * f + 2], 0.f, v_means_cam + 3 * n, v_quats_cam + 4 * n,
                                           v_scales_cam + 3 * n, vA, vt);
            gs::project_vjp<gs::preal>(scales + 3 * n, cam, p, v_means2d[2 * f], v_means2d[2 * f + 1], v_conics[3 * f],
                                       v_conics[3 * f + 1], v_conics[3 * f + 2], 0.f, v_means_ref + 3 * n, v_quats_ref + 4 * n,
                                       v_scales_ref + 3 * n);
            for (int i = 0; i < 9; ++i) out[i] += (double)vA[i];
            for (int i = 0; i < 3; ++i) out[9 + i] += (double)vt[i];
        }
    }
    return 0;
}

}  // extern "C"
