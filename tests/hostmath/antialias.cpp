// Host (g++) build of the antialiased-mode instantiations of the projection chain and its VJP in
// easy_gaussian_splatting_amd/csrc/gs_math.h (project_gaussian_cm<kCamPinhole, AA>, project_chain<T, kCamPinhole, AA>,
// project_vjp_cam<T, kCamPinhole, AA>), composed as the kernel bodies compose them (gs_project_fwd_body.h, gs_project_bwd_body.h).
// TEST-ONLY (tests/test_antialias_host.py); it is never loaded by the product package.
// With -DAA_MAIN: a stand-alone program that runs both on a small scene with rank-deficient covariances and prints what it found
// (exit status 0: every output finite) -- the form a sanitizer build takes (g++ -fsanitize=address,undefined -DAA_MAIN).
#include "../../easy_gaussian_splatting_amd/csrc/gs_math.h"
#include <cstdio>
#include <cstring>

namespace {

template <bool AA>
void forward(int C, int N, const float* means, const float* quats, const float* scales, const float* opacities, const float* viewmats,
             const float* Ks, int W, int H, int tile, float eps2d, float near_p, float far_p, float radius_clip, int32_t* radii,
             float* means2d, float* depths, float* conics, float* rho, float* op_eff, float* extents) {
    const int tw = (W + tile - 1) / tile, th = (H + tile - 1) / tile;
    for (int c = 0; c < C; ++c) {
        gs::Camera cam;
        gs::make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, cam);
        for (int n = 0; n < N; ++n) {
            const long f = (long)c * N + n;
            gs::Splat2D s = gs::project_gaussian_cm<gs::kCamPinhole, AA>(means + 3 * n, quats + 4 * n, scales + 3 * n, cam, W, H, eps2d, near_p,
                                                                         far_p, radius_clip, tile, tw, th);
            radii[f] = s.radius; means2d[2 * f] = s.mx; means2d[2 * f + 1] = s.my; depths[f] = s.depth;
            conics[3 * f] = s.A; conics[3 * f + 1] = s.B; conics[3 * f + 2] = s.C;
            // the forward body's composition: the record's opacity and the extents taken from it
            float op = 0.f, ex = -1.f, ey = -1.f, comp = 0.f;
            if (s.radius > 0) {
                op = opacities[n];
                if (AA) { op *= s.rho; comp = s.rho; }
                gs::alpha_extent(op, s.cxx, s.cyy, ex, ey);
            }
            rho[f] = comp; op_eff[f] = op; extents[2 * f] = ex; extents[2 * f + 1] = ey;
        }
    }
}

// v_op_eff: the gradient of the record's opacity per (camera, Gaussian) -- what the blend leaves as s.v[7].
template <bool AA>
void backward(int C, int N, const float* means, const float* quats, const float* scales, const float* opacities, const float* viewmats,
              const float* Ks, int W, int H, float eps2d, float near_p, float far_p, const int32_t* radii, const float* v_means2d,
              const float* v_conics, const float* v_depths, const float* v_op_eff, float* v_means, float* v_quats, float* v_scales,
              float* v_opacities, double* cam_sums) {
    for (int c = 0; c < C; ++c) {
        gs::Camera cam;
        gs::make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, cam);
        for (int n = 0; n < N; ++n) {
            const long f = (long)c * N + n;
            if (radii[f] <= 0) continue;
            gs::ProjChain p;
            if (!gs::project_chain<gs::preal, gs::kCamPinhole, AA>(means + 3 * n, quats + 4 * n, scales + 3 * n, cam, eps2d, near_p, far_p, p)) continue;
            gs::preal vA[9], vt[3];
            gs::preal v_rho = 0;
            if (AA) v_rho = (gs::preal)v_op_eff[f] * (gs::preal)opacities[n];
            gs::project_vjp_cam<gs::preal, gs::kCamPinhole, AA>(means + 3 * n, scales + 3 * n, cam, p, v_means2d[2 * f], v_means2d[2 * f + 1],
                                                                v_conics[3 * f], v_conics[3 * f + 1], v_conics[3 * f + 2],
                                                                v_depths ? v_depths[f] : 0.f, v_means + 3 * n, v_quats + 4 * n, v_scales + 3 * n,
                                                                vA, vt, v_rho, (gs::preal)eps2d);
            v_opacities[n] += AA ? v_op_eff[f] * (float)p.rho : v_op_eff[f];
            for (int i = 0; i < 9; ++i) cam_sums[12 * c + i] += (double)vA[i];
            for (int i = 0; i < 3; ++i) cam_sums[12 * c + 9 + i] += (double)vt[i];
        }
    }
}

}  // namespace

extern "C" {

int aa_forward(int aa, int C, int N, const float* means, const float* quats, const float* scales, const float* opacities,
               const float* viewmats, const float* Ks, int W, int H, int tile, float eps2d, float near_p, float far_p, float radius_clip,
               int32_t* radii, float* means2d, float* depths, float* conics, float* rho, float* op_eff, float* extents) {
    if (aa) forward<true>(C, N, means, quats, scales, opacities, viewmats, Ks, W, H, tile, eps2d, near_p, far_p, radius_clip, radii, means2d,
                          depths, conics, rho, op_eff, extents);
    else forward<false>(C, N, means, quats, scales, opacities, viewmats, Ks, W, H, tile, eps2d, near_p, far_p, radius_clip, radii, means2d,
                        depths, conics, rho, op_eff, extents);
    return 0;
}

int aa_backward(int aa, int C, int N, const float* means, const float* quats, const float* scales, const float* opacities,
                const float* viewmats, const float* Ks, int W, int H, float eps2d, float near_p, float far_p, const int32_t* radii,
                const float* v_means2d, const float* v_conics, const float* v_depths, const float* v_op_eff, float* v_means, float* v_quats,
                float* v_scales, float* v_opacities, double* cam_sums) {
    if (N <= 0) return 0;
    std::memset(v_means, 0, sizeof(float) * 3 * N);
    std::memset(v_quats, 0, sizeof(float) * 4 * N);
    std::memset(v_scales, 0, sizeof(float) * 3 * N);
    std::memset(v_opacities, 0, sizeof(float) * N);
    std::memset(cam_sums, 0, sizeof(double) * 12 * C);
    if (aa) backward<true>(C, N, means, quats, scales, opacities, viewmats, Ks, W, H, eps2d, near_p, far_p, radii, v_means2d, v_conics, v_depths,
                           v_op_eff, v_means, v_quats, v_scales, v_opacities, cam_sums);
    else backward<false>(C, N, means, quats, scales, opacities, viewmats, Ks, W, H, eps2d, near_p, far_p, radii, v_means2d, v_conics, v_depths,
                         v_op_eff, v_means, v_quats, v_scales, v_opacities, cam_sums);
    return 0;
}

}  // extern "C"

#ifdef AA_MAIN
// Sixteen Gaussians in front of an axis-aligned camera, the first eight with scales (s, 0, 0) or (0, s, 0) -- rank-deficient covariances,
// det0 = 0 -- under the exact quaternions of the identity and the half turns; unit upstream gradients.
int main() {
    const int N = 16, W = 64, H = 48;
    float means[3 * N], quats[4 * N], scales[3 * N], opac[N];
    const float V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 3, 0, 0, 0, 1}, K[9] = {55.4f, 0, 32, 0, 55.4f, 24, 0, 0, 1};
    for (int n = 0; n < N; ++n) {
        means[3 * n] = -1.2f + 0.16f * n; means[3 * n + 1] = 0.7f - 0.09f * n; means[3 * n + 2] = 0.05f * (n % 5);
        for (int k = 0; k < 4; ++k) quats[4 * n + k] = n < 8 ? (k == n % 4 ? 1.f : 0.f) : 0.3f + 0.1f * ((n + k) % 7);
        scales[3 * n] = scales[3 * n + 1] = scales[3 * n + 2] = 0.02f + 0.03f * n;
        if (n < 8) { scales[3 * n + 1] = scales[3 * n + 2] = 0.f; if (n >= 4) { scales[3 * n + 1] = scales[3 * n]; scales[3 * n] = 0.f; } }
        opac[n] = 0.9f;
    }
    int32_t radii[N];
    float m2[2 * N], dep[N], con[3 * N], rho[N], ope[N], ext[2 * N], vm[2 * N], vc[3 * N], vo[N], g_m[3 * N], g_q[4 * N], g_s[3 * N], g_o[N];
    double sums[12];
    aa_forward(1, 1, N, means, quats, scales, opac, V, K, W, H, 16, 0.3f, 0.01f, 1e10f, 0.f, radii, m2, dep, con, rho, ope, ext);
    for (int i = 0; i < 2 * N; ++i) vm[i] = 1.f;
    for (int i = 0; i < 3 * N; ++i) vc[i] = 1.f;
    for (int i = 0; i < N; ++i) vo[i] = 1.f;
    aa_backward(1, 1, N, means, quats, scales, opac, V, K, W, H, 0.3f, 0.01f, 1e10f, radii, vm, vc, nullptr, vo, g_m, g_q, g_s, g_o, sums);
    int bad = 0, zero = 0, vis = 0;
    for (int n = 0; n < N; ++n) {
        vis += radii[n] > 0; zero += radii[n] > 0 && rho[n] == 0.f && ope[n] == 0.f && ext[2 * n] < 0.f;
        for (int k = 0; k < 3; ++k) bad += !std::isfinite(g_m[3 * n + k]) || !std::isfinite(g_s[3 * n + k]) || !std::isfinite(con[3 * n + k]);
        for (int k = 0; k < 4; ++k) bad += !std::isfinite(g_q[4 * n + k]);
        bad += !std::isfinite(g_o[n]) || !std::isfinite(rho[n]) || !std::isfinite(ext[2 * n]) || !std::isfinite(ext[2 * n + 1]);
    }
    for (int i = 0; i < 12; ++i) bad += !std::isfinite(sums[i]);
    std::printf("visible %d, rho == 0 and no extent: %d, non-finite outputs: %d\n", vis, zero, bad);
    return (bad == 0 && zero == 8 && vis == N) ? 0 : 1;
}
#endif
