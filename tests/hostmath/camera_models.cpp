// Host (g++) build of the camera-model instantiations of the projection chain and its VJP in
// easy_gaussian_splatting_amd/csrc/gs_math.h (project_gaussian_cm, project_chain<T, CAM>, project_vjp_cam<T, CAM>).
// TEST-ONLY (tests/test_camera_model_host.py); it is never loaded by the product package.
#include "../../easy_gaussian_splatting_amd/csrc/gs_math.h"
#include <cstring>

namespace {

template <int CAM>
void forward(int C, int N, int K, int degree, const float* means, const float* quats, const float* scales, const float* shs,
             const float* viewmats, const float* Ks, int W, int H, int tile, float eps2d, float near_p, float far_p,
             float radius_clip, int32_t* radii, float* means2d, float* depths, float* conics, float* colors,
             int32_t* tiles_per_gauss) {
    const int tw = (W + tile - 1) / tile, th = (H + tile - 1) / tile;
    for (int c = 0; c < C; ++c) {
        gs::Camera cam;
        gs::make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, cam);
        for (int n = 0; n < N; ++n) {
            const long f = (long)c * N + n;
            gs::Splat2D s = gs::project_gaussian_cm<CAM>(means + 3 * n, quats + 4 * n, scales + 3 * n, cam, W, H, eps2d, near_p,
                                                         far_p, radius_clip, tile, tw, th);
            radii[f] = s.radius; means2d[2 * f] = s.mx; means2d[2 * f + 1] = s.my; depths[f] = s.depth;
            conics[3 * f] = s.A; conics[3 * f + 1] = s.B; conics[3 * f + 2] = s.C;
            float rgb[3] = {0.5f, 0.5f, 0.5f};
            int cnt = 0;
            if (s.radius > 0) {
                float ux, uy, uz;
                gs::view_dir(means + 3 * n, cam, ux, uy, uz);
                gs::sh_to_rgb(degree, shs + (long)n * K * 3, ux, uy, uz, rgb);
                cnt = (s.x1 - s.x0) * (s.y1 - s.y0);
            }
            colors[3 * f] = rgb[0]; colors[3 * f + 1] = rgb[1]; colors[3 * f + 2] = rgb[2];
            tiles_per_gauss[f] = cnt;
        }
    }
}

// The geometry gradients (accumulated over the cameras from zero) and, per camera, cam_sums[c][12] = {v_A[9] row-major, v_t[3]}
// in double: the projection's share of the view matrix's gradient (the SH direction's share is model-independent).
template <int CAM>
void backward(int C, int N, const float* means, const float* quats, const float* scales, const float* viewmats, const float* Ks,
              int W, int H, float eps2d, float near_p, float far_p, const int32_t* radii, const float* v_means2d,
              const float* v_conics, const float* v_depths, float* v_means, float* v_quats, float* v_scales, double* cam_sums) {
    for (int c = 0; c < C; ++c) {
        gs::Camera cam;
        gs::make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, cam);
        for (int n = 0; n < N; ++n) {
            const long f = (long)c * N + n;
            if (radii[f] <= 0) continue;
            gs::ProjChain p;
            if (!gs::project_chain<gs::preal, CAM>(means + 3 * n, quats + 4 * n, scales + 3 * n, cam, eps2d, near_p, far_p, p)) continue;
            gs::preal vA[9], vt[3];
            gs::project_vjp_cam<gs::preal, CAM>(means + 3 * n, scales + 3 * n, cam, p, v_means2d[2 * f], v_means2d[2 * f + 1],
                                                v_conics[3 * f], v_conics[3 * f + 1], v_conics[3 * f + 2], v_depths ? v_depths[f] : 0.f,
                                                v_means + 3 * n, v_quats + 4 * n, v_scales + 3 * n, vA, vt);
            for (int i = 0; i < 9; ++i) cam_sums[12 * c + i] += (double)vA[i];
            for (int i = 0; i < 3; ++i) cam_sums[12 * c + 9 + i] += (double)vt[i];
        }
    }
}

}  // namespace

extern "C" {

// model: 0 pinhole, 1 ortho, 2 fisheye (include/gs_raster.h: GS_CAMERA_*); -1: unknown model
int cm_forward(int model, int C, int N, int K, int degree, const float* means, const float* quats, const float* scales,
               const float* shs, const float* viewmats, const float* Ks, int W, int H, int tile, float eps2d, float near_p,
               float far_p, float radius_clip, int32_t* radii, float* means2d, float* depths, float* conics, float* colors,
               int32_t* tiles_per_gauss) {
#define CM_FWD(M) forward<M>(C, N, K, degree, means, quats, scales, shs, viewmats, Ks, W, H, tile, eps2d, near_p, far_p, radius_clip, \
                             radii, means2d, depths, conics, colors, tiles_per_gauss)
    if (model == 0) CM_FWD(gs::kCamPinhole); else if (model == 1) CM_FWD(gs::kCamOrtho); else if (model == 2) CM_FWD(gs::kCamFisheye);
    else return -1;
#undef CM_FWD
    return 0;
}

int cm_backward(int model, int C, int N, const float* means, const float* quats, const float* scales, const float* viewmats,
                const float* Ks, int W, int H, float eps2d, float near_p, float far_p, const int32_t* radii, const float* v_means2d,
                const float* v_conics, const float* v_depths, float* v_means, float* v_quats, float* v_scales, double* cam_sums) {
    if (N <= 0) return 0;
    std::memset(v_means, 0, sizeof(float) * 3 * N);
    std::memset(v_quats, 0, sizeof(float) * 4 * N);
    std::memset(v_scales, 0, sizeof(float) * 3 * N);
    std::memset(cam_sums, 0, sizeof(double) * 12 * C);
#define CM_BWD(M) backward<M>(C, N, means, quats, scales, viewmats, Ks, W, H, eps2d, near_p, far_p, radii, v_means2d, v_conics, v_depths, \
                              v_means, v_quats, v_scales, cam_sums)
    if (model == 0) CM_BWD(gs::kCamPinhole); else if (model == 1) CM_BWD(gs::kCamOrtho); else if (model == 2) CM_BWD(gs::kCamFisheye);
    else return -1;
#undef CM_BWD
    return 0;
}

// The fisheye's radial terms on their own: {k, e, g, h} of n camera-space points, in double (series below the threshold, closed form above).
int cm_fisheye_terms(int n, const double* xyz, double* out) {
    for (int i = 0; i < n; ++i)
        gs::fisheye_terms<double>(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
    return 0;
}

}  // extern "C"
