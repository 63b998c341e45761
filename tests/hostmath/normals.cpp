// Host build of csrc/gs_normals.h for tests/test_normals_host.py and tests/test_gpu_normals.py: the device's own text, driven over
// whole arrays and frames -- what gs_gauss_normals_fwd / _bwd and gs_normal_loss_fwd / _bwd must return bit for bit (the loss value:
// the same terms, summed here in row-major order in fp64).
#include "../../easy_gaussian_splatting_amd/csrc/gs_normals.h"

#include <vector>

namespace {
float usable(int H, int W, const float* render4, const float* alphas, float min_alpha, int x, int y) {
    if (x < 0 || y < 0 || x >= W || y >= H) return 0.f;
    const int64_t p = (int64_t)y * W + x;
    return gs::normal_depth_ok(render4[4 * p + 3], alphas[p], min_alpha);
}
bool centre(int H, int W, const gs::NormalCam& cam, const float* render4, const float* alphas, float min_alpha, int x, int y,
            gs::NormalCentre& c) {
    if (x < 1 || y < 1 || x > W - 2 || y > H - 2) return false;
    return gs::normal_centre(cam, x, y, usable(H, W, render4, alphas, min_alpha, x, y), usable(H, W, render4, alphas, min_alpha, x - 1, y),
                             usable(H, W, render4, alphas, min_alpha, x + 1, y), usable(H, W, render4, alphas, min_alpha, x, y - 1),
                             usable(H, W, render4, alphas, min_alpha, x, y + 1), c);
}
}  // namespace

extern "C" {
int nm_axis(float s0, float s1, float s2) { return gs::normal_axis(s0, s1, s2); }

void nm_gauss_fwd(int64_t N, int C, const float* means, const float* quats, const float* scales, const float* viewmats, float* normals) {
    for (int64_t i = 0; i < N; ++i) gs::gauss_normals_fwd(N, C, i, means, quats, scales, viewmats, normals);
}

void nm_gauss_bwd(int64_t N, int C, const float* means, const float* quats, const float* scales, const float* viewmats,
                  const float* v_normals, float* v_quats) {
    for (int64_t i = 0; i < N; ++i) gs::gauss_normals_bwd(N, C, i, means, quats, scales, viewmats, v_normals, v_quats);
}

// rec[2] = {value, 1 / sum(w)}; sums[2] = {sum(w e), sum(w)} in fp64; depth_normals [H][W][3] or null
void nm_loss_fwd(int H, int W, const float* K, float min_alpha, const float* render4, const float* alphas, const float* mask, float* rec,
                 double* sums, float* depth_normals) {
    const gs::NormalCam cam = gs::normal_cam(K);
    double acc[2] = {0.0, 0.0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t p = (int64_t)y * W + x;
            gs::NormalCentre c;
            const bool valid = centre(H, W, cam, render4, alphas, min_alpha, x, y, c);
            if (valid) {
                const float w = gs::normal_loss_weight(mask ? mask[p] : 0.f);
                if (w != 0.f) gs::normal_loss_accumulate(acc, c, render4 + 4 * p, w);
            }
            if (depth_normals)
                for (int k = 0; k < 3; ++k) depth_normals[3 * p + k] = valid ? c.n[k] : 0.f;
        }
    gs::normal_loss_finish(acc[0], acc[1], rec[0], rec[1]);
    sums[0] = acc[0];
    sums[1] = acc[1];
}

void nm_loss_bwd(int H, int W, const float* K, float min_alpha, int detach_depth, const float* render4, const float* alphas,
                 const float* mask, float inv_w, float v_loss, float* v_render4) {
    const gs::NormalCam cam = gs::normal_cam(K);
    const float scale = v_loss * inv_w;
    const int64_t n = (int64_t)H * W;
    std::vector<float> sent((size_t)(4 * n), 0.f);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t p = (int64_t)y * W + x;
            float v_nb[3] = {0.f, 0.f, 0.f}, send[4] = {0.f, 0.f, 0.f, 0.f};
            gs::NormalCentre c;
            if (centre(H, W, cam, render4, alphas, min_alpha, x, y, c)) {
                const float w = gs::normal_loss_weight(mask ? mask[p] : 0.f);
                if (w != 0.f) gs::normal_centre_vjp(cam, x, y, c, render4 + 4 * p, -(scale * w), v_nb, send);
            }
            for (int k = 0; k < 3; ++k) v_render4[4 * p + k] = v_nb[k];
            if (!detach_depth)
                for (int k = 0; k < 4; ++k) sent[(size_t)(4 * p + k)] = send[k];
        }
    auto at = [&](int x, int y, int k) { return (x < 0 || y < 0 || x >= W || y >= H) ? 0.f : sent[(size_t)(4 * ((int64_t)y * W + x) + k)]; };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            v_render4[4 * ((int64_t)y * W + x) + 3] = gs::normal_depth_gather(at(x, y - 1, 1), at(x, y + 1, 0), at(x - 1, y, 3), at(x + 1, y, 2));
}
}
