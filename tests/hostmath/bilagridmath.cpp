// Host build of csrc/gs_bilagrid.h for tests/test_bilagrid_host.py: the device's own text, driven over whole images.
#include <vector>

#include "../../easy_gaussian_splatting_amd/csrc/gs_bilagrid.h"

namespace {
struct Shape { int H, W, Wg, Hg, L; };

inline float node(const float* slab, const Shape& s, int k, int z, int y, int x) {
    return slab[(((int64_t)k * s.L + z) * s.Hg + y) * s.Wg + x];
}
// M and D = M_z1 - M_z0 of a pixel, the kernels' bilagrid_slice over the slab itself
inline void slice(const float* slab, const Shape& s, const gs::BilagridCell& c, float M[12], float D[12]) {
    for (int k = 0; k < 12; ++k) {
        float n[8], m0, m1;
        for (int i = 0; i < 8; ++i) n[i] = node(slab, s, k, c.iz + (i >> 2), c.iy + ((i >> 1) & 1), c.ix + (i & 1));
        M[k] = gs::bilagrid_slice1(n, c.tx, c.ty, c.tz, m0, m1);
        D[k] = m1 - m0;
    }
}
}  // namespace

extern "C" {
// cells[n][3] = (ix, iy, iz) of every pixel
void bm_cells(const float* img, int H, int W, int Wg, int Hg, int L, int* cells) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t p = (int64_t)y * W + x;
            const gs::BilagridCell c = gs::bilagrid_cell(x, y, W, H, Wg, Hg, L, gs::bilagrid_luma(img[3 * p], img[3 * p + 1], img[3 * p + 2]));
            cells[3 * p] = c.ix; cells[3 * p + 1] = c.iy; cells[3 * p + 2] = c.iz;
        }
}
// first[c] for c = 0 .. n_nodes - 1: the pixel ranges of an axis' cells
void bm_axis_first(int n_pix, int n_nodes, int* first) {
    for (int c = 0; c < n_nodes; ++c) first[c] = gs::bilagrid_axis_first(c, n_pix, n_nodes);
}
// out[H][W][3] = the slice of slab applied to img
void bm_apply(const float* slab, const float* img, int H, int W, int Wg, int Hg, int L, float* out) {
    const Shape s = {H, W, Wg, Hg, L};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t p = 3 * ((int64_t)y * W + x);
            const gs::BilagridCell c = gs::bilagrid_cell(x, y, W, H, Wg, Hg, L, gs::bilagrid_luma(img[p], img[p + 1], img[p + 2]));
            float M[12], D[12];
            slice(slab, s, c, M, D);
            gs::bilagrid_apply(M, img[p], img[p + 1], img[p + 2], out[p], out[p + 1], out[p + 2]);
        }
}
// dv[H][W][3] = dL/d img from v = dL/d out, the part through the guide included
void bm_vjp(const float* slab, const float* img, const float* v, int H, int W, int Wg, int Hg, int L, float* dv) {
    const Shape s = {H, W, Wg, Hg, L};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t p = 3 * ((int64_t)y * W + x);
            const gs::BilagridCell c = gs::bilagrid_cell(x, y, W, H, Wg, Hg, L, gs::bilagrid_luma(img[p], img[p + 1], img[p + 2]));
            float M[12], D[12];
            slice(slab, s, c, M, D);
            gs::bilagrid_vjp(M, D, c.zin, L, img[p], img[p + 1], img[p + 2], v[p], v[p + 1], v[p + 2], dv[p], dv[p + 1], dv[p + 2]);
        }
}
// v_slab[12][L][Hg][Wg]: per luminance node and spatial cell the header's accumulation in pixel order (fp64), the cells that touch
// a node added in the kernels' order, rounded to fp32 once
void bm_adjoint(const float* img, const float* v, int H, int W, int Wg, int Hg, int L, float* v_slab) {
    const int cells = (Wg - 1) * (Hg - 1);
    std::vector<double> acc((size_t)cells * L * 48, 0.0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t p = 3 * ((int64_t)y * W + x);
            const gs::BilagridCell c = gs::bilagrid_cell(x, y, W, H, Wg, Hg, L, gs::bilagrid_luma(img[p], img[p + 1], img[p + 2]));
            double wx[2], wy[2], wz[2], a[12];
            gs::bilagrid_axis_weights(c.tx, wx); gs::bilagrid_axis_weights(c.ty, wy); gs::bilagrid_axis_weights(c.tz, wz);
            gs::bilagrid_products(v[p], v[p + 1], v[p + 2], img[p], img[p + 1], img[p + 2], a);
            const int cell = c.iy * (Wg - 1) + c.ix;
            for (int dz = 0; dz < 2; ++dz) gs::bilagrid_accumulate(&acc[((size_t)cell * L + c.iz + dz) * 48], wz[dz], wy, wx, a);
        }
    for (int k = 0; k < 12; ++k)
        for (int z = 0; z < L; ++z)
            for (int y = 0; y < Hg; ++y)
                for (int x = 0; x < Wg; ++x) {
                    double t = 0.0;
                    for (int cy = y - 1; cy <= y; ++cy)
                        for (int cx = x - 1; cx <= x; ++cx) {
                            if (cy < 0 || cy > Hg - 2 || cx < 0 || cx > Wg - 2) continue;
                            t += acc[((size_t)(cy * (Wg - 1) + cx) * L + z) * 48 + 12 * (2 * (y - cy) + (x - cx)) + k];
                        }
                    v_slab[(((int64_t)k * L + z) * Hg + y) * Wg + x] = (float)t;
                }
}
// tv[0] = the value (fp64 in node order, rounded once); v_grids = fl32(tv_weight * d tv / d grids)
void bm_tv(const float* grids, int n_views, int Wg, int Hg, int L, float tv_weight, float* tv, float* v_grids) {
    const int64_t plane = (int64_t)Hg * Wg, slab = 12 * (int64_t)L * plane, strides[3] = {plane, Wg, 1};
    const int extent[3] = {L, Hg, Wg};
    double inv_cnt[3], sum = 0.0;
    for (int a = 0; a < 3; ++a) inv_cnt[a] = 1.0 / ((double)n_views * (double)(slab / extent[a] * (extent[a] - 1)));
    for (int64_t e = 0; e < slab * n_views; ++e) {
        const int64_t in_slab = e % slab;
        const int at[3] = {(int)((in_slab / plane) % L), (int)((in_slab / Wg) % Hg), (int)(in_slab % Wg)};
        float gm[3], gp[3];
        bool has_m[3], has_p[3];
        for (int a = 0; a < 3; ++a) {
            has_m[a] = at[a] > 0; has_p[a] = at[a] < extent[a] - 1;
            gm[a] = has_m[a] ? grids[e - strides[a]] : 0.f;
            gp[a] = has_p[a] ? grids[e + strides[a]] : 0.f;
        }
        double value, grad;
        gs::bilagrid_tv_node(grids[e], gm, gp, has_m, has_p, inv_cnt, value, grad);
        sum += value;
        v_grids[e] = (float)((double)tv_weight * grad);
    }
    tv[0] = (float)sum;
}
void bm_adam(float* p, const float* g, float* m, float* v, int64_t n, float b1, float b2, float eps, float isbc2, float ss) {
    for (int64_t i = 0; i < n; ++i) gs::bilagrid_adam1(p[i], g[i], m[i], v[i], b1, b2, eps, isbc2, ss);
}
}
