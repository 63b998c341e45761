// gs_bilagrid.h -- the per-pixel math of bilagrid.BilateralGrids (gs_bilagrid.hip; DESIGN.md "Bilateral grids in the captured step"):
// a view's slab grids[12][L][Hg][Wg] of 3x4 colour affines (channel k = 4 i + j is entry (i, j) of [A | b]) sliced at a pixel's
// position and at the luminance of its own colour, the affine applied, the transpose applied to the pixel's gradient with the part
// that flows through the luminance, the weights of the slice's adjoint, the total-variation term of one node and the Adam update
// of one element.  Plain C++ that compiles for the device and for the host alike: tests/test_bilagrid_host.py builds it with the
// host compiler (tests/hostmath/bilagridmath.cpp) and holds it to torch's grid_sample in fp64.  Every multiply-add is spelled
// fmaf: the order below is the order on both sides, whatever the compiler would contract.
#pragma once
#include "gs_exposure.h"

namespace gs {

// Where a pixel falls in the slab: the cell's lowest node per axis and the fractions inside it.  zin: 0 < luma < 1, where the
// slice depends on the luminance (torch's border rule: no gradient through a clamped coordinate).
struct BilagridCell {
    int ix, iy, iz;
    float tx, ty, tz;
    bool zin;
};

// The cell of coordinate g on an axis of n >= 2 nodes: min(floor(g), n - 2), not below 0.  The comparisons are written so that a
// NaN takes the branch to 0 and no value outside [0, n - 2] is ever converted: the index is inside the slab whatever g is.
GS_HD int bilagrid_axis_cell(float g, int n) {
    const float f = floorf(g);
    int i = f >= 0.f ? (f <= (float)(n - 2) ? (int)f : n - 2) : 0;
    i = i > n - 2 ? n - 2 : i;
    return i < 0 ? 0 : i;
}

// (p + 0.5) / n_pix * (n_nodes - 1): the align_corners=True coordinate of pixel centre p.  Two roundings.
GS_HD float bilagrid_axis_coord(int p, int n_pix, int n_nodes) { return ((float)p + 0.5f) / (float)n_pix * (float)(n_nodes - 1); }

// The first pixel of cell c on an axis (the smallest p in [0, n_pix] whose cell is >= c; c = n_nodes - 1: n_pix).  The cell of a
// pixel is monotone in p, so cell c owns the pixels [first(c), first(c + 1)): the kernels' blocks partition the image by it, with
// the very expression the pixels themselves use.
GS_HD int bilagrid_axis_first(int c, int n_pix, int n_nodes) {
    if (c <= 0) return 0;
    if (c >= n_nodes - 1) return n_pix;
    int p = (int)ceilf((float)c * (float)n_pix / (float)(n_nodes - 1) - 0.5f);
    p = p < 0 ? 0 : (p > n_pix ? n_pix : p);
    while (p > 0 && bilagrid_axis_cell(bilagrid_axis_coord(p - 1, n_pix, n_nodes), n_nodes) >= c) --p;
    while (p < n_pix && bilagrid_axis_cell(bilagrid_axis_coord(p, n_pix, n_nodes), n_nodes) < c) ++p;
    return p;
}

// luma = fma(0.114, b, fma(0.587, g, 0.299 r)): three roundings
GS_HD float bilagrid_luma(float c0, float c1, float c2) { return fmaf(0.114f, c2, fmaf(0.587f, c1, 0.299f * c0)); }

// The luminance part of a pixel's cell (the cheap part: a block that owns one luminance node looks at it first) ...
GS_HD void bilagrid_cell_z(float luma, int L, BilagridCell& c) {
#ifdef __clang__
#pragma clang fp contract(off)   // gz is a rounded product of its own: its floor and its fraction belong to the same number
#endif
    const float lc = fminf(fmaxf(luma, 0.f), 1.f);   // (a NaN clamps to 0: fmaxf returns its other argument)
    const float gz = lc * (float)(L - 1);
    c.iz = bilagrid_axis_cell(gz, L);
    c.tz = gz - (float)c.iz;   // exact: g and its floor share g's grid of floats
    c.zin = luma > 0.f && luma < 1.f;
}
// ... and the spatial part
GS_HD void bilagrid_cell_xy(int x, int y, int W, int H, int Wg, int Hg, BilagridCell& c) {
    const float gx = bilagrid_axis_coord(x, W, Wg), gy = bilagrid_axis_coord(y, H, Hg);
    c.ix = bilagrid_axis_cell(gx, Wg); c.iy = bilagrid_axis_cell(gy, Hg);
    c.tx = gx - (float)c.ix; c.ty = gy - (float)c.iy;
}
GS_HD BilagridCell bilagrid_cell(int x, int y, int W, int H, int Wg, int Hg, int L, float luma) {
    BilagridCell c;
    bilagrid_cell_xy(x, y, W, H, Wg, Hg, c);
    bilagrid_cell_z(luma, L, c);
    return c;
}

// fmaf(t, b - a, a): two roundings, and b == a comes back as a for every t
GS_HD float bilagrid_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// One channel of the slice from the cell's 8 nodes n[z][y][x]: along x, then y, then z.  m0 / m1: the bilinear interpolants on the
// cell's two luminance planes (the backward needs their difference).
GS_HD float bilagrid_slice1(const float n[8], float tx, float ty, float tz, float& m0, float& m1) {
    m0 = bilagrid_lerp(bilagrid_lerp(n[0], n[1], tx), bilagrid_lerp(n[2], n[3], tx), ty);
    m1 = bilagrid_lerp(bilagrid_lerp(n[4], n[5], tx), bilagrid_lerp(n[6], n[7], tx), ty);
    return bilagrid_lerp(m0, m1, tz);
}

// out = M[:, :3] c + M[:, 3]: exposure's fixed chain.  At identity grids M is [I | 0] exactly and the input comes back bit for bit.
GS_HD void bilagrid_apply(const float M[12], float c0, float c1, float c2, float& o0, float& o1, float& o2) {
    exposure_apply(M, c0, c1, c2, o0, o1, o2);
}

// v_c = M[:, :3]^T v + w v_luma, v_luma = (L - 1) sum_i v_i ((M_z1 - M_z0)_i . [c; 1]) inside 0 < luma < 1 and 0 outside.
// D = M_z1 - M_z0 per channel (one rounding each).  At identity grids D is exactly 0, v_luma is exactly 0 (a sum of zeros times
// finite factors) and v_c = v: fma(0, v_2, fma(0, v_1, 1 * v_0)) and the like, then fma(w_j, 0, .).
GS_HD void bilagrid_vjp(const float M[12], const float D[12], bool zin, int L, float c0, float c1, float c2, float v0, float v1, float v2,
                        float& d0, float& d1, float& d2) {
    exposure_vjp(M, v0, v1, v2, d0, d1, d2);
    float e0, e1, e2;
    exposure_apply(D, c0, c1, c2, e0, e1, e2);
    const float s = fmaf(v2, e2, fmaf(v1, e1, v0 * e0));
    const float vl = zin ? (float)(L - 1) * s : 0.f;
    d0 = fmaf(0.299f, vl, d0); d1 = fmaf(0.587f, vl, d1); d2 = fmaf(0.114f, vl, d2);
}

// The adjoint of the slice: a pixel adds wz[.] wy[.] wx[.] a_k to its cell's 8 nodes, a_k = {v_i c_j, v_i} (exact in fp64 from
// fp32 factors, as exposure_accumulate forms them).  The weights of one axis in fp64 from the fp32 fraction: {1 - t, t}.
GS_HD void bilagrid_axis_weights(float t, double w[2]) { w[0] = 1.0 - (double)t; w[1] = (double)t; }
GS_HD void bilagrid_products(float v0, float v1, float v2, float c0, float c1, float c2, double a[12]) {
    const double dv[3] = {(double)v0, (double)v1, (double)v2}, dc[4] = {(double)c0, (double)c1, (double)c2, 1.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) a[4 * i + j] = dv[i] * dc[j];
}
// acc[4 spatial corners (y, x)][12] += (wz wy[.] wx[.]) a: a block's accumulation for ONE luminance node, whose weight is wz
GS_HD void bilagrid_accumulate(double acc[48], double wz, const double wy[2], const double wx[2], const double a[12]) {
    for (int sc = 0; sc < 4; ++sc) {
        const double w = wz * (wy[sc >> 1] * wx[sc & 1]);
        for (int k = 0; k < 12; ++k) acc[12 * sc + k] += w * a[k];
    }
}

// Total variation.  One node's terms of the value -- the squares of its FORWARD differences, each over its axis' count -- and its
// derivative: sum over the axes of (2 / count_a) ((g - g_minus) - (g_plus - g)), a missing neighbour contributing nothing.  All in
// fp64 from the fp32 nodes; inv_cnt[a] = 1 / (n_views count_a), the axes in the order {L, Hg, Wg}.  has_m / has_p: the neighbour
// below / above along the axis exists.
GS_HD void bilagrid_tv_node(float g, const float gm[3], const float gp[3], const bool has_m[3], const bool has_p[3], const double inv_cnt[3],
                            double& value, double& grad) {
    value = 0.0;
    grad = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double fwd = has_p[a] ? (double)gp[a] - (double)g : 0.0, bwd = has_m[a] ? (double)g - (double)gm[a] : 0.0;
        value += fwd * fwd * inv_cnt[a];
        grad += 2.0 * inv_cnt[a] * (bwd - fwd);
    }
}

// One Adam update: the exposure table's element (gs_adam_step's arithmetic, tests/adam_ref.py "The bounds")
GS_HD void bilagrid_adam1(float& p, float g, float& m, float& v, float b1, float b2, float eps, float isbc2, float ss) {
    exposure_adam1(p, g, m, v, b1, b2, eps, isbc2, ss);
}

}  // namespace gs
