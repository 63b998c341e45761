// gs_tsdf.h -- THE definition of the TSDF integration and of the marching-tetrahedra extraction (gs_tsdf.hip, mesh.py).
// Plain C++ that compiles for the device and for the host alike: tests/hostmath/tsdf.cpp builds it with the host compiler,
// tests/test_tsdf_host.py holds it to a float64 restatement and tests/test_gpu_mesh.py holds the kernels to it bit for bit.  Every
// product that feeds a sum is an explicit fmaf, so the result is the same with and without -ffp-contract; every division is the
// correctly rounded one.
//
// Volume: samples at the grid corners p(ix, iy, iz) = fmaf(i, h, origin) per axis, linear index ix + nx (iy + ny iz).
//
// Integrating a pinhole view (viewmat [4][4] world -> camera, K [3][3] without skew), per voxel:
//   x = fmaf(R02, pz, fmaf(R01, py, fmaf(R00, px, t0)))   (y, z alike)         skip unless z > 0
//   u = fmaf(fx, x / z, cx), v = fmaf(fy, y / z, cy); pixel (floor u, floor v)  skip unless inside [0, W) x [0, H)
//   d = the pixel's depth                                                       skip unless 0 < d <= depth_max, d finite,
//                                                                               and (with an alpha image) alpha >= min_alpha
//   sdf = d - z                                                                 skip if sdf < -trunc
//   s = min(1, sdf / trunc); w' = w + 1; tsdf = fmaf(tsdf, w, s) / w'; colour alike per channel; weight = min(w', max_weight)
// A skipped voxel keeps all its bits.
//
// Marching tetrahedra over the Kuhn split of every cell: corners c = bx + 2 by + 4 bz; tetrahedron k = 0..5 has the corners
// {0, m1, m2, 7} of the axis orders xyz, xzy, yxz, yzx, zxy, zyx.  Every tetrahedron edge joins a corner to one whose mask contains
// its own, so an edge of the grid is (owner voxel = the lower end, kind = the mask difference in 1..7) and carries vertex number
// owner * 7 + kind - 1 in the order of the vertices.  The 16-case table below is written for a tetrahedron (v0, v1, v2, v3) of
// positive orientation, det[v1 - v0, v2 - v0, v3 - v0] > 0 -- the even axis orders k = 0, 3, 4; the odd ones swap the last two
// vertices of every triangle.  (v1 - v0) x (v2 - v0) of a triangle points from inside (tsdf < 0) towards outside.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_TS_HD __host__ __device__ __forceinline__
#else
#define GS_TS_HD static inline
#endif

namespace gs {

struct TsdfGrid {
    int32_t nx, ny, nz;
    float ox, oy, oz, h;
};

// 7 nx ny nz < 2^31 (an edge flag per (voxel, kind) is indexed in int32), every dimension >= 2, h > 0
GS_TS_HD bool tsdf_grid_ok(const TsdfGrid& g) {
    if (g.nx < 2 || g.ny < 2 || g.nz < 2 || !(g.h > 0.f)) return false;
    const int64_t lim = ((int64_t)1 << 31) - 1;   // 7 n <= 2^31 - 1
    if (g.nx > lim / 28 || g.ny > lim / 28 || g.nz > lim / 28) return false;   // (the other two are >= 2; the products below fit)
    int64_t n = (int64_t)g.nx * g.ny;
    if (7 * n > lim) return false;
    n *= g.nz;
    return 7 * n <= lim;
}
GS_TS_HD int64_t tsdf_index(const TsdfGrid& g, int ix, int iy, int iz) { return ix + (int64_t)g.nx * (iy + (int64_t)g.ny * iz); }
GS_TS_HD float tsdf_coord(int i, float h, float o) { return fmaf((float)i, h, o); }

struct TsdfView {
    float r[9], t[3], fx, fy, cx, cy;
    int W, H;
    const float* image;   // [H][W][stride]
    int stride, dch, cch;  // the depth channel; the first of three colour channels or -1
    const float* alphas;  // [H][W] or null
    float trunc, depth_max, min_alpha, max_weight;
};
GS_TS_HD void tsdf_view_camera(TsdfView& v, const float* viewmat, const float* K) {
    v.r[0] = viewmat[0]; v.r[1] = viewmat[1]; v.r[2] = viewmat[2]; v.t[0] = viewmat[3];
    v.r[3] = viewmat[4]; v.r[4] = viewmat[5]; v.r[5] = viewmat[6]; v.t[1] = viewmat[7];
    v.r[6] = viewmat[8]; v.r[7] = viewmat[9]; v.r[8] = viewmat[10]; v.t[2] = viewmat[11];
    v.fx = K[0]; v.cx = K[2]; v.fy = K[4]; v.cy = K[5];
}

// one voxel at p = (px, py, pz); tsdf / weight / color point at ITS entries (color: 3 floats or null)
GS_TS_HD void tsdf_integrate_voxel(const TsdfView& v, float px, float py, float pz, float* tsdf, float* weight, float* color) {
    const float x = fmaf(v.r[2], pz, fmaf(v.r[1], py, fmaf(v.r[0], px, v.t[0])));
    const float y = fmaf(v.r[5], pz, fmaf(v.r[4], py, fmaf(v.r[3], px, v.t[1])));
    const float z = fmaf(v.r[8], pz, fmaf(v.r[7], py, fmaf(v.r[6], px, v.t[2])));
    if (!(z > 0.f)) return;
    const float fu = floorf(fmaf(v.fx, x / z, v.cx)), fv = floorf(fmaf(v.fy, y / z, v.cy));
    if (!(fu >= 0.f && fu < (float)v.W && fv >= 0.f && fv < (float)v.H)) return;   // (false for a NaN)
    const int64_t pix = (int64_t)(int)fv * v.W + (int)fu;
    const float* texel = v.image + pix * v.stride;
    const float d = texel[v.dch];
    if (!(d > 0.f && d <= v.depth_max && d < INFINITY)) return;
    if (v.alphas != nullptr && !(v.alphas[pix] >= v.min_alpha)) return;
    const float sdf = d - z;
    if (sdf < -v.trunc) return;
    const float s = fminf(1.f, sdf / v.trunc);
    const float w = *weight, w1 = w + 1.f;
    *tsdf = fmaf(*tsdf, w, s) / w1;
    if (color != nullptr && v.cch >= 0) {
        color[0] = fmaf(color[0], w, texel[v.cch]) / w1;
        color[1] = fmaf(color[1], w, texel[v.cch + 1]) / w1;
        color[2] = fmaf(color[2], w, texel[v.cch + 2]) / w1;
    }
    *weight = fminf(w1, v.max_weight);
}

// ---- marching tetrahedra ----

GS_TS_HD bool mt_inside(float f) { return f < 0.f; }   // zero is outside
// the voxel of cube corner m (or the far end of an edge of kind m) of the cell / owner at linear index o
GS_TS_HD int64_t mt_corner(int nx, int ny, int64_t o, int m) {
    return o + (m & 1) + (int64_t)nx * (((m >> 1) & 1) + (int64_t)ny * ((m >> 2) & 1));
}
// corner j = 0..3 of tetrahedron k as a cube corner: 3 bits each of {0, m1, m2, 7}
constexpr uint32_t mt_tet12(int m1, int m2) { return (uint32_t)((m1 << 3) | (m2 << 6) | (7 << 9)); }
GS_TS_HD uint32_t mt_tet(int k) {
    switch (k) {
        case 0: return mt_tet12(1, 3);    // x y z
        case 1: return mt_tet12(1, 5);    // x z y
        case 2: return mt_tet12(2, 3);    // y x z
        case 3: return mt_tet12(2, 6);    // y z x
        case 4: return mt_tet12(4, 5);    // z x y
        default: return mt_tet12(4, 6);   // z y x
    }
}
GS_TS_HD int mt_tet_corner(uint32_t tet, int j) { return (int)((tet >> (3 * j)) & 7u); }
GS_TS_HD bool mt_tet_positive(int k) { return ((0x19 >> k) & 1) != 0; }   // the even axis orders: k = 0, 3, 4
// which of the tetrahedron's four corners are inside, from the cell's 8-bit corner mask
GS_TS_HD int mt_tet_case(uint32_t tet, int mask) {
    return ((mask >> mt_tet_corner(tet, 0)) & 1) | (((mask >> mt_tet_corner(tet, 1)) & 1) << 1) |
           (((mask >> mt_tet_corner(tet, 2)) & 1) << 2) | (((mask >> mt_tet_corner(tet, 3)) & 1) << 3);
}

// The 16 cases of a positively oriented tetrahedron.  An entry: bits 0-1 the number of triangles; vertex i of triangle t in the four
// bits at 4 + 12 t + 4 i, an edge pq (p < q, positions in the corner list) as p | q << 2.
//   one corner i inside: the triangle on its three edges, in the order that an even relabelling (i, ...) of the tetrahedron gives
//     -- (0,1,2,3), (1,0,3,2), (2,0,1,3), (3,0,2,1); three inside: the one outside corner's triangle reversed.
//   two inside {a, b}, outside {c, d}, each pair in list order: the quad ac, ad, bd, bc, cut along ac-bd into (ac, ad, bd) and
//     (ac, bd, bc) when (a, b, c, d) is an even permutation of (0, 1, 2, 3), into (ac, bd, ad) and (ac, bc, bd) when it is odd
//     ({0,2} and {1,3} inside).
constexpr uint32_t mt_e(int p, int q) { return (uint32_t)(p | (q << 2)); }
constexpr uint32_t mt_one(uint32_t a, uint32_t b, uint32_t c) { return 1u | (a << 4) | (b << 8) | (c << 12); }
constexpr uint32_t mt_two(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f) {
    return 2u | (a << 4) | (b << 8) | (c << 12) | (d << 16) | (e << 20) | (f << 24);
}
GS_TS_HD uint32_t mt_case(int c) {
    constexpr uint32_t e01 = mt_e(0, 1), e02 = mt_e(0, 2), e03 = mt_e(0, 3), e12 = mt_e(1, 2), e13 = mt_e(1, 3), e23 = mt_e(2, 3);
    switch (c) {
        case 1: return mt_one(e01, e02, e03);
        case 2: return mt_one(e01, e13, e12);
        case 4: return mt_one(e02, e12, e23);
        case 8: return mt_one(e03, e23, e13);
        case 14: return mt_one(e01, e03, e02);
        case 13: return mt_one(e01, e12, e13);
        case 11: return mt_one(e02, e23, e12);
        case 7: return mt_one(e03, e13, e23);
        case 3: return mt_two(e02, e03, e13, e02, e13, e12);    // {0,1} | {2,3}  even
        case 5: return mt_two(e01, e23, e03, e01, e12, e23);    // {0,2} | {1,3}  odd
        case 9: return mt_two(e01, e02, e23, e01, e23, e13);    // {0,3} | {1,2}  even
        case 6: return mt_two(e01, e13, e23, e01, e23, e02);    // {1,2} | {0,3}  even
        case 10: return mt_two(e01, e23, e12, e01, e03, e23);   // {1,3} | {0,2}  odd
        case 12: return mt_two(e02, e12, e13, e02, e13, e03);   // {2,3} | {0,1}  even
        default: return 0u;                                     // 0, 15: no surface
    }
}

// The corner mask of the cell whose lowest corner is voxel o (bit c: corner c inside), or -1 when the cell is not valid: a corner
// with weight < min_weight.  weight == null: the mask alone (the caller knows the cell to be valid).
GS_TS_HD int mt_cell_mask(int nx, int ny, int64_t o, const float* tsdf, const float* weight, float min_weight) {
    int mask = 0;
    bool valid = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t i = mt_corner(nx, ny, o, c);
        if (weight != nullptr) valid = valid && (weight[i] >= min_weight);
        mask |= (mt_inside(tsdf[i]) ? 1 : 0) << c;
    }
    return valid ? mask : -1;
}

// A valid cell marks the edges its surface crosses -- the 19 comparable corner pairs (a, a | m) whose ends differ -- with a plain
// store of 1 into edge_flags[owner * 7 + m - 1] and returns its number of triangles.
GS_TS_HD int mt_cell_flags(int nx, int ny, int64_t o, int mask, int32_t* edge_flags) {
    if (mask == 0 || mask == 255) return 0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int m = 1; m < 8; ++m)
            if ((a & m) == 0 && (((mask >> a) ^ (mask >> (a | m))) & 1)) edge_flags[mt_corner(nx, ny, o, a) * 7 + (m - 1)] = 1;
    int count = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) count += (int)(mt_case(mt_tet_case(mt_tet(k), mask)) & 3u);
    return count;
}

// The vertex on the edge (owner o at (ix, iy, iz), kind): t = f0 / (f0 - f1), position fmaf(t * step, h, p0) per axis, colour
// fmaf(t, c1 - c0, c0).  color / col may be null.
GS_TS_HD void mt_vertex(const TsdfGrid& g, const float* tsdf, const float* color, int64_t o, int ix, int iy, int iz, int kind, float* pos,
                        float* col) {
    const int64_t o1 = mt_corner(g.nx, g.ny, o, kind);
    const float f0 = tsdf[o], f1 = tsdf[o1];
    const float t = f0 / (f0 - f1);
    pos[0] = fmaf(t * (float)(kind & 1), g.h, tsdf_coord(ix, g.h, g.ox));
    pos[1] = fmaf(t * (float)((kind >> 1) & 1), g.h, tsdf_coord(iy, g.h, g.oy));
    pos[2] = fmaf(t * (float)((kind >> 2) & 1), g.h, tsdf_coord(iz, g.h, g.oz));
    if (color != nullptr && col != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float c0 = color[3 * o + c], c1 = color[3 * o1 + c];
            col[c] = fmaf(t, c1 - c0, c0);
        }
    }
}

// The triangles of a valid cell, tetrahedra 0..5 in order, into faces[3 * (first + i)] for i < its count; edge_incl is the inclusive
// scan of the edge flags, so edge e carries vertex edge_incl[e] - 1.  No store at or behind face n_faces; an index outside
// [0, n_vertices) is stored as -1.  Returns the number of triangles.
GS_TS_HD int mt_cell_faces(int nx, int ny, int64_t o, int mask, const int32_t* edge_incl, int64_t n_vertices, int64_t first, int64_t n_faces,
                           int32_t* faces) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t tet = mt_tet(k);
        const uint32_t entry = mt_case(mt_tet_case(tet, mask));
        const int cnt = (int)(entry & 3u);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (t >= cnt) continue;
            int32_t id0 = 0, id1 = 0, id2 = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t code = (entry >> (4 + 12 * t + 4 * i)) & 15u;
                const int a = mt_tet_corner(tet, (int)(code & 3u)), b = mt_tet_corner(tet, (int)(code >> 2));
                const int64_t e = mt_corner(nx, ny, o, a) * 7 + ((a ^ b) - 1);
                int32_t id = edge_incl[e] - 1;
                if (id < 0 || id >= n_vertices) id = -1;
                if (i == 0) id0 = id; else if (i == 1) id1 = id; else id2 = id;
            }
            const int64_t f = first + n;
            if (f >= 0 && f < n_faces) {
                faces[3 * f] = id0;
                faces[3 * f + 1] = mt_tet_positive(k) ? id1 : id2;
                faces[3 * f + 2] = mt_tet_positive(k) ? id2 : id1;
            }
            ++n;
        }
    }
    return n;
}

}  // namespace gs
