// Host build of csrc/gs_tsdf.h for tests/test_tsdf_host.py and tests/test_gpu_mesh.py: the device's own text, driven over whole
// volumes -- what gs_tsdf_integrate, gs_mt_flags, gs_mt_vertices and gs_mt_faces must return bit for bit.
#include "../../easy_gaussian_splatting_amd/csrc/gs_tsdf.h"

#include <vector>

namespace {
gs::TsdfGrid grid_of(const int32_t* dims, const float* origin, float h) {
    gs::TsdfGrid g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2];
    g.h = h;
    return g;
}
}  // namespace

extern "C" {
int ts_grid_ok(const int32_t* dims, float h) {
    const float zero[3] = {0.f, 0.f, 0.f};
    return gs::tsdf_grid_ok(grid_of(dims, zero, h)) ? 1 : 0;
}

// one view into tsdf[n], weight[n], color[n][3] (or null), in place
void ts_integrate(const int32_t* dims, const float* origin, float h, float trunc, float depth_max, float min_alpha, float max_weight,
                  const float* viewmat, const float* K, int W, int H, const float* image, int stride, int dch, int cch,
                  const float* alphas, float* tsdf, float* weight, float* color) {
    const gs::TsdfGrid g = grid_of(dims, origin, h);
    gs::TsdfView v;
    gs::tsdf_view_camera(v, viewmat, K);
    v.W = W; v.H = H; v.image = image; v.stride = stride; v.dch = dch; v.cch = cch; v.alphas = alphas;
    v.trunc = trunc; v.depth_max = depth_max; v.min_alpha = min_alpha; v.max_weight = max_weight;
    for (int iz = 0; iz < g.nz; ++iz)
        for (int iy = 0; iy < g.ny; ++iy)
            for (int ix = 0; ix < g.nx; ++ix) {
                const int64_t o = gs::tsdf_index(g, ix, iy, iz);
                gs::tsdf_integrate_voxel(v, gs::tsdf_coord(ix, g.h, g.ox), gs::tsdf_coord(iy, g.h, g.oy), gs::tsdf_coord(iz, g.h, g.oz),
                                         tsdf + o, weight + o, color ? color + 3 * o : nullptr);
            }
}

// The extraction.  Called twice: with vertices == null it only counts (totals[0] vertices, totals[1] faces); then it fills
// vertices[nv][3], colors[nv][3] (with color), faces[nf][3], owner[nv] and kind[nv].
void ts_extract(const int32_t* dims, const float* origin, float h, float min_weight, const float* tsdf, const float* weight,
                const float* color, int64_t* totals, float* vertices, float* colors, int32_t* faces, int64_t* owner, int32_t* kind) {
    const gs::TsdfGrid g = grid_of(dims, origin, h);
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    std::vector<int32_t> edge((size_t)(7 * n), 0), tri((size_t)n, 0), cell_mask((size_t)n, -1);
    for (int iz = 0; iz + 1 < g.nz; ++iz)
        for (int iy = 0; iy + 1 < g.ny; ++iy)
            for (int ix = 0; ix + 1 < g.nx; ++ix) {
                const int64_t o = gs::tsdf_index(g, ix, iy, iz);
                const int mask = gs::mt_cell_mask(g.nx, g.ny, o, tsdf, weight, min_weight);
                cell_mask[(size_t)o] = mask;
                if (mask >= 0) tri[(size_t)o] = gs::mt_cell_flags(g.nx, g.ny, o, mask, edge.data());
            }
    std::vector<int32_t> edge_incl((size_t)(7 * n)), tri_incl((size_t)n);
    int64_t nv = 0, nf = 0;
    for (int64_t e = 0; e < 7 * n; ++e) { nv += edge[(size_t)e]; edge_incl[(size_t)e] = (int32_t)nv; }
    for (int64_t o = 0; o < n; ++o) { nf += tri[(size_t)o]; tri_incl[(size_t)o] = (int32_t)nf; }
    totals[0] = nv;
    totals[1] = nf;
    if (vertices == nullptr) return;
    for (int iz = 0; iz < g.nz; ++iz)
        for (int iy = 0; iy < g.ny; ++iy)
            for (int ix = 0; ix < g.nx; ++ix) {
                const int64_t o = gs::tsdf_index(g, ix, iy, iz);
                for (int k = 1; k < 8; ++k) {
                    const int64_t e = 7 * o + (k - 1);
                    if (!edge[(size_t)e]) continue;
                    const int64_t r = edge_incl[(size_t)e] - 1;
                    gs::mt_vertex(g, tsdf, color, o, ix, iy, iz, k, vertices + 3 * r, color ? colors + 3 * r : nullptr);
                    owner[r] = o;
                    kind[r] = k;
                }
                if (tri[(size_t)o] > 0)
                    gs::mt_cell_faces(g.nx, g.ny, o, cell_mask[(size_t)o], edge_incl.data(), nv, tri_incl[(size_t)o] - tri[(size_t)o], nf, faces);
            }
}
}
