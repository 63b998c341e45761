// gs_tsdf.hip -- a triangle mesh out of rendered depth, for gfx950: TSDF fusion and marching tetrahedra (mesh.py).
// Every value is the function gs_tsdf.h states, bit for bit.
//
//   tsdf_integrate_kernel : one thread per voxel, one launch per view.  The camera is read from device memory (uniform loads); the
//                           depth, the colour and the alpha of the voxel's pixel are read in place from the [H][W][stride] render.
//                           A voxel the view does not reach neither loads nor stores its entries.
//   mt_flags_kernel       : one thread per cell.  A valid cell stores 1 into the flag of every edge its surface crosses (several
//                           cells may store the same 1: identical plain stores) and its triangle count into tri_counts; every
//                           other voxel stores a count of 0.
//   (gs_scan_rows_i32 of gs_refine.hip: the inclusive scans of the 7 n edge flags and of the n triangle counts)
//   mt_totals_kernel      : {vertices, faces} into page-locked host memory: the extraction's one host read
//   mt_vertices_kernel    : one thread per owner voxel walks its 7 edge kinds; a flagged edge stores its vertex at scan - 1
//   mt_faces_kernel       : one thread per cell with triangles stores them at (scan - count) ..
//
// All kernels share one map of threads to voxels: a block of 256 is 64 voxels along x by 4 along y of one z layer, the blocks
// numbered x fastest, so a wave reads and writes one contiguous run of a row.  No atomics, no scratch, no LDS; every store of the
// emit kernels is checked against the totals the host read.
#include "gs_common.h"
#include "gs_tsdf.h"

namespace gs {

constexpr int kTsBx = 64, kTsBy = 4;

struct TsdfBlocks {
    int nbx, nby;
    unsigned total;
};
static TsdfBlocks tsdf_blocks(const TsdfGrid& g) {
    TsdfBlocks b;
    b.nbx = (g.nx + kTsBx - 1) / kTsBx;
    b.nby = (g.ny + kTsBy - 1) / kTsBy;
    b.total = (unsigned)((int64_t)b.nbx * b.nby * g.nz);   // <= nx ny nz < 2^31 / 7
    return b;
}
// the block's voxel of this thread; false outside the grid.  (two scalar divisions per block)
__device__ __forceinline__ bool tsdf_my_voxel(const TsdfGrid& g, int nbx, int nby, int& ix, int& iy, int& iz) {
    const int b = (int)blockIdx.x;
    const int bx = b % nbx, r = b / nbx;
    const int by = r % nby;
    iz = r / nby;
    ix = bx * kTsBx + (int)(threadIdx.x & (kTsBx - 1));
    iy = by * kTsBy + (int)(threadIdx.x >> 6);
    return ix < g.nx && iy < g.ny && iz < g.nz;
}

struct TsdfIntegrateArgs {
    TsdfGrid g;
    int nbx, nby;
    const float *viewmat, *K;
    TsdfView v;   // (the camera fields are filled by the kernel)
    float *tsdf, *weight, *color;
};

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const TsdfIntegrateArgs a) {
    int ix, iy, iz;
    if (!tsdf_my_voxel(a.g, a.nbx, a.nby, ix, iy, iz)) return;
    TsdfView v = a.v;
    tsdf_view_camera(v, a.viewmat, a.K);
    const int64_t o = tsdf_index(a.g, ix, iy, iz);
    tsdf_integrate_voxel(v, tsdf_coord(ix, a.g.h, a.g.ox), tsdf_coord(iy, a.g.h, a.g.oy), tsdf_coord(iz, a.g.h, a.g.oz), a.tsdf + o,
                         a.weight + o, a.color != nullptr ? a.color + 3 * o : nullptr);
}

__global__ __launch_bounds__(256) void mt_flags_kernel(const TsdfGrid g, int nbx, int nby, float min_weight, const float* __restrict__ tsdf,
                                                       const float* __restrict__ weight, int32_t* edge_flags,
                                                       int32_t* __restrict__ tri_counts) {
    int ix, iy, iz;
    if (!tsdf_my_voxel(g, nbx, nby, ix, iy, iz)) return;
    const int64_t o = tsdf_index(g, ix, iy, iz);
    int count = 0;
    if (ix < g.nx - 1 && iy < g.ny - 1 && iz < g.nz - 1) {
        const int mask = mt_cell_mask(g.nx, g.ny, o, tsdf, weight, min_weight);
        if (mask >= 0) count = mt_cell_flags(g.nx, g.ny, o, mask, edge_flags);
    }
    tri_counts[o] = count;
}

__global__ void mt_totals_kernel(int64_t n, const int32_t* __restrict__ edge_incl, const int32_t* __restrict__ tri_incl,
                                 int64_t* __restrict__ totals_host) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    totals_host[0] = edge_incl[7 * n - 1];
    totals_host[1] = tri_incl[n - 1];
    __threadfence_system();
}

__global__ __launch_bounds__(256) void mt_vertices_kernel(const TsdfGrid g, int nbx, int nby, const float* __restrict__ tsdf,
                                                          const float* __restrict__ color, const int32_t* __restrict__ edge_flags,
                                                          const int32_t* __restrict__ edge_incl, int64_t n_vertices,
                                                          float* __restrict__ vertices, float* __restrict__ colors) {
    int ix, iy, iz;
    if (!tsdf_my_voxel(g, nbx, nby, ix, iy, iz)) return;
    const int64_t o = tsdf_index(g, ix, iy, iz);
#pragma unroll
    for (int kind = 1; kind < 8; ++kind) {
        const int64_t e = 7 * o + (kind - 1);
        if (edge_flags[e] == 0) continue;
        // (a flagged edge belongs to a valid cell, so its far end is inside the grid; an address is still never taken on trust)
        if (ix + (kind & 1) >= g.nx || iy + ((kind >> 1) & 1) >= g.ny || iz + ((kind >> 2) & 1) >= g.nz) continue;
        const int64_t r = (int64_t)edge_incl[e] - 1;
        if (r < 0 || r >= n_vertices) continue;
        float pos[3], col[3] = {0.f, 0.f, 0.f};
        mt_vertex(g, tsdf, color, o, ix, iy, iz, kind, pos, col);
        vertices[3 * r] = pos[0]; vertices[3 * r + 1] = pos[1]; vertices[3 * r + 2] = pos[2];
        if (colors != nullptr) { colors[3 * r] = col[0]; colors[3 * r + 1] = col[1]; colors[3 * r + 2] = col[2]; }
    }
}

__global__ __launch_bounds__(256) void mt_faces_kernel(const TsdfGrid g, int nbx, int nby, const float* __restrict__ tsdf,
                                                       const int32_t* __restrict__ tri_counts, const int32_t* __restrict__ tri_incl,
                                                       const int32_t* __restrict__ edge_incl, int64_t n_vertices, int64_t n_faces,
                                                       int32_t* __restrict__ faces) {
    int ix, iy, iz;
    if (!tsdf_my_voxel(g, nbx, nby, ix, iy, iz)) return;
    if (ix >= g.nx - 1 || iy >= g.ny - 1 || iz >= g.nz - 1) return;
    const int64_t o = tsdf_index(g, ix, iy, iz);
    const int count = tri_counts[o];
    if (count <= 0) return;
    const int mask = mt_cell_mask(g.nx, g.ny, o, tsdf, nullptr, 0.f);
    mt_cell_faces(g.nx, g.ny, o, mask, edge_incl, n_vertices, (int64_t)tri_incl[o] - count, n_faces, faces);
}

static bool tsdf_grid_from(const int32_t* dims, const float* origin, float h, TsdfGrid* g) {
    if (dims == nullptr) return false;
    g->nx = dims[0]; g->ny = dims[1]; g->nz = dims[2];
    g->ox = origin ? origin[0] : 0.f; g->oy = origin ? origin[1] : 0.f; g->oz = origin ? origin[2] : 0.f;
    g->h = h;
    return tsdf_grid_ok(*g);
}

}  // namespace gs

using namespace gs;

#define GS_TSDF_DIMS_MSG "dims: every dimension >= 2 and 7 * nx * ny * nz < 2^31; voxel size > 0"

extern "C" int gs_tsdf_integrate(void* stream, const int32_t dims[3], const float origin[3], float h, float trunc, float depth_max,
                                 float min_alpha, float max_weight, const float* viewmat_dev, const float* K_dev, int W, int H,
                                 const float* image, int image_stride, int depth_channel, int color_channel, const float* alphas,
                                 float* tsdf, float* weight, float* color) {
    TsdfIntegrateArgs a;
    GS_REQUIRE(tsdf_grid_from(dims, origin, h, &a.g), GS_TSDF_DIMS_MSG);
    GS_REQUIRE(origin != nullptr, "null origin");
    GS_REQUIRE(trunc > 0.f && trunc < INFINITY, "trunc must be positive and finite");
    GS_REQUIRE(!(depth_max != depth_max) && !(min_alpha != min_alpha) && max_weight > 0.f, "depth_max, min_alpha not NaN; max_weight > 0");
    GS_REQUIRE(W >= 1 && H >= 1 && image_stride >= 1 && (int64_t)W * H * image_stride < (1ll << 31), "W, H, stride >= 1; H*W*stride < 2^31");
    GS_REQUIRE(W <= (1 << 24) && H <= (1 << 24), "W, H <= 2^24 (the pixel test compares in float32, where they must be exact)");
    GS_REQUIRE(depth_channel >= 0 && depth_channel < image_stride, "depth_channel outside the image's channels");
    GS_REQUIRE(color_channel == -1 || (color_channel >= 0 && color_channel + 3 <= image_stride), "color_channel: -1 or the first of three channels of the image");
    GS_REQUIRE((color_channel >= 0) == (color != nullptr), "a colour volume and colour channels come together");
    GS_REQUIRE(viewmat_dev && K_dev && image && tsdf && weight, "null pointer");
    const TsdfBlocks b = tsdf_blocks(a.g);
    a.nbx = b.nbx; a.nby = b.nby;
    a.viewmat = viewmat_dev; a.K = K_dev;
    memset(&a.v, 0, sizeof(a.v));
    a.v.W = W; a.v.H = H; a.v.image = image; a.v.stride = image_stride; a.v.dch = depth_channel; a.v.cch = color_channel;
    a.v.alphas = alphas; a.v.trunc = trunc; a.v.depth_max = depth_max; a.v.min_alpha = min_alpha; a.v.max_weight = max_weight;
    a.tsdf = tsdf; a.weight = weight; a.color = color;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(b.total), dim3(256), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("tsdf_integrate_kernel");
    return GS_OK;
}

extern "C" size_t gs_mt_scan_workspace_ints(const int32_t dims[3]) {
    TsdfGrid g;
    if (!tsdf_grid_from(dims, nullptr, 1.f, &g)) return 0;
    return gs_scan_rows_workspace_ints(1, 7 * (int64_t)g.nx * g.ny * g.nz);
}

extern "C" int gs_mt_flags(void* stream, const int32_t dims[3], float min_weight, const float* tsdf, const float* weight,
                           int32_t* edge_flags, int32_t* edge_incl, int32_t* tri_counts, int32_t* tri_incl, int32_t* scan_workspace,
                           int64_t* totals_host_mapped) {
    TsdfGrid g;
    GS_REQUIRE(tsdf_grid_from(dims, nullptr, 1.f, &g), GS_TSDF_DIMS_MSG);
    GS_REQUIRE(min_weight > 0.f, "min_weight must be positive (a voxel no view reached has weight 0)");
    GS_REQUIRE(tsdf && weight && edge_flags && edge_incl && tri_counts && tri_incl && scan_workspace && totals_host_mapped, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    const TsdfBlocks b = tsdf_blocks(g);
    GS_HIP_CHECK(hipMemsetAsync(edge_flags, 0, sizeof(int32_t) * 7 * (size_t)n, st));
    hipLaunchKernelGGL(mt_flags_kernel, dim3(b.total), dim3(256), 0, st, g, b.nbx, b.nby, min_weight, tsdf, weight, edge_flags, tri_counts);
    GS_LAUNCH_CHECK("mt_flags_kernel");
    int rc = gs_scan_rows_i32(stream, 1, 7 * n, edge_flags, edge_incl, scan_workspace);
    if (rc != GS_OK) return rc;
    rc = gs_scan_rows_i32(stream, 1, n, tri_counts, tri_incl, scan_workspace);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(mt_totals_kernel, dim3(1), dim3(64), 0, st, n, (const int32_t*)edge_incl, (const int32_t*)tri_incl, totals_host_mapped);
    GS_LAUNCH_CHECK("mt_totals_kernel");
    return GS_OK;
}

extern "C" int gs_mt_vertices(void* stream, const int32_t dims[3], const float origin[3], float h, const float* tsdf, const float* color,
                              const int32_t* edge_flags, const int32_t* edge_incl, int64_t n_vertices, float* vertices, float* colors) {
    TsdfGrid g;
    GS_REQUIRE(tsdf_grid_from(dims, origin, h, &g), GS_TSDF_DIMS_MSG);
    GS_REQUIRE(origin != nullptr, "null origin");
    GS_REQUIRE(n_vertices >= 0 && n_vertices <= 7 * (int64_t)g.nx * g.ny * g.nz, "0 <= n_vertices <= 7 * voxels");
    GS_REQUIRE((color != nullptr) == (colors != nullptr), "a colour volume and vertex colours come together");
    if (n_vertices == 0) return GS_OK;
    GS_REQUIRE(tsdf && edge_flags && edge_incl && vertices, "null pointer");
    const TsdfBlocks b = tsdf_blocks(g);
    hipLaunchKernelGGL(mt_vertices_kernel, dim3(b.total), dim3(256), 0, (hipStream_t)stream, g, b.nbx, b.nby, tsdf, color, edge_flags,
                       edge_incl, n_vertices, vertices, colors);
    GS_LAUNCH_CHECK("mt_vertices_kernel");
    return GS_OK;
}

extern "C" int gs_mt_faces(void* stream, const int32_t dims[3], const float* tsdf, const int32_t* tri_counts, const int32_t* tri_incl,
                           const int32_t* edge_incl, int64_t n_vertices, int64_t n_faces, int32_t* faces) {
    TsdfGrid g;
    GS_REQUIRE(tsdf_grid_from(dims, nullptr, 1.f, &g), GS_TSDF_DIMS_MSG);
    GS_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_faces <= 12 * (int64_t)g.nx * g.ny * g.nz, "0 <= n_vertices; 0 <= n_faces <= 12 * voxels");
    if (n_faces == 0) return GS_OK;
    GS_REQUIRE(tsdf && tri_counts && tri_incl && edge_incl && faces, "null pointer");
    const TsdfBlocks b = tsdf_blocks(g);
    hipLaunchKernelGGL(mt_faces_kernel, dim3(b.total), dim3(256), 0, (hipStream_t)stream, g, b.nbx, b.nby, tsdf, tri_counts, tri_incl, edge_incl,
                       n_vertices, n_faces, faces);
    GS_LAUNCH_CHECK("mt_faces_kernel");
    return GS_OK;
}
