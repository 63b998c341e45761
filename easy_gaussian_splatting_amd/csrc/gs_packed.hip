// gs_packed.hip -- gsplat's packed meta and sparse gradient rows (rasterization(packed=True, sparse_grad=True)).
//
// The pipeline stays dense: projection, lists, blend and both backward passes work on [C][N] arrays.  Packing is a compaction of
// what the call hands out, behind the pipeline -- the visible (camera, Gaussian) pairs, radii > 0, in row-major order of (c, n):
//
//   pack_flags_kernel    one thread per Gaussian walks its C cameras: the pair flags [C*N] and, when asked, behind them the
//                        flag "some camera saw it" [N]
//   (gs_scan_rows_i32 of gs_refine.hip: ONE inclusive scan over the flags [C*N (+ N)] as one row)
//   pack_totals_kernel   the two totals {nnz, nu} into page-locked host memory: the call's one host read
//   pack_gather_kernel   one thread per SOURCE pair: coalesced reads, and per visible pair one store into each packed array
//                        (consecutive visible pairs land in consecutive rows: the stores of a wave are one dense run)
//   pack_take_kernel     generic row gather of 1..4 32-bit words by the same scan (tiles_per_gauss, .grad / .absgrad of means2d,
//                        the value rows and ids of the sparse gradients)
//   pack_remap_kernel    flatten_ids: dense pair index -> packed row
//
// Eager-path kernels: no step guard.  Fixed order, no atomics, plain vector stores; every store is bounds-checked against the
// totals the host read.
#include "gs_common.h"

namespace gs {

constexpr int kPackThreads = 256;

__global__ __launch_bounds__(kPackThreads) void pack_flags_kernel(int C, int64_t N, const int32_t* __restrict__ radii,
                                                                  int32_t* __restrict__ flags, int want_seen) {
    const int64_t n = (int64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (n >= N) return;
    int any = 0;
    for (int c = 0; c < C; ++c) {
        const int f = radii[(int64_t)c * N + n] > 0 ? 1 : 0;
        flags[(int64_t)c * N + n] = f;
        any |= f;
    }
    if (want_seen) flags[(int64_t)C * N + n] = any;
}

// incl: the inclusive scan of [pair flags | seen flags] as ONE row, so the seen part carries nnz as its base
__global__ void pack_totals_kernel(int64_t pairs, int64_t N, int want_seen, const int32_t* __restrict__ incl,
                                   int64_t* __restrict__ totals_host) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t nnz = incl[pairs - 1];
    totals_host[0] = nnz;
    totals_host[1] = want_seen ? (int64_t)incl[pairs + N - 1] - nnz : 0;
    __threadfence_system();
}

struct PackGatherArgs {
    int64_t N, nnz;
    const int32_t *radii, *incl;
    const float2* means2d;
    const float *depths, *conics, *opacities;
    int opac_per_cam;
    int64_t *camera_ids, *gaussian_ids;
    int32_t* radii_out;
    float2* means2d_out;
    float *depths_out, *conics_out, *opacities_out;
};

__global__ __launch_bounds__(kPackThreads) void pack_gather_kernel(const PackGatherArgs a) {
    const int64_t n = (int64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (n >= a.N) return;
    const int c = blockIdx.y;
    const int64_t i = (int64_t)c * a.N + n;
    const int32_t r = a.radii[i];
    if (r <= 0) return;
    const int64_t o = (int64_t)a.incl[i] - 1;
    if (o < 0 || o >= a.nnz) return;   // (cannot happen with the scan of these radii: no store leaves the packed arrays)
    a.camera_ids[o] = c;
    a.gaussian_ids[o] = n;
    a.radii_out[o] = r;
    a.means2d_out[o] = a.means2d[i];
    a.depths_out[o] = a.depths[i];
    const float k0 = a.conics[3 * i], k1 = a.conics[3 * i + 1], k2 = a.conics[3 * i + 2];
    a.conics_out[3 * o] = k0; a.conics_out[3 * o + 1] = k1; a.conics_out[3 * o + 2] = k2;
    a.opacities_out[o] = a.opacities[a.opac_per_cam ? i : n];
}

// out[incl[i] - base - 1][:] = src[i][:] for every i the scan steps at (incl[i] > incl[i - 1], incl[-1] = base); ids[...] = i
template <int W>
__global__ __launch_bounds__(kPackThreads) void pack_take_kernel(int64_t n_src, int64_t n_out, const int32_t* __restrict__ incl, int32_t base,
                                                                 const uint32_t* __restrict__ src, uint32_t* __restrict__ out,
                                                                 int64_t* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (i >= n_src) return;
    const int32_t cur = incl[i], prev = i > 0 ? incl[i - 1] : base;
    if (cur <= prev) return;
    const int64_t o = (int64_t)cur - base - 1;
    if (o < 0 || o >= n_out) return;
    if (src != nullptr) {
        if (W == 1) {
            out[o] = src[i];
        } else if (W == 2) {
            reinterpret_cast<uint2*>(out)[o] = reinterpret_cast<const uint2*>(src)[i];
        } else if (W == 3) {
            const uint32_t x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
            out[3 * o] = x; out[3 * o + 1] = y; out[3 * o + 2] = z;
        } else {
            reinterpret_cast<uint4*>(out)[o] = reinterpret_cast<const uint4*>(src)[i];
        }
    }
    if (ids != nullptr) ids[o] = i;
}

__global__ __launch_bounds__(kPackThreads) void pack_remap_kernel(int64_t n, int64_t pairs, const int32_t* __restrict__ flatten_ids,
                                                                  const int32_t* __restrict__ incl, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t f = flatten_ids[i];
    // every listed entry is a visible pair (its tile count is > 0 only where radii > 0): incl steps at f, and incl[f] - 1 is its row
    out[i] = (f >= 0 && f < pairs) ? incl[f] - 1 : -1;
}

static inline unsigned pack_blocks(int64_t n) { return (unsigned)((n + kPackThreads - 1) / kPackThreads); }

}  // namespace gs

using namespace gs;

extern "C" int gs_pack_flags(void* stream, int C, int64_t N, const int32_t* radii, int want_seen, int32_t* flags, int32_t* incl,
                             int32_t* scan_workspace, int64_t* totals_host_mapped) {
    GS_REQUIRE(C >= 1 && N >= 1, "C >= 1, N >= 1 (an empty call has nothing to pack: the caller knows its totals)");
    GS_REQUIRE((int64_t)C * N + N < (1ll << 31), "C*N + N must fit int32");
    GS_REQUIRE(radii && flags && incl && scan_workspace && totals_host_mapped, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t pairs = (int64_t)C * N, total = pairs + (want_seen ? N : 0);
    hipLaunchKernelGGL(pack_flags_kernel, dim3(pack_blocks(N)), dim3(kPackThreads), 0, st, C, N, radii, flags, want_seen);
    GS_LAUNCH_CHECK("pack_flags_kernel");
    const int rc = gs_scan_rows_i32(stream, 1, total, flags, incl, scan_workspace);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(pack_totals_kernel, dim3(1), dim3(64), 0, st, pairs, N, want_seen, (const int32_t*)incl, totals_host_mapped);
    GS_LAUNCH_CHECK("pack_totals_kernel");
    return GS_OK;
}

extern "C" int gs_pack_gather(void* stream, int C, int64_t N, int64_t nnz, const int32_t* radii, const int32_t* incl, const float* means2d,
                              const float* depths, const float* conics, const float* opacities, int opacities_per_camera,
                              int64_t* camera_ids, int64_t* gaussian_ids, int32_t* radii_out, float* means2d_out, float* depths_out,
                              float* conics_out, float* opacities_out) {
    GS_REQUIRE(C >= 1 && N >= 1 && C <= 65535, "1 <= C <= 65535, N >= 1");
    GS_REQUIRE((int64_t)C * N < (1ll << 31), "C*N must fit int32");
    GS_REQUIRE(nnz >= 0 && nnz <= (int64_t)C * N, "0 <= nnz <= C*N");
    if (nnz == 0) return GS_OK;
    GS_REQUIRE(radii && incl && means2d && depths && conics && opacities && camera_ids && gaussian_ids && radii_out && means2d_out &&
               depths_out && conics_out && opacities_out, "null pointer");
    GS_REQUIRE(((uintptr_t)means2d & 7) == 0 && ((uintptr_t)means2d_out & 7) == 0, "means2d rows must be 8-byte aligned");
    PackGatherArgs a;
    a.N = N; a.nnz = nnz; a.radii = radii; a.incl = incl; a.means2d = reinterpret_cast<const float2*>(means2d);
    a.depths = depths; a.conics = conics; a.opacities = opacities; a.opac_per_cam = opacities_per_camera ? 1 : 0;
    a.camera_ids = camera_ids; a.gaussian_ids = gaussian_ids; a.radii_out = radii_out;
    a.means2d_out = reinterpret_cast<float2*>(means2d_out); a.depths_out = depths_out; a.conics_out = conics_out;
    a.opacities_out = opacities_out;
    hipLaunchKernelGGL(pack_gather_kernel, dim3(pack_blocks(N), (unsigned)C), dim3(kPackThreads), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("pack_gather_kernel");
    return GS_OK;
}

extern "C" int gs_pack_take(void* stream, int64_t n_src, int64_t n_out, int words, const int32_t* incl, int32_t base, const void* src,
                            void* out, int64_t* ids_out) {
    GS_REQUIRE(n_src >= 0 && n_src < (1ll << 31), "0 <= n_src < 2^31");
    GS_REQUIRE(n_out >= 0 && n_out <= n_src, "0 <= n_out <= n_src");
    GS_REQUIRE(words >= 1 && words <= 4, "rows of 1..4 32-bit words");
    GS_REQUIRE((src == nullptr) == (out == nullptr), "src and out come together");
    if (n_out == 0 || (src == nullptr && ids_out == nullptr)) return GS_OK;
    GS_REQUIRE(incl != nullptr, "null scan");
    const uintptr_t align = words == 2 ? 7 : (words == 4 ? 15 : 3);
    GS_REQUIRE(((uintptr_t)src & align) == 0 && ((uintptr_t)out & align) == 0, "rows must be aligned to their size (4, 8, 4, 16 bytes)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(pack_blocks(n_src)), block(kPackThreads);
    const uint32_t* s = (const uint32_t*)src;
    uint32_t* o = (uint32_t*)out;
    switch (words) {
        case 1: hipLaunchKernelGGL(pack_take_kernel<1>, grid, block, 0, st, n_src, n_out, incl, base, s, o, ids_out); break;
        case 2: hipLaunchKernelGGL(pack_take_kernel<2>, grid, block, 0, st, n_src, n_out, incl, base, s, o, ids_out); break;
        case 3: hipLaunchKernelGGL(pack_take_kernel<3>, grid, block, 0, st, n_src, n_out, incl, base, s, o, ids_out); break;
        default: hipLaunchKernelGGL(pack_take_kernel<4>, grid, block, 0, st, n_src, n_out, incl, base, s, o, ids_out); break;
    }
    GS_LAUNCH_CHECK("pack_take_kernel");
    return GS_OK;
}

extern "C" int gs_pack_remap(void* stream, int64_t n, int64_t pairs, const int32_t* flatten_ids, const int32_t* incl, int32_t* out) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31) && pairs >= 0 && pairs < (1ll << 31), "0 <= n, pairs < 2^31");
    if (n == 0) return GS_OK;
    GS_REQUIRE(flatten_ids && incl && out, "null pointer");
    hipLaunchKernelGGL(pack_remap_kernel, dim3(pack_blocks(n)), dim3(kPackThreads), 0, (hipStream_t)stream, n, pairs, flatten_ids, incl, out);
    GS_LAUNCH_CHECK("pack_remap_kernel");
    return GS_OK;
}
