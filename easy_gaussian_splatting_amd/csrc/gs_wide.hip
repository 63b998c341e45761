// gs_wide.hip -- colour features of more than four channels, rendered in chunks of four over ONE set of tile lists.
// The blend kernels stay the 1 .. 4 channel ones of gs_blend.hip; what is here moves a chunk in and out of them, for gfx950:
//   rec_colors_chunk_kernel    : the colour quad of the blend record (floats 8..11, zero above `count`) from channels
//                                [first, first + count) of a D-wide colour array              (gs_channels.hip: rec_colors_kernel)
//   channel_grads_chunk_kernel : the per-Gaussian sums of the gradient rows' colour quads, stored at stride D, offset `first`
//                                (same quad_sums_wave, same camera order as channel_grads_kernel)
//   rows_accumulate_kernel     : floats 0..7 of every gradient row (the geometry part gs_project_bwd sums) folded into an
//                                accumulator of n_rows x 12 floats; the first chunk stores (and zeroes floats 8..11), later ones add
//   chunk_scatter / _gather    : dense [P, count] <-> channels [first, first + count) of a [P, D] image
// All stream: a float4 per lane wherever the layout allows it (count = 4 of a D that is a multiple of 4; the rows always).
#include "gs_common.h"

namespace gs {

constexpr int kWideThreads = 256;

__global__ __launch_bounds__(kWideThreads) void rec_colors_chunk_kernel(int64_t CN, int64_t N, int D, int first, int count, int vec,
                                                                        const float* __restrict__ colors, int per_cam,
                                                                        const int32_t* __restrict__ radii, float4* __restrict__ rec,
                                                                        const int64_t* guard) {
    if (guard_tripped(guard)) return;
    const int64_t f = (int64_t)blockIdx.x * kWideThreads + threadIdx.x;
    if (f >= CN || radii[f] <= 0) return;
    const float* src = colors + (int64_t)D * (per_cam ? f : f % N) + first;
    float4 c;
    if (vec) {
        c = *reinterpret_cast<const float4*>(src);
    } else {
        c.x = src[0];
        c.y = count > 1 ? src[1] : 0.f;
        c.z = count > 2 ? src[2] : 0.f;
        c.w = count > 3 ? src[3] : 0.f;
    }
    rec[3 * f + 2] = c;
}

struct ChunkGradArgs {
    int C, D, first, count, per_cam, vec;
    int64_t N;
    const int32_t *radii, *tiles_per_gauss, *cum_tiles, *row_base;
    const uint8_t* qmask;
    const float4* rows;   // [rows][3]: the colour quad is float4 2 of a row
    float* v_colors;      // [N, D] or [C, N, D]
    const int64_t* guard;
};

__device__ __forceinline__ void store_chunk(float* d, int count, int vec, const float4 v) {
    if (vec) { *reinterpret_cast<float4*>(d) = v; return; }
    d[0] = v.x;
    if (count > 1) d[1] = v.y;
    if (count > 2) d[2] = v.z;
    if (count > 3) d[3] = v.w;
}

// One thread per Gaussian n; the cameras in order (channel_grads_kernel of gs_channels.hip with a strided destination).
__global__ __launch_bounds__(kWideThreads) void channel_grads_chunk_kernel(const ChunkGradArgs a) {
    __shared__ float4 items[kWideThreads / 64][64];
    if (guard_tripped(a.guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kWideThreads + threadIdx.x;
    const bool in_range = n < a.N;
    float4* item = items[threadIdx.x >> 6];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < a.C; ++c) {
        const int64_t f = (int64_t)c * a.N + n;
        const bool vis = in_range && a.radii[f] > 0;
        const int cnt = vis ? a.tiles_per_gauss[f] : 0;
        const int base = vis ? a.cum_tiles[f] : 0;
        int r0 = 0, nr = 0;
        if (cnt > 0) { r0 = rows_before(a.row_base, a.qmask, base); nr = rows_before(a.row_base, a.qmask, base + cnt) - r0; }
        const float4 s = quad_sums_wave(a.rows, nr, r0, item);
        if (a.per_cam) {
            if (in_range) store_chunk(a.v_colors + (int64_t)a.D * f + a.first, a.count, a.vec, s);
        } else {
            acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
        }
    }
    if (!a.per_cam && in_range) store_chunk(a.v_colors + (int64_t)a.D * n + a.first, a.count, a.vec, acc);
}

// One thread per float4 of a row (three per row): quads 0 and 1 are folded, quad 2 -- the colour quad, which belongs to the chunk
// and not to the sum -- is zeroed once, by the first chunk.
template <bool FIRST>
__global__ __launch_bounds__(kWideThreads) void rows_accumulate_kernel(int64_t n_quads, const float4* __restrict__ rows,
                                                                       float4* __restrict__ acc, const int64_t* guard) {
    if (guard_tripped(guard)) return;
    const int64_t i = (int64_t)blockIdx.x * kWideThreads + threadIdx.x;
    if (i >= n_quads) return;
    const bool colour = i % 3 == 2;
    if (FIRST) {
        acc[i] = colour ? make_float4(0.f, 0.f, 0.f, 0.f) : rows[i];
    } else if (!colour) {
        const float4 r = rows[i];
        float4 s = acc[i];
        s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
        acc[i] = s;
    }
}

// dense [P, CNT] <-> channels [first, first + CNT) of [P, D].  VEC (CNT = 4, D a multiple of 4): a float4 per pixel; otherwise one
// thread per element of the dense side, which stays coalesced.
// The step guard as an image sees it: a walk that outgrew its capacities (GS_FLAG_UNITS / GS_FLAG_ROWS, raised by the training blend
// right in front of the scatter) voids the walk -- the image that launch wrote is complete and has to reach its channels.
__device__ __forceinline__ bool guard_tripped_image(const int64_t* info) {
    return info != nullptr && (info[3] & ~(int64_t)(GS_FLAG_UNITS | GS_FLAG_ROWS)) != 0;
}

template <int CNT, bool VEC, bool SCATTER>
__global__ __launch_bounds__(kWideThreads) void chunk_copy_kernel(int64_t n_pixels, int D, int first, const float* __restrict__ src,
                                                                  float* __restrict__ dst, const int64_t* guard) {
    if (guard_tripped_image(guard)) return;
    const int64_t i = (int64_t)blockIdx.x * kWideThreads + threadIdx.x;
    if (VEC) {
        if (i >= n_pixels) return;
        const int64_t wide = (i * D + first) >> 2;   // (D and first are multiples of 4)
        if (SCATTER) reinterpret_cast<float4*>(dst)[wide] = reinterpret_cast<const float4*>(src)[i];
        else reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[wide];
    } else {
        if (i >= n_pixels * CNT) return;
        const int64_t p = i / CNT;
        const int64_t wide = p * D + first + (i - p * CNT);
        if (SCATTER) dst[wide] = src[i];
        else dst[i] = src[wide];
    }
}

template <bool SCATTER>
static int chunk_copy_launch(void* stream, int64_t n_pixels, int D, int count, int first, const float* src, float* dst) {
    const bool vec = count == 4 && D % 4 == 0;
    const int64_t items = vec ? n_pixels : n_pixels * count;
    const dim3 grid((unsigned)((items + kWideThreads - 1) / kWideThreads)), block(kWideThreads);
    const int64_t* guard = current_guard().info;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((chunk_copy_kernel<4, true, SCATTER>), grid, block, 0, st, n_pixels, D, first, src, dst, guard);
    else if (count == 1) hipLaunchKernelGGL((chunk_copy_kernel<1, false, SCATTER>), grid, block, 0, st, n_pixels, D, first, src, dst, guard);
    else if (count == 2) hipLaunchKernelGGL((chunk_copy_kernel<2, false, SCATTER>), grid, block, 0, st, n_pixels, D, first, src, dst, guard);
    else if (count == 3) hipLaunchKernelGGL((chunk_copy_kernel<3, false, SCATTER>), grid, block, 0, st, n_pixels, D, first, src, dst, guard);
    else hipLaunchKernelGGL((chunk_copy_kernel<4, false, SCATTER>), grid, block, 0, st, n_pixels, D, first, src, dst, guard);
    GS_LAUNCH_CHECK("chunk_copy_kernel");
    return GS_OK;
}

}  // namespace gs

using namespace gs;

// the chunk [first, first + count) of D channels: chunks are four wide and start at multiples of four, the last one may be shorter
#define GS_REQUIRE_CHUNK()                                                                                                   \
    GS_REQUIRE(D >= 1 && first >= 0 && first % 4 == 0 && count >= 1 && count <= 4 && (int64_t)first + count <= D,            \
               "channels: D >= 1, first a multiple of 4, count in 1..4, first + count <= D")
// a D-wide float array read or written at the chunk: float4 accesses where the chunk is a whole quad of a D that is a multiple of 4
#define GS_WIDE_ALIGNED(p) ((((uintptr_t)(p)) & ((count == 4 && D % 4 == 0) ? 15 : 3)) == 0)

extern "C" int gs_rec_colors_chunk(void* stream, int C, int64_t N, int D, int first, int count, const float* colors,
                                   int colors_per_camera, const int32_t* radii, float* rec) {
    GS_REQUIRE_CHUNK();
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    const int64_t CN = (int64_t)C * N;
    if (CN == 0) return GS_OK;   // (no Gaussian: nothing is read, as gs_project_fwd)
    GS_REQUIRE(colors && radii && rec, "null pointer");
    GS_REQUIRE(((uintptr_t)rec & 15) == 0 && GS_WIDE_ALIGNED(colors), "rec must be 16-byte aligned, colors as its chunks are read");
    GS_REQUIRE(CN < (1ll << 31) * kWideThreads, "C * N exceeds one grid");
    hipLaunchKernelGGL(rec_colors_chunk_kernel, dim3((unsigned)((CN + kWideThreads - 1) / kWideThreads)), dim3(kWideThreads), 0,
                       (hipStream_t)stream, CN, N, D, first, count, (count == 4 && D % 4 == 0) ? 1 : 0, colors, colors_per_camera ? 1 : 0,
                       radii, reinterpret_cast<float4*>(rec), current_guard().info);
    GS_LAUNCH_CHECK("rec_colors_chunk_kernel");
    return GS_OK;
}

extern "C" int gs_channel_grads_chunk(void* stream, int C, int64_t N, int D, int first, int count, int colors_per_camera,
                                      const int32_t* radii, const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows,
                                      const int32_t* row_base, const uint8_t* qmask, float* v_colors) {
    GS_REQUIRE_CHUNK();
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(current_rounds().phase == 0, "the rows of depth rounds are two ranges: channel gradients are one-round only");
    if (N == 0) return GS_OK;   // (no Gaussian: nothing is read or written, as gs_project_bwd)
    GS_REQUIRE(radii && tiles_per_gauss && cum_tiles && rows && row_base && qmask && v_colors, "null pointer");
    GS_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)qmask & 15) == 0 && GS_WIDE_ALIGNED(v_colors),
               "rows / qmask 16-byte aligned, v_colors as its chunks are written");
    ChunkGradArgs a;
    a.C = C; a.D = D; a.first = first; a.count = count; a.per_cam = colors_per_camera ? 1 : 0; a.vec = (count == 4 && D % 4 == 0) ? 1 : 0;
    a.N = N;
    a.radii = radii; a.tiles_per_gauss = tiles_per_gauss; a.cum_tiles = cum_tiles; a.row_base = row_base; a.qmask = qmask;
    a.rows = reinterpret_cast<const float4*>(rows); a.v_colors = v_colors;
    a.guard = current_guard().info;
    hipLaunchKernelGGL(channel_grads_chunk_kernel, dim3((unsigned)((N + kWideThreads - 1) / kWideThreads)), dim3(kWideThreads), 0,
                       (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("channel_grads_chunk_kernel");
    return GS_OK;
}

extern "C" int gs_rows_accumulate(void* stream, int64_t n_rows, const float* rows, float* acc, int first_chunk) {
    GS_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "0 <= n_rows < 2^31 gradient rows");
    GS_REQUIRE(rows && acc, "null pointer");
    GS_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)acc & 15) == 0, "rows / acc 16-byte aligned");
    GS_REQUIRE(rows != acc, "rows and acc are two buffers");
    if (n_rows == 0) return GS_OK;
    const int64_t quads = 3 * n_rows;
    const dim3 grid((unsigned)((quads + kWideThreads - 1) / kWideThreads)), block(kWideThreads);
    const int64_t* guard = current_guard().info;
    if (first_chunk)
        hipLaunchKernelGGL(rows_accumulate_kernel<true>, grid, block, 0, (hipStream_t)stream, quads, reinterpret_cast<const float4*>(rows),
                           reinterpret_cast<float4*>(acc), guard);
    else
        hipLaunchKernelGGL(rows_accumulate_kernel<false>, grid, block, 0, (hipStream_t)stream, quads, reinterpret_cast<const float4*>(rows),
                           reinterpret_cast<float4*>(acc), guard);
    GS_LAUNCH_CHECK("rows_accumulate_kernel");
    return GS_OK;
}

extern "C" int gs_chunk_scatter(void* stream, int64_t n_pixels, int D, int first, int count, const float* src, float* dst) {
    GS_REQUIRE_CHUNK();
    GS_REQUIRE(n_pixels >= 0 && n_pixels < (1ll << 36), "0 <= n_pixels < 2^36");
    GS_REQUIRE(src && dst, "null pointer");
    GS_REQUIRE(GS_WIDE_ALIGNED(src) && GS_WIDE_ALIGNED(dst), "src / dst aligned to the chunk's accesses (16 bytes for whole quads)");
    if (n_pixels == 0) return GS_OK;
    return chunk_copy_launch<true>(stream, n_pixels, D, count, first, src, dst);
}

extern "C" int gs_chunk_gather(void* stream, int64_t n_pixels, int D, int first, int count, const float* src, float* dst) {
    GS_REQUIRE_CHUNK();
    GS_REQUIRE(n_pixels >= 0 && n_pixels < (1ll << 36), "0 <= n_pixels < 2^36");
    GS_REQUIRE(src && dst, "null pointer");
    GS_REQUIRE(GS_WIDE_ALIGNED(src) && GS_WIDE_ALIGNED(dst), "src / dst aligned to the chunk's accesses (16 bytes for whole quads)");
    if (n_pixels == 0) return GS_OK;
    return chunk_copy_launch<false>(stream, n_pixels, D, count, first, src, dst);
}
