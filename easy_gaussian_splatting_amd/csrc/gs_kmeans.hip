// gs_kmeans.hip -- Lloyd's k-means on the device, for gfx950: the codebook over the higher SH bands of compress.save_compact
// (DESIGN.md "Exporting a trained model").  Labels, distances and centroids are the functions gs_kmeans.h states, bit for bit.
//
//   kmeans_prep_kernel   : the centroids k-major and zero-padded, ct[Dp][Kp] (Dp = D rounded up to the MFMA's k-step of 2, Kp = K
//                          rounded up to the 128-centroid tile), and their norms cn[Kp]; a padded column has norm NaN -- its score is
//                          NaN and never wins.
//   kmeans_assign_kernel : a block of 4 waves owns 128 points, staged once k-major in LDS, and walks the centroids in LDS tiles of
//                          128.  A wave owns 32 of the points against the tile's 128 centroids: four accumulator tiles of
//                          v_mfma_f32_32x32x2_f32, the f32-input MFMA whose result is bit for bit the k-ordered fmaf chain.  In the
//                          C/D layout (column = centroid = lane & 31, the 16 rows = points in registers) every lane keeps a running
//                          best (score, index) per row over the columns it owns -- it meets them in ascending index order, so a strict
//                          < keeps the smallest index -- and the 32 lanes of a half-wave are reduced lexicographically ONCE, after the
//                          last tile.  No score is ever stored.  (The usual 2 x 2 tiles per wave would halve the LDS reads, which
//                          are 5 per 256 MFMA cycles here, and need a cross-wave reduction; 1 x 4 needs none.)
//   kmeans_update_kernel : one wave per cluster walks its segment of `order` in ascending order, lanes across D (coalesced gathers),
//                          one fp64 accumulator per (cluster, dimension).
// No atomics, no scratch, every loop to a count fixed before it starts; labels index memory only after a range check.
#include "gs_common.h"
#include "gs_kmeans.h"

namespace gs {

constexpr int kKmTile = 128;      // points per block = centroids per LDS tile
typedef float f32x16 __attribute__((ext_vector_type(16)));

static int64_t km_kp(int64_t K) { return (K + kKmTile - 1) / kKmTile * kKmTile; }
static int km_dp(int D) { return (D + 1) & ~1; }
static size_t km_up(size_t b) { return (b + 255) & ~(size_t)255; }

// element (k, col) of a k-major [Dp][128] LDS tile.  The two half-waves of an MFMA operand read rows k and k + 1 at the same
// columns: odd rows are stored with the column's bit 5 flipped, so the halves fall into different banks.
__device__ __forceinline__ int km_lds(int k, int col) { return k * kKmTile + (col ^ ((k & 1) << 5)); }

__global__ __launch_bounds__(256) void kmeans_prep_kernel(int K, int Kp, int D, int Dp, const float* __restrict__ centroids,
                                                          float* __restrict__ ct, float* __restrict__ cn) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= Kp) return;
    if (j < K) {
        const float* c = centroids + (int64_t)j * D;
        for (int k = 0; k < D; ++k) ct[(int64_t)k * Kp + j] = c[k];
        for (int k = D; k < Dp; ++k) ct[(int64_t)k * Kp + j] = 0.f;
        cn[j] = kmeans_norm(c, D);
    } else {
        for (int k = 0; k < Dp; ++k) ct[(int64_t)k * Kp + j] = 0.f;
        cn[j] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void kmeans_assign_kernel(int N, int K, int Kp, int D, int Dp, const float* __restrict__ x,
                                                            const float* __restrict__ centroids, const float* __restrict__ ct,
                                                            const float* __restrict__ cn, int32_t* __restrict__ labels,
                                                            float* __restrict__ dist2) {
    extern __shared__ float km_smem[];
    float* Xs = km_smem;                       // [Dp][128] the block's points
    float* Cs = km_smem + Dp * kKmTile;        // [Dp][128] the current centroid tile
    int32_t* Ls = (int32_t*)(Cs + Dp * kKmTile);   // [128] the block's labels
    const int t = (int)threadIdx.x, lane = t & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t p0 = (int64_t)blockIdx.x * kKmTile;
    {   // the points, once: thread = (point, k parity); rows behind N and the padded k are zeros
        const int p = t & 127;
        const bool real = p0 + p < N;
        const float* xp = x + (p0 + (real ? p : 0)) * D;
        for (int k = t >> 7; k < Dp; k += 2) Xs[km_lds(k, p)] = (real && k < D) ? xp[k] : 0.f;
    }
    float bs[16];
    int32_t bi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { bs[i] = __builtin_huge_valf(); bi[i] = kKmNoLabel; }

    const int acol = wave * 32 + r;
    const int steps = Dp >> 1;
#pragma unroll 1
    for (int j0 = 0; j0 < Kp; j0 += kKmTile) {
        __syncthreads();   // the previous tile has been read (first pass: nothing to wait for but the barrier is cheap)
        {
            const int j = t & 127;
            for (int k = t >> 7; k < Dp; k += 2) Cs[km_lds(k, j)] = ct[(int64_t)k * Kp + j0 + j];
        }
        __syncthreads();
        f32x16 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
        for (int s = 0; s < steps; ++s) {
            const int k = 2 * s + h;   // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
            const float a = Xs[km_lds(k, acol)];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Cs[km_lds(k, q * 32 + r)], acc[q], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // column tiles in ascending index order
            const int32_t idx = j0 + q * 32 + r;
            const float n2 = cn[idx];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float s = kmeans_score(acc[q][i], n2);
                if (s < bs[i]) { bs[i] = s; bi[i] = idx; }
            }
        }
    }
    // the 32 columns of a half-wave, lexicographic on (score, index); register i is row (i & 3) + 8 (i >> 2) + 4 h of the wave's 32
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) {
            const float os = __shfl_xor(bs[i], d, 64);
            const int32_t oi = __shfl_xor(bi[i], d, 64);
            if (kmeans_better(os, oi, bs[i], bi[i])) { bs[i] = os; bi[i] = oi; }
        }
        if (r == 0) Ls[wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] = kmeans_final_label(bi[i]);
    }
    __syncthreads();
    if (t < kKmTile && p0 + t < N) {
        int32_t l = Ls[t];
        l = (uint32_t)l < (uint32_t)K ? l : 0;   // (always inside: a label is never an address unchecked)
        labels[p0 + t] = l;
        dist2[p0 + t] = kmeans_dist2(x + (p0 + t) * D, centroids + (int64_t)l * D, D);
    }
}

__global__ __launch_bounds__(256) void kmeans_update_kernel(int N, int K, int D, const float* __restrict__ x,
                                                            const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                            float* __restrict__ centroids, int32_t* __restrict__ counts) {
    const int lane = lane_id();
    const int j = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= K) return;   // wave-uniform; no block-wide barrier below
    const int s0 = min(max(seg[j], 0), N), s1 = min(max(seg[j + 1], s0), N);   // (a segment is never trusted beyond `order`)
    const bool lo = lane < D, hi = lane + 64 < D;
    double sum0 = 0.0, sum1 = 0.0;
    int32_t count = 0;
#pragma unroll 1
    for (int i0 = s0; i0 < s1; i0 += 64) {
        const int mine = i0 + lane < s1 ? order[i0 + lane] : -1;   // 64 members at once: their gathers do not wait for each other
        const int n = min(64, s1 - i0);
        for (int m = 0; m < n; ++m) {
            const int idx = __shfl(mine, m, 64);
            if ((unsigned)idx >= (unsigned)N) continue;   // wave-uniform: an index outside the points is skipped, never an address
            const float* xp = x + (int64_t)idx * D;
            if (lo) sum0 += (double)xp[lane];
            if (hi) sum1 += (double)xp[lane + 64];
            ++count;
        }
    }
    if (lane == 0) counts[j] = count;
    if (count > 0) {   // an empty cluster keeps its centroid's bits
        if (lo) centroids[(int64_t)j * D + lane] = kmeans_mean(sum0, count);
        if (hi) centroids[(int64_t)j * D + lane + 64] = kmeans_mean(sum1, count);
    }
}

struct KmLayout {   // byte offsets into the workspace, 256-byte aligned
    int64_t Kp;
    int Dp;
    size_t ct_off;   // float [Dp][Kp]
    size_t cn_off;   // float [Kp]
    size_t total;
};
static KmLayout km_layout(int64_t K, int D) {
    KmLayout L;
    L.Kp = km_kp(K);
    L.Dp = km_dp(D);
    L.ct_off = 0;
    L.cn_off = km_up(sizeof(float) * (size_t)L.Dp * (size_t)L.Kp);
    L.total = L.cn_off + km_up(sizeof(float) * (size_t)L.Kp);
    return L;
}
static bool km_sizes_ok(int64_t N, int64_t K, int D) {
    return N >= 1 && N <= GS_KMEANS_MAX_N && K >= 1 && K <= GS_KMEANS_MAX_K && D >= 1 && D <= GS_KMEANS_MAX_D;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_kmeans_workspace_bytes(int64_t N, int64_t K, int D) {
    if (!km_sizes_ok(N, K, D)) return 0;
    return km_layout(K, D).total;
}

extern "C" int gs_kmeans_assign(void* stream, int64_t N, int64_t K, int D, const float* x, const float* centroids, int32_t* labels,
                                float* dist2, void* workspace) {
    GS_REQUIRE(km_sizes_ok(N, K, D), "N in [1, GS_KMEANS_MAX_N = 2^30], K in [1, GS_KMEANS_MAX_K = 2^24], D in [1, GS_KMEANS_MAX_D = 128]");
    GS_REQUIRE(x && centroids && labels && dist2 && workspace, "null pointer");
    GS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    const KmLayout L = km_layout(K, D);
    float* ct = (float*)((char*)workspace + L.ct_off);
    float* cn = (float*)((char*)workspace + L.cn_off);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = sizeof(float) * (size_t)(2 * L.Dp * kKmTile + kKmTile);   // <= 131.5 KB of the CU's 160 KB
    if (int rc = ensure_lds((const void*)kmeans_assign_kernel, lds)) return rc;
    hipLaunchKernelGGL(kmeans_prep_kernel, dim3((unsigned)((L.Kp + 255) / 256)), dim3(256), 0, st, (int)K, (int)L.Kp, D, L.Dp, centroids, ct, cn);
    GS_LAUNCH_CHECK("kmeans_prep_kernel");
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)((N + kKmTile - 1) / kKmTile)), dim3(256), lds, st, (int)N, (int)K, (int)L.Kp, D,
                       L.Dp, x, centroids, ct, cn, labels, dist2);
    GS_LAUNCH_CHECK("kmeans_assign_kernel");
    return GS_OK;
}

extern "C" int gs_kmeans_update(void* stream, int64_t N, int64_t K, int D, const float* x, const int32_t* order, const int32_t* seg,
                                float* centroids, int32_t* counts) {
    GS_REQUIRE(km_sizes_ok(N, K, D), "N in [1, GS_KMEANS_MAX_N = 2^30], K in [1, GS_KMEANS_MAX_K = 2^24], D in [1, GS_KMEANS_MAX_D = 128]");
    GS_REQUIRE(x && order && seg && centroids && counts, "null pointer");
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (int)N, (int)K, D, x, order,
                       seg, centroids, counts);
    GS_LAUNCH_CHECK("kmeans_update_kernel");
    return GS_OK;
}
