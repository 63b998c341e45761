// gs_knn.hip -- exact k-nearest-neighbour distances of a 3-D point cloud, for gfx950: what the reference's constructor takes
// from sklearn.neighbors.NearestNeighbors (model/utils.py:8-11) to size the initial Gaussians, k <= GS_KNN_MAX_K.
//
//   knn_bbox_partial_kernel / knn_bbox_final_kernel : the cloud's bounding box (min / max: order-free, no atomics)
//   knn_codes_kernel   : 63-bit Morton code of every point, 21 bits per axis of the box-normalised coordinate; an axis of zero
//                        (or non-finite) extent gives 0 on that axis
//   -- the caller sorts the point indices by code (gs_raster.h: gs_knn_codes / gs_knn_dists) --
//   knn_gather_kernel  : the points in sorted order as float4 {x, y, z, bits of the caller's index}, cut into LEAVES of GS_KNN_LEAF
//                        = 64 consecutive points, each with its tight box; the last leaf is padded with +inf points
//   knn_nodes_kernel   : the box of every NODE = GS_KNN_FANOUT consecutive leaves
//   knn_search_kernel  : one wave per leaf, one lane per query.  The k best SQUARED distances are a sorted register list
//                        (compile-time K, insertion = K median-of-three operations); seeded from the lane's own leaf, then a walk
//                        over all nodes and, inside a node some lane cannot rule out, over its leaves.  A box is visited when ANY
//                        lane's squared distance to it is strictly below that lane's k-th best (a wave-uniform branch: the 64
//                        queries are Morton neighbours); the box comes in through uniform loads, a visited leaf's 64 candidates
//                        through ONE coalesced 1 KB load into the wave's LDS slice and 64 broadcast ds_read_b128.
//
// Exact, whatever the order: a pair's squared distance is d2(q - c) below, one fixed sequence of roundings; a box's is the same
// d2 of the per-axis gaps max(lo - q, q - hi, 0).  Rounding is monotone, so for every point c inside the box each |q - c| is at
// least the gap as rounded, and d2 -- non-decreasing in each magnitude -- of the gaps is at most the point's own d2: a box is
// skipped only when none of its points could enter the list, and a tie (not strictly below) cannot change the list's VALUES.
// The rows therefore depend on the input alone -- not on the sort's tie order, the leaf size or the walk -- and two calls give
// the same bits.  Clouds of coincident points have a k-th best of 0 after the seed and skip every box: no all-pairs scan.
// Every loop runs to a count fixed before it starts (nodes, leaves per node, 64 points); coordinates never become indices.  A
// NaN or an infinity in the input gives a meaningless row and nothing worse.
#include "gs_common.h"

namespace gs {

constexpr int kLeaf = GS_KNN_LEAF, kFan = GS_KNN_FANOUT;
constexpr int kBoxBlocks = 1024;                  // partial boxes of the first reduction stage
static_assert(kLeaf == kWave, "one wave per leaf, one lane per query");

struct KnnLayout {       // byte offsets into the workspace, 256-byte aligned
    int64_t n_leaf, n_node;
    size_t partial_off;  // float [kBoxBlocks][8]   partial boxes {lo xyz, -, hi xyz, -}
    size_t bbox_off;     // float [8]               the cloud's box
    size_t sorted_off;   // float4 [n_leaf * 64]
    size_t leaf_off;     // float4 [n_leaf][2]      {lo, hi}
    size_t node_off;     // float4 [n_node][2]
    size_t total;
};

static KnnLayout knn_layout(int64_t N) {
    KnnLayout L;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    L.n_leaf = (N + kLeaf - 1) / kLeaf;
    L.n_node = (L.n_leaf + kFan - 1) / kFan;
    L.partial_off = 0;
    L.bbox_off = up(sizeof(float) * 8 * kBoxBlocks);
    L.sorted_off = L.bbox_off + 256;
    L.leaf_off = L.sorted_off + up(sizeof(float4) * (size_t)L.n_leaf * kLeaf);
    L.node_off = L.leaf_off + up(sizeof(float4) * 2 * (size_t)L.n_leaf);
    L.total = L.node_off + up(sizeof(float4) * 2 * (size_t)L.n_node);
    return L;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// block-wide box of the per-thread boxes (256 threads); thread 0 writes {lo, -, hi, -} to out[8]
__device__ __forceinline__ void block_box_store(float lo[3], float hi[3], float* out) {
    __shared__ float red[4][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out[a] = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
            out[4 + a] = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
        }
        out[3] = 0.f; out[7] = 0.f;
    }
}

__global__ __launch_bounds__(256) void knn_bbox_partial_kernel(int N, const float* __restrict__ pts, float* __restrict__ partial) {
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    const int stride = (int)gridDim.x * 256;   // (<= 2^18; i stays below N + 2^18 < 2^31)
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < N; i += stride) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * (int64_t)i + a];
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    }
    block_box_store(lo, hi, partial + 8 * blockIdx.x);
}

__global__ __launch_bounds__(256) void knn_bbox_final_kernel(int n_partial, const float* __restrict__ partial, float* __restrict__ bbox) {
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int i = threadIdx.x; i < n_partial; i += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], partial[8 * i + a]); hi[a] = fmaxf(hi[a], partial[8 * i + 4 + a]); }
    }
    block_box_store(lo, hi, bbox);
}

// bits ..cba of a 21-bit value -> ..00c00b00a
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(256) void knn_codes_kernel(int N, const float* __restrict__ pts, const float* __restrict__ bbox,
                                                        int64_t* __restrict__ codes) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= N) return;
    uint64_t code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = bbox[a], ext = bbox[4 + a] - lo;
        // a flat axis (ext == 0), an overflowing or a NaN extent: cell 0 on this axis, no division by zero
        const float inv = (ext > 0.f && ext < __builtin_huge_valf()) ? 1.f / ext : 0.f;
        const float t = fminf(fmaxf((pts[3 * (int64_t)i + a] - lo) * inv, 0.f), 1.f);   // (fmaxf drops a NaN)
        code |= spread3(min((uint32_t)(t * 2097151.f), 2097151u)) << a;
    }
    codes[i] = (int64_t)code;
}

__global__ __launch_bounds__(256) void knn_gather_kernel(int N, const float* __restrict__ pts, const int32_t* __restrict__ order,
                                                         float4* __restrict__ sorted, float4* __restrict__ leaf_box) {
    const int pos = (int)blockIdx.x * 256 + (int)threadIdx.x;   // (the grid covers n_leaf * 64 slots exactly or runs past: guarded)
    const int n_slots = ((N + kLeaf - 1) / kLeaf) * kLeaf;
    if (pos >= n_slots) return;                                  // wave-uniform: slots come in whole leaves
    const float inf = __builtin_huge_valf();
    float4 p = make_float4(inf, inf, inf, __int_as_float(-1));
    if (pos < N) {
        const int src = order[pos];
        if ((unsigned)src < (unsigned)N)   // (an index outside the cloud is a padded slot, never an address)
            p = make_float4(pts[3 * (int64_t)src], pts[3 * (int64_t)src + 1], pts[3 * (int64_t)src + 2], __int_as_float(src));
    }
    sorted[pos] = p;
    const bool real = __float_as_int(p.w) >= 0;
    const float lx = wave_min(real ? p.x : inf), ly = wave_min(real ? p.y : inf), lz = wave_min(real ? p.z : inf);
    const float hx = wave_max(real ? p.x : -inf), hy = wave_max(real ? p.y : -inf), hz = wave_max(real ? p.z : -inf);
    if (lane_id() == 0) {
        leaf_box[2 * (pos >> 6)] = make_float4(lx, ly, lz, 0.f);
        leaf_box[2 * (pos >> 6) + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

__global__ __launch_bounds__(256) void knn_nodes_kernel(int n_leaf, int n_node, const float4* __restrict__ leaf_box,
                                                        float4* __restrict__ node_box) {
    const int node = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (node >= n_node) return;   // wave-uniform
    const int leaf = node * kFan + lane_id();
    const float inf = __builtin_huge_valf();
    float4 lo = make_float4(inf, inf, inf, 0.f), hi = make_float4(-inf, -inf, -inf, 0.f);
    if (leaf < n_leaf) { lo = leaf_box[2 * leaf]; hi = leaf_box[2 * leaf + 1]; }
    const float lx = wave_min(lo.x), ly = wave_min(lo.y), lz = wave_min(lo.z);
    const float hx = wave_max(hi.x), hy = wave_max(hi.y), hz = wave_max(hi.z);
    if (lane_id() == 0) {
        node_box[2 * node] = make_float4(lx, ly, lz, 0.f);
        node_box[2 * node + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

// THE squared distance: products and sums rounded in this one order wherever a distance is formed (the file's header)
__device__ __forceinline__ float d2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

__device__ __forceinline__ float box_d2(float4 q, float4 lo, float4 hi) {
    const float gx = fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.f);
    return d2(gx, gy, gz);
}

template <int K>
__device__ __forceinline__ void knn_insert(float (&best)[K], float d) {
    // sorted insert that drops the largest: new[i] = median(best[i-1], d, best[i]), downwards so that best[i-1] is still the old one
#pragma unroll
    for (int i = K - 1; i > 0; --i) best[i] = __builtin_amdgcn_fmed3f(best[i - 1], d, best[i]);
    best[0] = fminf(best[0], d);
}

template <int K>
__global__ __launch_bounds__(256) void knn_search_kernel(int n_leaf, int n_node, const float4* __restrict__ sorted,
                                                         const float4* __restrict__ leaf_box, const float4* __restrict__ node_box,
                                                         float* __restrict__ dists) {
    __shared__ float4 cand[4][kLeaf];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    const int own = (int)blockIdx.x * 4 + wave;
    if (own >= n_leaf) return;   // wave-uniform; no block-wide barrier below
    float4* slice = cand[wave];
    const float inf = __builtin_huge_valf();
    const float4 q = sorted[own * kLeaf + lane];
    const int dst = __float_as_int(q.w);
    const bool valid = dst >= 0;   // (a padded slot of the last leaf: takes part in the loads, never in a vote or a store)
    float best[K];
#pragma unroll
    for (int i = 0; i < K; ++i) best[i] = inf;

    // seed: the own leaf, self excluded by INDEX (a coincident point is a neighbour at distance 0)
    slice[lane] = q;
    __builtin_amdgcn_wave_barrier();   // (LDS operations of one wave complete in issue order)
#pragma unroll 8
    for (int j = 0; j < kLeaf; ++j) {
        const float4 c = slice[j];
        const float d = d2(q.x - c.x, q.y - c.y, q.z - c.z);
        knn_insert<K>(best, j == lane ? inf : d);   // (a padded candidate is at +inf: never below anything)
    }
    __builtin_amdgcn_wave_barrier();

#pragma unroll 1
    for (int node = 0; node < n_node; ++node) {
        if (!__any(valid && box_d2(q, node_box[2 * node], node_box[2 * node + 1]) < best[K - 1])) continue;
        const int l1 = min(node * kFan + kFan, n_leaf);
#pragma unroll 1
        for (int leaf = node * kFan; leaf < l1; ++leaf) {
            if (leaf == own) continue;
            if (!__any(valid && box_d2(q, leaf_box[2 * leaf], leaf_box[2 * leaf + 1]) < best[K - 1])) continue;
            slice[lane] = sorted[leaf * kLeaf + lane];
            __builtin_amdgcn_wave_barrier();
#pragma unroll 8
            for (int j = 0; j < kLeaf; ++j) {
                const float4 c = slice[j];
                knn_insert<K>(best, d2(q.x - c.x, q.y - c.y, q.z - c.z));
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (valid) {
#pragma unroll
        for (int i = 0; i < K; ++i) dists[(int64_t)dst * K + i] = sqrtf(best[i]);
    }
}

template <int K>
static void launch_search(hipStream_t st, const KnnLayout& L, const float4* sorted, const float4* leaf_box, const float4* node_box,
                          float* dists) {
    hipLaunchKernelGGL(knn_search_kernel<K>, dim3((unsigned)((L.n_leaf + 3) / 4)), dim3(256), 0, st, (int)L.n_leaf, (int)L.n_node, sorted,
                       leaf_box, node_box, dists);
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_knn_workspace_bytes(int64_t N) {
    if (N < 1 || N > GS_KNN_MAX_N) return 0;
    return knn_layout(N).total;
}

extern "C" int gs_knn_codes(void* stream, int64_t N, const float* points, void* workspace, int64_t* codes) {
    GS_REQUIRE(N >= 2 && N <= GS_KNN_MAX_N, "N must be in [2, GS_KNN_MAX_N = 2^30]: positions and indices are int32");
    GS_REQUIRE(points && workspace && codes, "null pointer");
    GS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    const KnnLayout L = knn_layout(N);
    char* ws = (char*)workspace;
    float* partial = (float*)(ws + L.partial_off);
    float* bbox = (float*)(ws + L.bbox_off);
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = (N + 255) / 256;
    const int pb = (int)(blocks < kBoxBlocks ? blocks : kBoxBlocks);
    hipLaunchKernelGGL(knn_bbox_partial_kernel, dim3((unsigned)pb), dim3(256), 0, st, (int)N, points, partial);
    GS_LAUNCH_CHECK("knn_bbox_partial_kernel");
    hipLaunchKernelGGL(knn_bbox_final_kernel, dim3(1), dim3(256), 0, st, pb, partial, bbox);
    GS_LAUNCH_CHECK("knn_bbox_final_kernel");
    hipLaunchKernelGGL(knn_codes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (int)N, points, bbox, codes);
    GS_LAUNCH_CHECK("knn_codes_kernel");
    return GS_OK;
}

extern "C" int gs_knn_dists(void* stream, int64_t N, int k, const float* points, const int32_t* order, float* dists, void* workspace) {
    GS_REQUIRE(k >= 1 && k <= GS_KNN_MAX_K, "k must be in [1, GS_KNN_MAX_K = 8]");
    GS_REQUIRE(N >= (int64_t)k + 1, "a point needs k OTHER points: N >= k + 1");
    GS_REQUIRE(N <= GS_KNN_MAX_N, "N beyond GS_KNN_MAX_N = 2^30: positions and indices are int32");
    GS_REQUIRE(points && order && dists && workspace, "null pointer");
    GS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    const KnnLayout L = knn_layout(N);
    char* ws = (char*)workspace;
    float4* sorted = (float4*)(ws + L.sorted_off);
    float4* leaf_box = (float4*)(ws + L.leaf_off);
    float4* node_box = (float4*)(ws + L.node_off);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(knn_gather_kernel, dim3((unsigned)((L.n_leaf + 3) / 4)), dim3(256), 0, st, (int)N, points, order, sorted, leaf_box);
    GS_LAUNCH_CHECK("knn_gather_kernel");
    hipLaunchKernelGGL(knn_nodes_kernel, dim3((unsigned)((L.n_node + 3) / 4)), dim3(256), 0, st, (int)L.n_leaf, (int)L.n_node, leaf_box, node_box);
    GS_LAUNCH_CHECK("knn_nodes_kernel");
    switch (k) {
        case 1: launch_search<1>(st, L, sorted, leaf_box, node_box, dists); break;
        case 2: launch_search<2>(st, L, sorted, leaf_box, node_box, dists); break;
        case 3: launch_search<3>(st, L, sorted, leaf_box, node_box, dists); break;
        case 4: launch_search<4>(st, L, sorted, leaf_box, node_box, dists); break;
        case 5: launch_search<5>(st, L, sorted, leaf_box, node_box, dists); break;
        case 6: launch_search<6>(st, L, sorted, leaf_box, node_box, dists); break;
        case 7: launch_search<7>(st, L, sorted, leaf_box, node_box, dists); break;
        default: launch_search<8>(st, L, sorted, leaf_box, node_box, dists); break;
    }
    GS_LAUNCH_CHECK("knn_search_kernel");
    return GS_OK;
}
