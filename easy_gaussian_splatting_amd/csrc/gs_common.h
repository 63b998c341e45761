// gs_common.h -- internal helpers shared by the gfx950 translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <utility>

#include "../../include/gs_raster.h"

namespace gs {

void set_error(const char* fmt, ...);

#define GS_HIP_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            gs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                          __LINE__);                                                         \
            return GS_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

#define GS_LAUNCH_CHECK(name)                                                                \
    do {                                                                                     \
        hipError_t _e = hipGetLastError();                                                   \
        if (_e != hipSuccess) {                                                              \
            gs::set_error("launch of %s failed: %s", name, hipGetErrorString(_e));           \
            return GS_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

// (the attribute is raised once per kernel and size: nothing but launches reaches the stream afterwards, which
//  keeps a warmed-up pipeline capturable into a hipGraph)
inline int ensure_lds(const void* fn, size_t bytes) {
    if (bytes > 64 * 1024) {
        static std::mutex mu;
        static std::map<std::pair<int, const void*>, size_t> done;
        int dev = 0;
        GS_HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lock(mu);
        size_t& have = done[{dev, fn}];
        if (have < bytes) {
            GS_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            have = bytes;
        }
    }
    return GS_OK;
}

#define GS_REQUIRE(cond, msg)                                                                \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            gs::set_error("invalid argument: %s (%s)", msg, #cond);                          \
            return GS_ERR_ARG;                                                               \
        }                                                                                    \
    } while (0)

constexpr int kWave = 64;

// Step guard (gs_guard_set, include/gs_raster.h): a device int64[4] info block {I, n_buckets, max tile, flags} plus
// the capacities the caller sized its list buffers for.  While set (per host thread), gs_bin_count raises
// flags when a capacity is exceeded and every kernel that walks or fills the lists -- and the kernels that
// apply the step (statistics, Adam) -- returns at once when flags != 0.
struct Guard {
    const int64_t* info;   // device pointer, nullptr = unguarded
    int64_t cap_isects;    // capacity of the intersection-indexed buffers
    int64_t cap_tile;      // longest tile list the sort classes launched can take
    int per_call;          // gs_guard_set_call: the flags belong to ONE call -- its first flag writer overwrites info[3]
};
Guard current_guard();
// Host mirror of the info block (gs_info_mirror_set): page-locked, device-visible host memory the tile scan writes the
// eight info words into directly -- the eager seam learns the list sizes without a device-to-host copy on the stream.
int64_t* current_info_mirror();
// Host mirror of a training forward's walk record (gs_walk_mirror_set): int64[4] {work units, storage units, rows, flags}.
int64_t* current_walk_mirror();
__device__ __forceinline__ bool guard_tripped(const int64_t* info) { return info != nullptr && info[3] != 0; }

// Depth rounds (gs_rounds_set, include/gs_raster.h): the list stages, the blend forward and the row gather of the backward run
// the frame's Gaussians in TWO rounds -- the front slab by depth first, the rest only into tiles the front slab has not
// finished.  `phase` 0: off; 1: front round; 2: back round; 3: behind both (the backward: rows of the two rounds are two ranges);
// 4: the front round alone (a tile it leaves live voids the step: GS_FLAG_BACK) -- the list stages see it as 1.
struct Rounds {
    int64_t* blk;        // device int64[GS_ROUND_WORDS]
    uint8_t* live;       // [tiles]  1: the front round left the tile with live pixels
    float4* state;       // [tiles][4][64]  pixel states of the live tiles, the front round's lanes' own
    int32_t* tile_rec;   // [tiles][8]  training: the quadrant sublists' lengths and part-filled work units
    int phase;
};
Rounds current_rounds();
// the back round has nothing to do: the front round left no live tile (its kernels return at once)
__device__ __forceinline__ bool round_idle(const int64_t* blk, int phase) { return phase == 2 && blk[GS_ROUND_LIVE] == 0; }

// Gradient rows in front of slot s (training: gs_blend_fwd's row-base scan).  The scan leaves ONE base per 16 slots -- a base per
// slot was 4 bytes written per LISTED intersection for the 2 % a saturated scene walks (65 us at 57 M) --; the reader adds the
// popcounts of the slot's predecessors inside its group: one aligned 16-byte load of their 4-bit quadrant masks.  *slot_mask (if
// asked for) = the slot's own mask.  s may be the slot one past the end (its group exists; bytes at or beyond s are not looked at).
__device__ __forceinline__ int rows_before(const int32_t* __restrict__ row_base16, const uint8_t* __restrict__ qmask, int s, int* slot_mask = nullptr) {
    const int g = s >> 4, k = s & 15;
    const uint4 q = reinterpret_cast<const uint4*>(qmask)[g];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    int n = row_base16[g];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = min(max(k - 4 * j, 0), 4);                        // bytes of word j in front of the slot
        const uint32_t m = b >= 4 ? 0xffffffffu : ((1u << (8 * b)) - 1u);
        n += __popc(w[j] & m & 0x0f0f0f0fu);
    }
    if (slot_mask) *slot_mask = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xfu);
    return n;
}

// Workspace layout of the binning stage (all offsets in bytes, 256-B aligned).
struct BinLayout {
    int groups;          // Gaussian groups per camera
    int64_t per_group;   // Gaussians per group
    size_t hist_off;     // u32 [C*groups][tiles]   per-group tile histogram -> per-group tile base
    size_t tile_cnt_off; // u32 [C*tiles]
    size_t grp_tot_off;  // u32 [C*groups]          intersections emitted by each group
    size_t grp_base_off; // u32 [C*groups]          exclusive scan of the above
    size_t items_off;    // i32 work lists of the sort classes above 1024 keys (gs_binning.hip: class_items_kernel)
    size_t total;
};
BinLayout bin_layout(int C, int64_t N, int tiles);

// i / w for the small non-negative integers of a tile footprint (i < 2^20, w <= 2^12), w's reciprocal formed once per
// footprint: exact ((i + 0.5) / w is at least 0.5 / w away from an integer, far beyond fp32 rounding), and 3 instructions
// instead of the ~35 of a run-time integer division -- which was 20 % of the projection kernel's instruction count.
__device__ __forceinline__ int div_by_width(int i, float inv_w) { return (int)(((float)i + 0.5f) * inv_w); }

// The footprint record of a Gaussian, four u32 words: x0 | x1 << 16, y0 | y1 << 16, tile mask, count -- the tile rectangle
// [x0, x1) x [y0, y1) and which of its tiles are listed.  A rectangle of at most kMaskTiles tiles carries a row-major bit per
// tile and count = popcount(mask); a larger one is full: mask all ones, count = its area.  count == 0: not listed (an invisible
// Gaussian leaves four zero words).  Written by project_fwd_kernel, narrowed by the depth rounds (gs_rounds.hip), read by the
// list stages (gs_binning.hip).  kMaskTiles is the width of the mask word -- a format constant, not a tuning knob.
constexpr int kMaskTiles = 32;
__device__ __forceinline__ uint32_t fp_span(int lo, int hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }
__device__ __forceinline__ uint4 fp_pack(int x0, int x1, int y0, int y1, uint32_t mask, uint32_t count) {
    return make_uint4(fp_span(x0, x1), fp_span(y0, y1), mask, count);
}
__device__ __forceinline__ void fp_unpack(uint4 fp, int& x0, int& x1, int& y0, int& y1) {
    x0 = fp.x & 0xffff; x1 = fp.x >> 16; y0 = fp.y & 0xffff; y1 = fp.y >> 16;
}
// the mask of a rectangle all of whose tiles are listed
__device__ __forceinline__ uint32_t fp_full_mask(int rect_tiles) { return rect_tiles >= kMaskTiles ? 0xffffffffu : ((1u << rect_tiles) - 1u); }
// the rank of tile (tx, ty) among the listed tiles of a footprint (row-major over the rectangle / the set mask bits: the
// order in which the Gaussian's gradient rows are numbered), or -1 when the footprint does not list the tile
__device__ __forceinline__ int fp_rank(uint4 fp, int tx, int ty) {
    int x0, x1, y0, y1;
    fp_unpack(fp, x0, x1, y0, y1);
    if (tx < x0 || tx >= x1 || ty < y0 || ty >= y1) return -1;
    const int w = x1 - x0, idx = (ty - y0) * w + (tx - x0);
    if (w * (y1 - y0) > kMaskTiles) return idx;
    return (fp.z >> idx) & 1u ? __popc(fp.z & ((1u << idx) - 1u)) : -1;
}

// ---- wavefront helpers (wave = 64 lanes on gfx950) ----
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

template <typename T>
__device__ __forceinline__ T wave_incl_scan_add(T v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        T o = __shfl_up(v, d, 64);
        if (lane_id() >= d) v += o;
    }
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_reduce_add(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Sum over the 64 lanes with DPP only (no LDS crossbar): two quad permutes and two mirrors leave every lane of a 16-lane row with
// the row's sum, row_bcast:15 / row_bcast:31 carry the rows along; lane 63 holds the total, handed to every lane as a scalar.
// Six full-rate v_add_f32_dpp per value instead of six ds_bpermute round trips (wave_reduce_add): for wave-wide sums on a
// latency-bound path (gs_rowsum_body.inc).  Fixed order -> reproducible.
__device__ __forceinline__ float wave_reduce_add_dpp(float v) {
#define GS_DPP_ADD(ctrl, row_mask) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, row_mask, 0xf, false))
    GS_DPP_ADD(0xB1, 0xf);    // quad_perm [1,0,3,2]
    GS_DPP_ADD(0x4E, 0xf);    // quad_perm [2,3,0,1]
    GS_DPP_ADD(0x141, 0xf);   // row_half_mirror
    GS_DPP_ADD(0x140, 0xf);   // row_mirror
    GS_DPP_ADD(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    GS_DPP_ADD(0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef GS_DPP_ADD
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Sums of the colour quads (float4 2 of a 12-float gradient row: gs_blend_bwd / gs_blend_bwd_ch) of each lane's rows [r0, r0 + nr):
// gs_channel_grads' channel gradients and gs_depth_grads' depth gradient.  The rows of consecutive Gaussians are contiguous (gs_blend_fwd's
// row-base scan), so the wave's rows are ONE range, read 64 rows (an item) at a time, a row per lane.  An item that lies inside one
// Gaussian's range -- and the run of such items behind it -- is summed per lane and closed by one DPP reduction; otherwise the item
// is staged in LDS and every Gaussian adds its own rows of it in row order.  Fixed order: reproducible sums.
__device__ __forceinline__ float4 quad_sums_wave(const float4* __restrict__ rows, int nr, int r0, float4* item) {
    const int lane = lane_id();
    const int incl = wave_incl_scan_add(nr);
    const int o = incl - nr;
    const int T = __builtin_amdgcn_readlane(incl, 63);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (T == 0) return s;   // wave-uniform
    const unsigned long long fb = __ballot(nr > 0);
    const int R0 = __shfl(r0, __builtin_ctzll(fb), 64);
    auto fetch = [&](int it) {
        const int j = 64 * it + lane;
        return j < T ? rows[3 * (int64_t)(R0 + j) + 2] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    const int n_items = (T + 63) >> 6;
    float4 cur = fetch(0);
    int it = 0;
    while (it < n_items) {
        const int jb = 64 * it;
        const int lo = max(o, jb) - jb, hi = min(o + nr, jb + 64) - jb;   // this Gaussian's rows inside the item
        const unsigned long long whole = __ballot(nr > 0 && lo == 0 && hi == 64);
        if (whole) {   // wave-uniform
            const int owner = __builtin_ctzll(whole);
            const int last = (__shfl(o + nr, owner, 64) >> 6) - 1;   // the last item that is all this Gaussian's
            float4 p = cur;
#pragma unroll 4
            for (int k = it + 1; k <= last; ++k) {
                const float4 b = fetch(k);
                p.x += b.x; p.y += b.y; p.z += b.z; p.w += b.w;
            }
            const float tx = wave_reduce_add_dpp(p.x), ty = wave_reduce_add_dpp(p.y), tz = wave_reduce_add_dpp(p.z),
                        tw = wave_reduce_add_dpp(p.w);
            if (lane == owner) { s.x += tx; s.y += ty; s.z += tz; s.w += tw; }
            it = last + 1;
            if (it < n_items) cur = fetch(it);
            continue;
        }
        item[lane] = cur;
        __builtin_amdgcn_wave_barrier();   // (LDS operations of one wave complete in issue order)
        for (int r = max(lo, 0); r < hi; ++r) {
            const float4 b = item[r];
            s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
        }
        __builtin_amdgcn_wave_barrier();
        ++it;
        if (it < n_items) cur = fetch(it);
    }
    return s;
}

// Block-wide exclusive scan for blockDim.x <= 1024 (16 waves).  `scratch` >= 17 entries of T.
template <typename T>
__device__ __forceinline__ T block_excl_scan_add(T v, T* scratch, T* total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    T incl = wave_incl_scan_add(v);
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        T w = lane < nw ? scratch[lane] : T(0);
        T wi = wave_incl_scan_add(w);
        if (lane < nw) scratch[lane] = wi - w;
        if (lane == nw - 1) scratch[16] = wi;
    }
    __syncthreads();
    T res = incl - v + scratch[wave];
    *total = scratch[16];
    __syncthreads();
    return res;
}

// One Adam update (gs_adam.hip; also applied in place by the fused projection-backward + Adam kernel of gs_project.hip and
// by gs_sh_adam_views):  isbc2 = 1/sqrt(1-beta2^t),  ss = lr/(1-beta1^t), both formed on the host from (double)beta.
// It is Adam at the fp32 betas the ABI receives: 1.f - b is exact for b in [0.5, 1], so decay and increment belong to one
// beta.  Within the bounds of tests/adam_ref.py of that Adam in fp64; exp_avg_sq at a relative 1.3e-5 from torch's
// `_single_tensor_adam`, whose increment is fl32(0.001) and not 1 - fl32(0.999) (gs_adam.hip's header).
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float b1, float b2, float eps,
                                      float isbc2, float ss) {
    m = fmaf(b1, m, (1.f - b1) * g);
    v = fmaf(b2, v, (1.f - b2) * g * g);
    const float denom = sqrtf(v) * isbc2 + eps;
    p = p - ss * (m / denom);
}

// x as it is, hidden from the optimizer: a product behind it is rounded on its own instead of fused into the add that reads it
// (the library is built with -ffp-contract=fast; autograd rounds every product and every sum separately)
__device__ __forceinline__ float fp_opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// exp(x) as the compiler lowers expf without -ffp-contract=fast (torch.exp's device kernel, bit for bit): 2^(x log2 e) with log2 e in
// two parts, the integer part split off, v_exp_f32 of the rest, ldexp.  The library's own expf is built with contraction on, which
// fuses the product in front of `ph - e` into an fma and counts its rounding error twice (up to a few ulp off).
__device__ __forceinline__ float exp_ref(float x) {
    const float c = 0x1.715476p+0f, cc = 0x1.4ae0bep-26f;
    const float ph = fp_opaque(x * c);
    const float pl = fmaf(x, cc, fmaf(x, c, -ph));
    const float e = __builtin_rintf(ph);
    const float a = fp_opaque(ph - e) + pl;
    float r = __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
    r = x < -0x1.9d1da0p+6f ? 0.f : r;
    return x > 0x1.62e430p+6f ? __builtin_huge_valf() : r;
}

// Scale-ratio regulariser of one Gaussian (the reference's GaussianModel.get_regularization_dict): l = its log-scales, R = the
// largest ratio left free, g = the upstream gradient of its term (lambda * (1 / N) as torch forms it on the device).  Returns
// max(max_k s_k / min_k s_k, R) - R, s = exp(l) (exp_ref), and writes d(g * term)/dl into gl[3] in torch autograd's fp32 sequence:
// clamp(min=R) passes g where ratio >= R; div: g / amin for the max, -g * ((amax / amin) / amin) for the min; amax / amin
// backward: (part / count) * mask, so tied maxima or minima share evenly; the two parts summed, then * s (exp backward).
// Every gl[k] is a rounded value of its own (fp_opaque): the caller adds it to a render gradient as autograd does.
__device__ __forceinline__ float scale_reg_term(float l0, float l1, float l2, float R, float g, float gl[3]) {
    const float s[3] = {exp_ref(l0), exp_ref(l1), exp_ref(l2)};
    const float mx = fmaxf(fmaxf(s[0], s[1]), s[2]), mn = fminf(fminf(s[0], s[1]), s[2]);
    const float ratio = mx / mn;
    const float gc = ratio >= R ? g : 0.f;
    const float pmax = gc / mn, pmin = -gc * ((mx / mn) / mn);
    const float cmax = (float)((s[0] == mx) + (s[1] == mx) + (s[2] == mx)), cmin = (float)((s[0] == mn) + (s[1] == mn) + (s[2] == mn));
    const float qmax = pmax / cmax, qmin = pmin / cmin;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = fp_opaque(qmax * (s[k] == mx ? 1.f : 0.f)), b = fp_opaque(qmin * (s[k] == mn ? 1.f : 0.f));
        gl[k] = fp_opaque(fp_opaque(a + b) * s[k]);
    }
    return fmaxf(ratio, R) - R;
}
// g of scale_reg_term as torch forms it on the device: lambda (the mul by a Python float) times 1 / N (mean backward divides by a
// scalar, which torch's device kernel does as a multiply by the scalar's reciprocal)
inline float scale_reg_upstream(float lambda, int64_t N) { return lambda * (1.0f / (float)N); }

// Budget regulariser of one Gaussian (mcmc.MCMCStrategy.regularization: a mean(opacity) + b mean(scale)): o = sigmoid(logit) and
// s_k = exp(l_k) in fp64; the gradients ga o (1 - o) and gb s_k with the float32 upstream factors ga = fl32(a / N) and
// gb = fl32(b / (3 N)), each rounded to float32 once.  No product feeds a sum here, so the stand-alone pass (gs_mcmc_reg) and the
// fused one (project_bwd_budget_kernel) round alike whatever the compiler contracts around them.
__device__ __forceinline__ void budget_reg_term(float logit, float l0, float l1, float l2, float ga, float gb, double* o_out,
                                                double s_out[3], float* g_logit, float gl[3]) {
    const double o = 1.0 / (1.0 + exp(-(double)logit));
    const double s[3] = {exp((double)l0), exp((double)l1), exp((double)l2)};
    *o_out = o;
    *g_logit = (float)((double)ga * (o * (1.0 - o)));
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_out[k] = s[k]; gl[k] = (float)((double)gb * s[k]); }
}
inline float budget_reg_upstream(double coeff, int64_t count) { return (float)(coeff / (double)count); }

// streaming (non-temporal) 16-byte accesses for data that is touched once and then dead
#ifdef __HIPCC__
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4* p) {
    const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store4(float4 x, float4* p) {
    f4v v; v.x = x.x; v.y = x.y; v.z = x.z; v.w = x.w;
    __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p));
}

#endif

}  // namespace gs
