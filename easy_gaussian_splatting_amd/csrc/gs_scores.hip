// gs_scores.hip -- blend-weight scores for gfx950: how much every Gaussian contributed to the images.
//
// For a camera c, a Gaussian n and a pixel p the blend TAKES the pair when the pixel is live, sigma >= 0,
// alpha = min(0.999, opacity exp(-sigma)) >= 1/255 and T' = fma(-alpha, T, T) > 1e-4; a taken pair has the weight w = alpha T.
//   score_kernel       : gs_blend_scores -- the replay of a training walk (gs_blend_fwd / gs_blend_fwd_ch with checkpoints) through
//                        the work-unit pipelines of the blend backward (gs_blend.hip: bwd_wave), with the gradient arithmetic, the
//                        colour loads and eight of its eleven sums removed: per (intersection, quadrant) it leaves ONE 16-byte row
//                        (sum of w, max of w, number of taken pixels, 0) at the index the gradient row of the pair would have.
//                        sigma, alpha, w and T' are formed with the instruction sequence of bwd_pair -- which is the forward's --,
//                        so the taken set and every w are the forward's bit for bit.  No atomics: a row has one writer.
//   score_reduce_kernel: gs_score_reduce -- per (camera, Gaussian) the rows of the Gaussian (contiguous: gs_channel_grads' gather)
//                        folded in row order into weight_sum / weight_max / hits [C,N]
//   score_accum_kernel : gs_score_accumulate -- a [C,N] triple + radii folded into running per-Gaussian totals, cameras in order
#include "gs_blend_shared.h"
#include "gs_math.h"

namespace gs {

struct ScoreArgs {
    int C, W, H, tw, tiles;
    const float4* rec;
    const int32_t* walk;
    const int2* qlist;
    const int32_t* qcnt;
    const int4* unit_desc;
    const float4* ckpt;   // only the T plane (.x) is read
    const uint8_t* qmask;
    const int32_t* row_base;
    int cap_units;
    int64_t cap_rows;
    const int32_t* cls_hdr;   // fill classes (unit_classes_launch) or nullptr: every unit runs as class 4 straight from unit_desc
    const int4* cls_desc;
    int cls_cap;
    float4* rows;   // [cap_rows] (sum w, max w, taken pixels as int32 bits, 0)
    const int64_t* guard;
};

struct ScoreEntry {
    float mx, my, hA, Bc, hC, op;
    float s_w, m_w;
    int hits;
};

// bwd_pair of gs_blend.hip without the gradient: the same operations on the same inputs up to T' and the contributor test
__device__ __forceinline__ void score_pair(ScoreEntry& e, const float2 d1, float& T) {
    const float dx = e.mx - d1.x, dy = e.my - d1.y;
    const float sigma = fmaf(dy, fmaf(e.hC, dy, e.Bc * dx), e.hA * dx * dx);   // same op sequence as the forward
    const float vis = fast_exp2(-sigma);
    const float ov = e.op * vis;
    const float alpha = fminf(kAlphaMax, ov);
    const bool ok = T > 0.f && sigma >= 0.f && alpha >= kAlphaMin;
    const float w = fp_opaque(alpha * T);   // (a rounded product of its own, as the forward's: never fused into the sum below)
    const float Tn = fmaf(-alpha, T, T);    // identical to the forward's update
    const bool stop = ok && Tn <= kTMin;
    const bool contrib = ok && !stop;
    const float wm = contrib ? w : 0.f;
    e.s_w += wm;
    e.m_w = fmaxf(e.m_w, wm);
    e.hits += contrib ? 1 : 0;
    T = contrib ? Tn : (stop ? -1.f : T);
}

// One wave: eight work units of ONE fill class E = entries per lane (bwd_wave's pipeline; sT: the unit's 64 checkpoint T in LDS)
template <int E>
__device__ __forceinline__ void score_wave(const ScoreArgs& a, const int4 ud, const bool valid, float* sT, const int r) {
    const int tq = ud.x, su = ud.z;
    const bool first_unit = ud.y == 0;   // the sublist starts here: every pixel inside the image has T = 1
    const int t = tq >> 2, q = tq & 3;
    const int cam = t / a.tiles, tt = t - cam * a.tiles;
    const int tyi = tt / a.tw, txi = tt - tyi * a.tw;
    const int qx0 = txi * GS_TILE + 8 * (q & 1), qy0 = tyi * GS_TILE + 8 * (q >> 1);
    const float fx0 = (float)qx0 + 0.5f, fy0 = (float)qy0 + 0.5f;
    const float4* ckp = a.ckpt + (size_t)su * 64;

    // prologue, branch-free like bwd_wave's: out-of-range pixels / entries load from a valid address and are masked afterwards
    const int n_sub = valid ? a.qcnt[tq] : 0;
    int2 gs[E];
    {
        const int2* qp2 = a.qlist + (size_t)su * kUnit + E * r;
        if constexpr (E == 4) {
            const int4* qp = reinterpret_cast<const int4*>(qp2);
            const int4 g0 = qp[0], g1 = qp[1];
            gs[0] = make_int2(g0.x, g0.y); gs[1] = make_int2(g0.z, g0.w); gs[2] = make_int2(g1.x, g1.y); gs[3] = make_int2(g1.z, g1.w);
        } else if constexpr (E == 2) {
            const int4 g0 = *reinterpret_cast<const int4*>(qp2);
            gs[0] = make_int2(g0.x, g0.y); gs[1] = make_int2(g0.z, g0.w);
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) gs[i] = qp2[i];
        }
    }
    constexpr int kPix = kUnitPixels / kPipeLanes;
    float l_T[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) l_T[i] = reinterpret_cast<const float*>(ckp + (r + kPipeLanes * i))[0];
    const int n_in = min(kPipeLanes * E, n_sub - ud.y * kUnit);   // entries of the sublist that fall into this unit
    float4 rq[E][2];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const bool has = E * r + i < n_in;
        const float4* rp = a.rec + 3 * (size_t)(has ? gs[i].x : 0);
        rq[i][0] = rp[0]; rq[i][1] = rp[1];
    }
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
        const int p = r + kPipeLanes * i;
        const bool inside = valid && (qx0 + (p & 7)) < a.W && (qy0 + (p >> 3)) < a.H;
        sT[p] = inside ? (first_unit ? 1.f : l_T[i]) : -1.f;   // (T < 0: finished or outside the image)
    }
    ScoreEntry e[E];
    int slot[E];
    bool has[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        has[i] = E * r + i < n_in;
        slot[i] = has[i] ? gs[i].y : 0;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 q0 = has[i] ? rq[i][0] : z4, q1 = has[i] ? rq[i][1] : z4;   // (no entry: opacity 0, hence alpha 0)
        e[i].mx = q0.x; e[i].my = q0.y; e[i].hA = q0.z; e[i].Bc = q0.w; e[i].hC = q1.x; e[i].op = q1.y;
        e[i].s_w = 0.f; e[i].m_w = 0.f; e[i].hits = 0;
    }
    __builtin_amdgcn_wave_barrier();

    float T_out = -1.f;
    for (int s = 0; s < kBwdSteps; ++s) {
        float T = dpp_row_shr1(T_out);
        const int p = s - r;
        const bool act = (unsigned)p < (unsigned)kUnitPixels;
        const int pc = min(max(p, 0), kUnitPixels - 1);
        const float ck = sT[pc];
        const float2 d1 = make_float2(fx0 + (float)(pc & 7), fy0 + (float)(pc >> 3));   // pixel centre
        if (r == 0) T = ck;   // head of the pipeline: fed from the checkpoint
        T = act ? T : -1.f;   // pipeline fill / drain: nothing contributes
#pragma unroll
        for (int i = 0; i < E; ++i) score_pair(e[i], d1, T);
        T_out = T;
    }

    // the row of (slot, quadrant), as the gradient rows: rows_before + the rank of the quadrant among the slot's rows
#pragma unroll
    for (int i = 0; i < E; ++i) {
        int m;
        int row = rows_before(a.row_base, a.qmask, slot[i], &m);
        row += __popc((unsigned)m & ((1u << q) - 1u));
        if (has[i] && (int64_t)row < a.cap_rows) a.rows[row] = make_float4(e[i].s_w, e[i].m_w, __int_as_float(e[i].hits), 0.f);
    }
}

__global__ __launch_bounds__(kBwdWaves * 64) void score_kernel(const ScoreArgs a) {
    __shared__ float sT_all[kBwdWaves][kUnitsPerWave][64];   // 2 KB per wave: the checkpoint T of the unit's 64 pixels
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pipe = lane / kPipeLanes, r = lane & (kPipeLanes - 1);
    if (guard_tripped(a.guard)) return;
    if (a.walk[kWalkFlags] != 0 || a.walk[kWalkSkip] != 0) return;   // a void walk (GS_FLAG_UNITS / GS_FLAG_ROWS) or a skipped one: no rows
    // the block's class and its place in it, as blend_bwd_body
    constexpr int kPerBlock = kBwdWaves * kUnitsPerWave;
    int cls = 4, blk = (int)blockIdx.x, n_units, first = 0;
    if (a.cls_hdr == nullptr) {
        n_units = min(a.walk[kWalkUnits], a.cap_units);
    } else {
        const int b4 = (a.cap_units + kPerBlock - 1) / kPerBlock, bt = (a.cls_cap + kPerBlock - 1) / kPerBlock;
        if (blk >= b4) {
            const int k = (blk - b4) / bt;   // 0, 1, 2 -> class 3, 2, 1
            cls = 3 - k; blk -= b4 + k * bt; first = a.cap_units + k * a.cls_cap;
        }
        n_units = min(a.cls_hdr[cls], cls == 4 ? a.cap_units : a.cls_cap);
    }
    const int in_class = (blk * kBwdWaves + wave) * kUnitsPerWave + pipe;
    if ((blk * kBwdWaves + wave) * kUnitsPerWave >= n_units) return;   // wave-uniform
    const bool valid = in_class < n_units;
    float* sT = sT_all[wave][pipe];
    int4 ud = make_int4(0, 0, 0, 0);
    if (valid) ud = a.cls_hdr ? a.cls_desc[first + in_class] : a.unit_desc[in_class];
    if (cls == 4) score_wave<4>(a, ud, valid, sT, r);
    else if (cls == 3) score_wave<3>(a, ud, valid, sT, r);
    else if (cls == 2) score_wave<2>(a, ud, valid, sT, r);
    else score_wave<1>(a, ud, valid, sT, r);
}

// ------------------------------------------------------------------------------------------------
constexpr int kRedThreads = 256;
constexpr int kRedWide = 64;   // a Gaussian with at least this many rows is folded by its whole wave

struct ScoreReduceArgs {
    int64_t CN;
    const int32_t *radii, *tiles_per_gauss, *cum_tiles, *row_base, *walk;
    const uint8_t* qmask;
    const float4* rows;
    int64_t cap_rows;
    float *weight_sum, *weight_max;
    int32_t* hits;
    const int64_t* guard;
};

// One thread per (camera, Gaussian).  Fixed order: a short run of rows is added in row order by its thread; a long one by the
// wave -- lane l rows l, l + 64, ... in order, the 64 partial sums by one DPP reduction -- so two runs agree bit for bit.
__global__ __launch_bounds__(kRedThreads) void score_reduce_kernel(const ScoreReduceArgs a) {
    if (guard_tripped(a.guard)) return;
    const int64_t f = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    const bool in_range = f < a.CN;
    const bool walk_void = a.walk[kWalkFlags] != 0 || a.walk[kWalkSkip] != 0;   // no rows were written: zeros
    const bool vis = in_range && !walk_void && a.radii[f] > 0;
    const int cnt = vis ? a.tiles_per_gauss[f] : 0;
    const int base = vis ? a.cum_tiles[f] : 0;
    int r0 = 0, nr = 0;
    if (cnt > 0) {
        r0 = rows_before(a.row_base, a.qmask, base);
        nr = rows_before(a.row_base, a.qmask, base + cnt) - r0;
        nr = (int)max((int64_t)0, min((int64_t)nr, a.cap_rows - r0));
    }
    float s = 0.f, m = 0.f;
    int h = 0;
    if (nr < kRedWide) {
        for (int j = 0; j < nr; ++j) {
            const float4 v = a.rows[r0 + j];
            s += v.x; m = fmaxf(m, v.y); h += __float_as_int(v.z);
        }
    }
    const int lane = lane_id();
    for (unsigned long long wide = __ballot(nr >= kRedWide); wide; wide &= wide - 1) {   // wave-uniform
        const int owner = __builtin_ctzll(wide);
        const int R0 = __shfl(r0, owner, 64), NR = __shfl(nr, owner, 64);
        float ps = 0.f, pm = 0.f;
        int ph = 0;
        for (int j = lane; j < NR; j += 64) {
            const float4 v = a.rows[R0 + j];
            ps += v.x; pm = fmaxf(pm, v.y); ph += __float_as_int(v.z);
        }
        const float ts = wave_reduce_add_dpp(ps);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) pm = fmaxf(pm, __shfl_xor(pm, d, 64));
        const int th = wave_reduce_add(ph);
        if (lane == owner) { s = ts; m = pm; h = th; }
    }
    if (in_range) { a.weight_sum[f] = s; a.weight_max[f] = m; a.hits[f] = h; }
}

__global__ __launch_bounds__(kRedThreads) void score_accum_kernel(int C, int64_t N, const float* __restrict__ weight_sum,
                                                                  const float* __restrict__ weight_max, const int32_t* __restrict__ hits,
                                                                  const int32_t* __restrict__ radii, double* __restrict__ tot_sum,
                                                                  float* __restrict__ tot_max, int64_t* __restrict__ tot_hits,
                                                                  int32_t* __restrict__ views_seen, int32_t* __restrict__ views_hit,
                                                                  const int64_t* __restrict__ guard) {
    if (guard_tripped(guard)) return;
    const int64_t n = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    if (n >= N) return;
    double s = tot_sum[n];
    float m = tot_max[n];
    int64_t h = tot_hits[n];
    int seen = views_seen[n], hit = views_hit[n];
    for (int c = 0; c < C; ++c) {   // cameras in order
        const int64_t f = (int64_t)c * N + n;
        const int hc = hits[f];
        s += (double)weight_sum[f];
        m = fmaxf(m, weight_max[f]);
        h += (int64_t)hc;
        seen += radii[f] > 0 ? 1 : 0;
        hit += hc > 0 ? 1 : 0;
    }
    tot_sum[n] = s; tot_max[n] = m; tot_hits[n] = h; views_seen[n] = seen; views_hit[n] = hit;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_blend_scores(void* stream, int C, int width, int height, const float* rec, const int32_t* qlist,
                               const int32_t* qcnt, const int32_t* unit_desc, int64_t cap_units, const float* ckpt,
                               const uint8_t* qmask, const int32_t* row_base, const int32_t* walk_state, float* score_rows,
                               int64_t cap_rows, int32_t* unit_classes) {
    GS_REQUIRE(C >= 1 && width > 0 && height > 0 && cap_units >= 0 && cap_units < (1ll << 26), "C>=1, positive image size, 0 <= cap_units < 2^26");
    GS_REQUIRE(cap_rows >= 0 && cap_rows < (1ll << 31), "0 <= cap_rows < 2^31");
    if (cap_units == 0) return GS_OK;
    GS_REQUIRE(rec && qlist && qcnt && unit_desc && ckpt && qmask && row_base && walk_state && score_rows, "null pointer");
    GS_REQUIRE(((uintptr_t)rec & 15) == 0 && ((uintptr_t)qlist & 15) == 0 && ((uintptr_t)unit_desc & 15) == 0 && ((uintptr_t)ckpt & 15) == 0 &&
               ((uintptr_t)qmask & 15) == 0 && ((uintptr_t)score_rows & 15) == 0,
               "rec / qlist / unit_desc / ckpt / qmask / score_rows 16-byte aligned");
    GS_REQUIRE(((uintptr_t)row_base & 3) == 0 && ((uintptr_t)walk_state & 3) == 0 && ((uintptr_t)qcnt & 3) == 0, "int32 arrays 4-byte aligned");
    GS_REQUIRE(current_rounds().phase == 0, "the walk of depth rounds is two ranges of rows: scores are one-round only");
    ScoreArgs a;
    a.C = C; a.W = width; a.H = height;
    a.tw = (width + GS_TILE - 1) / GS_TILE;
    a.tiles = a.tw * ((height + GS_TILE - 1) / GS_TILE);
    a.rec = reinterpret_cast<const float4*>(rec);
    a.qlist = reinterpret_cast<const int2*>(qlist); a.qcnt = qcnt; a.walk = walk_state;
    a.unit_desc = reinterpret_cast<const int4*>(unit_desc); a.cap_units = (int)cap_units;
    a.ckpt = reinterpret_cast<const float4*>(ckpt); a.qmask = qmask; a.row_base = row_base;
    a.rows = reinterpret_cast<float4*>(score_rows); a.cap_rows = cap_rows;
    a.guard = current_guard().info;
    unsigned grid = (unsigned)((cap_units + kUnitsPerWave * kBwdWaves - 1) / (kUnitsPerWave * kBwdWaves));
    a.cls_hdr = nullptr; a.cls_desc = nullptr; a.cls_cap = 0;
    if (unit_classes) {
        GS_REQUIRE(((uintptr_t)unit_classes & 15) == 0, "unit_classes must be 16-byte aligned");
        a.cls_hdr = unit_classes; a.cls_desc = reinterpret_cast<const int4*>(unit_classes + kClsHdrInts);
        a.cls_cap = (int)unit_class_region(C, width, height);
        const int rc = unit_classes_launch((hipStream_t)stream, walk_state, a.unit_desc, qcnt, (int)cap_units, a.cls_cap, unit_classes, a.guard);
        if (rc != GS_OK) return rc;
        grid += 3u * (unsigned)(a.cls_cap / (kUnitsPerWave * kBwdWaves));
    }
    hipLaunchKernelGGL(score_kernel, dim3(grid), dim3(kBwdWaves * 64), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("score_kernel");
    return GS_OK;
}

extern "C" int gs_score_reduce(void* stream, int C, int64_t N, const int32_t* radii, const int32_t* tiles_per_gauss,
                               const int32_t* cum_tiles, const float* score_rows, int64_t cap_rows, const int32_t* row_base,
                               const uint8_t* qmask, const int32_t* walk_state, float* weight_sum, float* weight_max, int32_t* hits) {
    GS_REQUIRE(C >= 1 && N >= 0 && cap_rows >= 0 && cap_rows < (1ll << 31), "C>=1, N>=0, 0 <= cap_rows < 2^31");
    if (N == 0) return GS_OK;
    GS_REQUIRE(radii && tiles_per_gauss && cum_tiles && score_rows && row_base && qmask && walk_state && weight_sum && weight_max && hits,
               "null pointer");
    GS_REQUIRE(((uintptr_t)score_rows & 15) == 0 && ((uintptr_t)qmask & 15) == 0, "score_rows / qmask 16-byte aligned");
    GS_REQUIRE((((uintptr_t)weight_sum | (uintptr_t)weight_max | (uintptr_t)hits | (uintptr_t)radii) & 3) == 0, "outputs 4-byte aligned");
    GS_REQUIRE(current_rounds().phase == 0, "the rows of depth rounds are two ranges: scores are one-round only");
    ScoreReduceArgs a;
    a.CN = (int64_t)C * N;
    a.radii = radii; a.tiles_per_gauss = tiles_per_gauss; a.cum_tiles = cum_tiles; a.row_base = row_base; a.walk = walk_state;
    a.qmask = qmask; a.rows = reinterpret_cast<const float4*>(score_rows); a.cap_rows = cap_rows;
    a.weight_sum = weight_sum; a.weight_max = weight_max; a.hits = hits;
    a.guard = current_guard().info;
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)((a.CN + kRedThreads - 1) / kRedThreads)), dim3(kRedThreads), 0,
                       (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("score_reduce_kernel");
    return GS_OK;
}

extern "C" int gs_score_accumulate(void* stream, int C, int64_t N, const float* weight_sum, const float* weight_max,
                                   const int32_t* hits, const int32_t* radii, double* total_weight_sum, float* total_weight_max,
                                   int64_t* total_hits, int32_t* views_seen, int32_t* views_hit) {
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    if (N == 0) return GS_OK;
    GS_REQUIRE(weight_sum && weight_max && hits && radii && total_weight_sum && total_weight_max && total_hits && views_seen && views_hit,
               "null pointer");
    GS_REQUIRE((((uintptr_t)total_weight_sum | (uintptr_t)total_hits) & 7) == 0, "total_weight_sum / total_hits 8-byte aligned");
    GS_REQUIRE((((uintptr_t)weight_sum | (uintptr_t)weight_max | (uintptr_t)hits | (uintptr_t)radii | (uintptr_t)total_weight_max |
                 (uintptr_t)views_seen | (uintptr_t)views_hit) & 3) == 0, "32-bit arrays 4-byte aligned");
    hipLaunchKernelGGL(score_accum_kernel, dim3((unsigned)((N + kRedThreads - 1) / kRedThreads)), dim3(kRedThreads), 0, (hipStream_t)stream,
                       C, N, weight_sum, weight_max, hits, radii, total_weight_sum, total_weight_max, total_hits, views_seen, views_hit,
                       current_guard().info);
    GS_LAUNCH_CHECK("score_accum_kernel");
    return GS_OK;
}
