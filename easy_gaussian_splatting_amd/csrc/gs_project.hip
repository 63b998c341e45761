// gs_project.hip -- per-Gaussian stages for gfx950:
//   project_fwd_kernel : P-fwd + SH-fwd fused (one pass over means/quats/scales/shs); when training with SH colours it
//                        also leaves d colour / d view direction (sh_jac), so that the backward reads no coefficient
//   project_bwd_kernel : gradient-row reduction (compact rows, a row per lane: row_sum_wave) + SH-bwd + P-bwd fused, no atomics;
//                        <DEG, true>: Adam and update_statistics applied in the same pass (gs_project_bwd_adam)
//   project_cam_kernel : camera gradients (gs_project_bwd_cam): the chain recomputed from the projection backward's per-Gaussian
//                        outputs, 15 fp64 terms reduced per block without atomics; cam_sum_kernel adds a camera's block partials
// The [N,K,3] SH block (192 B per Gaussian at SH3, 300 B at SH4) is moved through LDS with coalesced 16-byte accesses and read per
// thread at an odd row stride (3K+1 dwords) so the per-thread walk over its own row is bank-conflict free.  The
// geometry half of the forward is VALU-bound (the fp64 chain), the rest HBM streams and gathers.
#include "gs_common.h"
#include "gs_math.h"

namespace gs {

#define GS_PROJ_THREADS 256
constexpr int kProjThreads = GS_PROJ_THREADS;

struct ProjFwdArgs {
    int C, K, colors_per_camera, W, H, tw, th, tight, activations;
    int64_t N;
    float eps2d, near_p, far_p, radius_clip;
    const float *means, *quats, *scales, *opacities, *colors_in, *sh_rest, *viewmats, *Ks;
    int32_t* radii;
    float *means2d, *depths, *conics, *colors_out;
    float4* rec;
    uint4* bbox;
    int32_t* tiles_per_gauss;
    uint2* rect_ref;   // optional [C*N]: the 3-sigma tile rectangle itself (x0 | x1 << 16, y0 | y1 << 16), whatever `tight` does to bbox
    float4* sh_jac;    // optional, 9 floats per (camera, Gaussian): d(pre-clamp colour)/d(view direction) of the visible Gaussians, for a backward without the coefficients
    float* compensations;   // antialiased mode (project_fwd_aa_kernel only) [C*N]: rho = sqrt(det(cov2_0) / det(cov2)), 0 where culled
};

// activations != 0: `scales` / `opacities` hold the reference model's parameters (log-scales, logit
// opacities, /root/reference/model/gaussian.py:98-103) and exp / sigmoid are applied here, so that the
// model's four activation kernels (two forward, two backward) disappear.
__device__ __forceinline__ float act_scale(float v, int activations) { return activations ? expf(v) : v; }
__device__ __forceinline__ float act_opacity(float v, int activations) { return activations ? 1.0f / (1.0f + expf(-v)) : v; }

// dynamic LDS carve (dwords): [0,32) camera | [32, 32+256) visibility | SH tile 256*(3K+1)
__device__ __forceinline__ void load_camera(const float* viewmats, const float* Ks, int c, int W,
                                            int H, float* lds_cam, Camera& cam) {
    if (threadIdx.x == 0) {
        Camera tmp;
        make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, tmp);
        const float* src = reinterpret_cast<const float*>(&tmp);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(Camera) / 4); ++i) lds_cam[i] = src[i];
    }
    __syncthreads();
    float* dst = reinterpret_cast<float*>(&cam);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(Camera) / 4); ++i) dst[i] = lds_cam[i];
}

// The same in two steps, for a kernel whose first phase does not need the camera: thread 0 leaves it in LDS (+ block barrier),
// every thread reads it when it gets there -- the ~30 camera registers are then not live across that phase (project_bwd_kernel's
// row sum is its register peak).
__device__ __forceinline__ void stage_camera(const float* viewmats, const float* Ks, int c, int W, int H, float* lds_cam) {
    if (threadIdx.x == 0) {
        Camera tmp;
        make_camera(viewmats + 16 * c, Ks + 9 * c, W, H, tmp);
        const float* src = reinterpret_cast<const float*>(&tmp);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(Camera) / 4); ++i) lds_cam[i] = src[i];
    }
    __syncthreads();
}
__device__ __forceinline__ void read_camera(const float* lds_cam, Camera& cam) {
    // (member by member: through a float* alias of the struct one instantiation kept the whole Camera as a 100-byte stack object)
    static_assert(sizeof(Camera) == 21 * sizeof(float), "Camera layout");
#pragma unroll
    for (int i = 0; i < 9; ++i) cam.R[i] = lds_cam[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { cam.t[i] = lds_cam[9 + i]; cam.pos[i] = lds_cam[12 + i]; }
    cam.fx = lds_cam[15]; cam.fy = lds_cam[16]; cam.cx = lds_cam[17]; cam.cy = lds_cam[18];
    cam.half_w = lds_cam[19]; cam.half_h = lds_cam[20];
}

// Cooperative global -> LDS copy of the first `ka3` floats of every visible Gaussian's SH row.
// KC > 0 fixes K at compile time (K = 16 is the reference's SH3 layout) so the per-element
// row/offset divisions become multiply-shifts; KC = 0 keeps K a run-time value.
template <int KC>
__device__ __forceinline__ void stage_sh_rows(const float* __restrict__ shs, int64_t n0, int rows,
                                              int Krt, int ka3, const int* vis, float* tile) {
    const int K = KC > 0 ? KC : Krt;
    const int row_f = 3 * K, stride = row_f + 1;
    const float* src = shs + n0 * row_f;
    if (ka3 == row_f && (row_f & 3) == 0) {
        // All of a thread's (<= 12) 16-byte loads are issued before the first LDS write: a single
        // loop "load, then store to LDS" makes hipcc wait for each load before the next is issued
        // (the LDS store may alias the visibility flags it reads), i.e. 12 serial HBM round trips.
        const int per_row = row_f >> 2, total4 = rows * per_row;
        const float4* src4 = reinterpret_cast<const float4*>(src);
        constexpr int kMaxQ = 12;   // K <= 16 -> at most 48 floats = 12 quads per Gaussian
        float4 v[kMaxQ];
        bool ld[kMaxQ];
#pragma unroll
        for (int q = 0; q < kMaxQ; ++q) {
            const int e = threadIdx.x + q * kProjThreads;
            ld[q] = e < total4 && vis[e / per_row];
            if (ld[q]) v[q] = src4[e];
        }
#pragma unroll
        for (int q = 0; q < kMaxQ; ++q) {
            if (ld[q]) {
                const int e = threadIdx.x + q * kProjThreads;
                const int g = e / per_row, o = e - g * per_row;
                float* d = tile + g * stride + 4 * o;
                d[0] = v[q].x; d[1] = v[q].y; d[2] = v[q].z; d[3] = v[q].w;
            }
        }
    } else {
        for (int e = threadIdx.x; e < rows * ka3; e += blockDim.x) {
            const int g = e / ka3, o = e - g * ka3;
            if (vis[g]) tile[g * stride + o] = src[(int64_t)g * row_f + o];
        }
    }
}

// Split parameter layout of the reference model (sh_0[N,1,3] and sh_rest[N,K-1,3] are separate
// nn.Parameters, /root/reference/model/gaussian.py:49-50, concatenated on every forward at :105-107):
// staging straight from the two tensors removes that cat (and the split of its gradient).
template <int KC>
__device__ __forceinline__ void stage_sh_rows_split(const float* __restrict__ sh0, const float* __restrict__ shr,
                                                    int64_t n0, int rows, int Krt, int ka3, const int* vis, float* tile) {
    const int K = KC > 0 ? KC : Krt;
    const int row_f = 3 * K, stride = row_f + 1, rest_f = row_f - 3, kr = ka3 - 3;
    for (int e = threadIdx.x; e < rows * 3; e += blockDim.x) {
        const int g = e / 3;
        if (vis[g]) tile[g * stride + (e - 3 * g)] = sh0[n0 * 3 + e];
    }
    if (kr <= 0) return;
    const float* src = shr + n0 * rest_f;
    const int total = rows * rest_f;
    if (kr == rest_f) {  // whole rows needed: one contiguous, 16-byte aligned stream for the block
        const float4* src4 = reinterpret_cast<const float4*>(src);
        constexpr int kMaxQ = KC == 25 ? 18 : 12;   // <= 45 floats per Gaussian -> at most 12 quads per thread (72 at SH4: 18)
        const int total4 = total >> 2;
        float4 v[kMaxQ];
        bool ld[kMaxQ];
#pragma unroll
        for (int q = 0; q < kMaxQ; ++q) {   // issue every load first (see stage_sh_rows)
            const int e4 = threadIdx.x + q * kProjThreads;
            ld[q] = e4 < total4;   // culled rows are loaded too: 12 % more bytes, but a dense stream (-8 % on the kernel)
            if (ld[q]) v[q] = nt_load4(src4 + e4);
        }
#pragma unroll
        for (int q = 0; q < kMaxQ; ++q) {
            if (ld[q]) {
                const int e = (threadIdx.x + q * kProjThreads) << 2;
                const float vv[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int g = (e + i) / rest_f, o = (e + i) - g * rest_f;
                    if (vis[g]) tile[g * stride + 3 + o] = vv[i];
                }
            }
        }
        for (int e = (total & ~3) + threadIdx.x; e < total; e += blockDim.x) {
            const int g = e / rest_f, o = e - g * rest_f;
            if (vis[g]) tile[g * stride + 3 + o] = src[e];
        }
    } else {
        for (int e = threadIdx.x; e < rows * kr; e += blockDim.x) {
            const int g = e / kr, o = e - g * kr;
            if (vis[g]) tile[g * stride + 3 + o] = src[(int64_t)g * rest_f + o];
        }
    }
}

// The same staging in two halves, for the one-launch forward (STAGE 0) with the reference's full SH3 rows in the split
// layout: `sh_rows_issue` requests a block's whole slice (every thread its 12 quads of sh_rest and <= 3 floats of sh_0) at
// the top of the kernel, `sh_rows_commit` moves it into the LDS tile once the visibility flags exist -- the 192 bytes
// per Gaussian then arrive while the fp64 projection chain runs instead of after it (the block used to stream them in
// a phase of its own, between two barriers, with nothing else to do).
struct ShPrefetch {
    float4 v[12];
    float s0[3];
};

__device__ __forceinline__ void sh_rows_issue(const float* __restrict__ sh0, const float* __restrict__ shr, int64_t n0,
                                              int rows, ShPrefetch& pf) {
    constexpr int rest_f = 45;
    const float4* src4 = reinterpret_cast<const float4*>(shr + n0 * rest_f);
    const int total4 = (rows * rest_f) >> 2;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int e4 = threadIdx.x + q * kProjThreads;
        pf.v[q] = e4 < total4 ? nt_load4(src4 + e4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int e = threadIdx.x + q * kProjThreads;
        pf.s0[q] = e < rows * 3 ? sh0[n0 * 3 + e] : 0.f;
    }
}

__device__ __forceinline__ void sh_rows_commit(const ShPrefetch& pf, const float* __restrict__ shr, int64_t n0, int rows,
                                               float* tile) {
    // Every row is written, visible or not (the loads were unconditional; a test per element was an LDS read of the flag, a
    // compare and an exec-mask round trip in front of each of the 51 LDS writes).  Element e of the sh_rest stream lies in row
    // g = e / 45 at tile[49 g + 3 + (e - 45 g)] = tile[e + 4 g + 3]: one division per quad, the row stepped where a quad
    // straddles two rows.
    constexpr int rest_f = 45, stride = 49;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int e = threadIdx.x + q * kProjThreads;
        if (e < rows * 3) { const int g = e / 3; tile[g * stride + (e - 3 * g)] = pf.s0[q]; }
    }
    const int total = rows * rest_f, total4 = total >> 2;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int e4 = threadIdx.x + q * kProjThreads;
        if (e4 < total4) {
            const float vv[4] = {pf.v[q].x, pf.v[q].y, pf.v[q].z, pf.v[q].w};
            const int e = e4 << 2, g = e / rest_f, o = e - g * rest_f;
            float* d = tile + e + 4 * g + 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i + (o + i >= rest_f ? 4 : 0)] = vv[i];
        }
    }
    const float* src = shr + n0 * rest_f;
    for (int e = (total & ~3) + threadIdx.x; e < total; e += blockDim.x) {   // (the last block's 0-3 trailing floats)
        const int g = e / rest_f;
        tile[e + 4 * g + 3] = src[e];
    }
}

// STAGE 0: geometry + colour in one launch.  STAGE 1: geometry only (radii, means2d, depths,
// conics, footprint, record quads 0-1).  STAGE 2: colour only (SH evaluation -> colors_out and
// record quad 2) for the Gaussians stage 1 found visible.  The split lets the host enqueue the
// colour pass BEHIND the tile-count kernels: the one host read-back of the path (I, to size the
// lists) then overlaps ~0.1 ms of SH streaming instead of leaving the GPU idle.
template <int DEG, int STAGE>
__global__ __launch_bounds__(kProjThreads) void project_fwd_kernel(const ProjFwdArgs a) {
    constexpr int CAM = kCamPinhole;
    constexpr bool AA = false;
#include "gs_project_fwd_body.h"
}
// ... under another camera model (gs_project_fwd_cm: CAM = kCamOrtho, kCamFisheye): the same text around project_gaussian_cm<CAM>.  A kernel
// template of its own: the pinhole kernel above keeps its symbol and its code.  STAGE 2 (colour only) has no camera model in it.
template <int DEG, int STAGE, int CAM>
__global__ __launch_bounds__(kProjThreads) void project_fwd_cm_kernel(const ProjFwdArgs a) {
    static_assert(CAM != kCamPinhole && STAGE != 2, "the pinhole model and the colour stage are project_fwd_kernel's");
    constexpr bool AA = false;
#include "gs_project_fwd_body.h"
}
// ... in the antialiased mode (gs_project_fwd_aa; pinhole): the record's opacity, the extents and the tile mask take opacity * rho, and rho
// is left in a.compensations.  Again a template of its own; the colour stage has no opacity in it and stays project_fwd_kernel's.
template <int DEG, int STAGE>
__global__ __launch_bounds__(kProjThreads) void project_fwd_aa_kernel(const ProjFwdArgs a) {
    static_assert(STAGE != 2, "the colour stage is project_fwd_kernel's");
    constexpr int CAM = kCamPinhole;
    constexpr bool AA = true;
#include "gs_project_fwd_body.h"
}

// ------------------------------------------------------------------------------------------------
struct ProjBwdArgs {
    int C, cam, K, colors_per_camera, W, H, accumulate;
    int64_t N;
    float eps2d, near_p, far_p;
    const float *means, *quats, *scales, *colors_in, *sh_rest, *viewmats, *Ks, *colors_post;
    const int32_t *radii, *tiles_per_gauss, *cum_tiles;
    const float4* rows;      // [I*4][3]: one row per (intersection slot, tile quadrant)
    const int32_t* row_base; // [I/16+1]: gradient rows in front of every 16th slot (gs_blend_fwd's scan of the quadrant masks)
    const uint8_t* qmask;    // [I] by slot: which of the four quadrant rows exist (the readers' share of the scan: rows_before)
    const float4* sh_jac;    // optional, from gs_project_fwd ([C*N][8] + [C*N]): the SH rows are then not read at all
    float *v_means, *v_quats, *v_scales, *v_opacities, *v_colors, *v_sh_rest, *v_means2d_abs, *v_means2d,
        *v_conics, *v_colors_post, *v_colors_pre;
    const float* opacities;   // raw (logit) opacities, read only when activations != 0
    int activations;
    const int64_t* guard;     // step guard (gs_guard_set) or nullptr
    // Fused Adam (gs_project_bwd_adam): when `adam` is set no gradient is written; every parameter element is updated
    // in place right where its gradient is formed.  Tensor order of the reference's param_names:
    // 0 means, 1 log_scales, 2 quats, 3 sh_0, 4 sh_rest, 5 logit_opacities.
    int adam;
    // (three bases + six offsets instead of eighteen pointers: the fused kernel is SGPR-bound -- 106 live -- and every pointer it
    //  keeps across the row sum is two of them; adam_p / adam_m / adam_v below)
    float *ad_pbase, *ad_mbase, *ad_vbase;
    int64_t ad_off[6];
    const float* ad_hyper;    // {1/sqrt(1-beta2^t), lr_k/(1-beta1^t) x 6}  (gs_adam_hyper)
    float ad_b1, ad_b2, ad_eps;
    int64_t* ad_applied;
    // ... and update_statistics (/root/reference/model/gaussian.py:188-197) for the single camera, from the radius and
    // the absgrad this thread holds anyway (optional: NULL = not fused)
    float *st_max_radii, *st_grad_norm, *st_counts;
    float st_max_hw;
    // View-parallel step (distributed.ViewParallelStep): the row sums come from gs_row_sums (formed early, for the colour
    // exchange), and this view's two additive statistics are WRITTEN (not accumulated) into the all-reduce bucket:
    // |absgrad|_2 * max_hw and the visibility flag, 0 for culled Gaussians (st_max_hw as above)
    const float* row_sums;            // optional [C*N][12]
    float *st_gn_out, *st_cnt_out;    // optional [N] each (single camera)
    const int64_t* rblk;              // depth rounds (gs_rounds_set phase 3): the rows are two ranges, split at slot rblk[GS_ROUND_BASE]
    // Scale-ratio regulariser (gs_project_bwd_adam_reg; REG & 1 only): the free ratio R and the upstream
    // gradient of one term, lambda * (1 / N) -- its gradient joins v_scale of every in-range Gaussian in front of the Adam update
    float reg_ratio, reg_grad;
    // Budget regulariser (gs_project_bwd_adam_mcmc; REG & 2 only): fl32(a / N) and fl32(b / (3 N)), the upstream gradients of one
    // opacity and of one scale -- its gradients join v_opacity and v_scale the same way (gs_common.h budget_reg_term)
    float bud_ga, bud_gb;
    // Depth supervision (gs_project_bwd_adam_depth; REG & 4 only): v_z per Gaussian from gs_depth_grads_z -- v_z times row 2 of the view
    // matrix joins v_mean behind the projection's VJP, as gs_depth_grads adds it to the gradient gs_project_bwd wrote
    const float* v_depths;
    // Antialiased mode (project_bwd_aa_kernel only): optional [C*N], the row sum's gradient of the record's opacity as it is -- what
    // the camera-gradient kernel needs per (camera, Gaussian) to form v_rho (gs_project_bwd_cam_aa)
    float* v_op_rec;
};

__device__ __forceinline__ float* adam_p(const ProjBwdArgs& a, int t) { return a.ad_pbase + a.ad_off[t]; }
__device__ __forceinline__ float* adam_m(const ProjBwdArgs& a, int t) { return a.ad_mbase + a.ad_off[t]; }
__device__ __forceinline__ float* adam_v(const ProjBwdArgs& a, int t) { return a.ad_vbase + a.ad_off[t]; }
__device__ __forceinline__ float sh_adam_isbc2(const ProjBwdArgs& a) { return a.ad_hyper[0]; }
__device__ __forceinline__ float sh_adam_ss(const ProjBwdArgs& a, int t) { return a.ad_hyper[1 + t]; }

struct RowSum {
    float v[12];
};
constexpr int kRow4 = GS_ROW_FLOATS / 4;   // float4 per gradient row (include/gs_raster.h)

// Dense, coalesced write-out of one block's SH-gradient tile (LDS rows of 3K floats, row stride
// 3K+1) to v_shs[n0 : n0+rows]: unsplit [N,K,3] or split v_sh_0[N,1,3] + v_sh_rest[N,K-1,3].
template <int KC>   // KC > 0: K at compile time (divisions by 45 / 48 / 12 as multiply-shifts), see stage_sh_rows
__device__ __forceinline__ void write_sh_tile_k(const float* tile, int rows, int Krt, int64_t n0, float* v_colors,
                                                float* v_sh_rest, bool accumulate) {
    const int K = KC > 0 ? KC : Krt;
    const int row_f = 3 * K, stride = row_f + 1;
        if (v_sh_rest) {  // split layout: v_sh_0[N,1,3] and v_sh_rest[N,K-1,3]
            const int rest_f = row_f - 3, total = rows * rest_f;
            float* d0 = v_colors + n0 * 3;
            for (int e = threadIdx.x; e < rows * 3; e += blockDim.x) {
                const int g = e / 3;
                float v = tile[g * stride + (e - 3 * g)];
                if (accumulate) v += d0[e];
                d0[e] = v;
            }
            float* dr = v_sh_rest + n0 * rest_f;
            float4* dr4 = reinterpret_cast<float4*>(dr);
            for (int e4 = threadIdx.x; e4 < (total >> 2); e4 += blockDim.x) {
                float vv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = (e4 << 2) + i, g = e / rest_f;
                    vv[i] = tile[g * stride + 3 + (e - g * rest_f)];
                }
                float4 v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                if (accumulate) { const float4 o = dr4[e4]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                nt_store4(v, dr4 + e4);
            }
            for (int e = (total & ~3) + threadIdx.x; e < total; e += blockDim.x) {
                const int g = e / rest_f;
                float v = tile[g * stride + 3 + (e - g * rest_f)];
                if (accumulate) v += dr[e];
                dr[e] = v;
            }
        } else {
        float* dst = v_colors + n0 * row_f;
        if ((row_f & 3) == 0) {
            const int per_row = row_f >> 2;
            float4* dst4 = reinterpret_cast<float4*>(dst);
            for (int e = threadIdx.x; e < rows * per_row; e += blockDim.x) {
                const int g = e / per_row, q = e - g * per_row;
                const float* sp = tile + g * stride + 4 * q;
                float4 v = make_float4(sp[0], sp[1], sp[2], sp[3]);
                if (accumulate) { const float4 o = dst4[e]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                dst4[e] = v;
            }
        } else {
            for (int e = threadIdx.x; e < rows * row_f; e += blockDim.x) {
                const int g = e / row_f, o = e - g * row_f;
                float v = tile[g * stride + o];
                if (accumulate) v += dst[e];
                dst[e] = v;
            }
        }
        }
}

__device__ __forceinline__ void write_sh_tile(const float* tile, int rows, int K, int64_t n0, float* v_colors,
                                              float* v_sh_rest, bool accumulate) {
    if (K == 16) write_sh_tile_k<16>(tile, rows, 16, n0, v_colors, v_sh_rest, accumulate);
    else write_sh_tile_k<0>(tile, rows, K, n0, v_colors, v_sh_rest, accumulate);
}

#define GS_ADAM_BATCH 3
// The same walk over one block's SH-gradient tile, but as an in-place Adam update of sh_0 / sh_rest (split layout)
// and their moments: the 48 SH gradients per Gaussian (81 % of all gradient bytes at SH3) are never written to HBM
// nor read back by a separate optimizer pass.  (The block staged its own SH rows into LDS before the barrier in
// front of this call, and no other block touches them, so updating in place is race-free.)
// KC > 0 fixes K at compile time (K = 16: the reference's SH3 layout): the per-element Gaussian / offset divisions by 45
// become multiply-shifts (four run-time integer divisions per 16 bytes otherwise).
// (templated on the argument block: project_bwd_kernel reads the bias corrections from the device array gs_adam_hyper wrote,
//  sh_grad_views_kernel<.., ADAM> carries them as kernel arguments; both expose ad_p / ad_m / ad_v [3], [4] and the betas)
struct ProjBwdArgs;
__device__ __forceinline__ float* adam_p(const ProjBwdArgs& a, int t);
__device__ __forceinline__ float* adam_m(const ProjBwdArgs& a, int t);
__device__ __forceinline__ float* adam_v(const ProjBwdArgs& a, int t);
__device__ __forceinline__ float sh_adam_isbc2(const ProjBwdArgs& a);
__device__ __forceinline__ float sh_adam_ss(const ProjBwdArgs& a, int t);
// SEL (project_bwd_selective_kernel): vis_s[g] says whether Gaussian g of the block was seen -- a culled one keeps its bits, a 16-byte
// group none of whose (at most two: rest_f >= 9) Gaussians was seen is neither loaded nor stored, a mixed one selects per element.
__device__ __forceinline__ void adam1_sel(bool on, float& p, float g, float& m, float& v, float b1, float b2, float eps, float isbc2, float ss) {
    float pn = p, mn = m, vn = v;
    adam1(pn, g, mn, vn, b1, b2, eps, isbc2, ss);
    p = on ? pn : p; m = on ? mn : m; v = on ? vn : v;
}
template <int KC, bool SEL = false, class A>
__device__ __forceinline__ void adam_sh_tile(const float* tile, int rows, int Krt, int64_t n0, const A& a, const int* vis_s = nullptr) {
    const int K = KC > 0 ? KC : Krt;
    const int row_f = 3 * K, stride = row_f + 1;
    const float isbc2 = sh_adam_isbc2(a), ss0 = sh_adam_ss(a, 3), ssr = sh_adam_ss(a, 4);
    {
        float *p0 = adam_p(a, 3) + n0 * 3, *m0 = adam_m(a, 3) + n0 * 3, *v0 = adam_v(a, 3) + n0 * 3;
        for (int e = threadIdx.x; e < rows * 3; e += blockDim.x) {
            const int g = e / 3;
            if (SEL && !vis_s[g]) continue;
            float p = p0[e], m = m0[e], v = v0[e];
            adam1(p, tile[g * stride + (e - 3 * g)], m, v, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss0);
            p0[e] = p; m0[e] = m; v0[e] = v;
        }
    }
    if (K > 1) {
        const int rest_f = row_f - 3, total = rows * rest_f;
        float *pr = adam_p(a, 4) + n0 * rest_f, *mr = adam_m(a, 4) + n0 * rest_f, *vr = adam_v(a, 4) + n0 * rest_f;
        // (n0 is a multiple of the block size and rest_f * kProjThreads of 4: the block's slice starts 16-byte aligned
        //  whenever the tensor does)
        const bool aligned = ((((uintptr_t)pr | (uintptr_t)mr | (uintptr_t)vr) & 15) == 0);
        const int vec_end = aligned ? (total & ~3) : 0;
        float4 *pr4 = reinterpret_cast<float4*>(pr), *mr4 = reinterpret_cast<float4*>(mr), *vr4 = reinterpret_cast<float4*>(vr);
        // kAdamBatch iterations' worth of parameters and moments are requested before the first update is stored: the
        // in-place stores may alias the next loads as far as the compiler can tell, and a thread would otherwise pay one
        // HBM round trip per 16 bytes x 3
        constexpr int kAdamBatch = GS_ADAM_BATCH;
        const int n4 = vec_end >> 2;
        for (int e0 = threadIdx.x; e0 < n4; e0 += kAdamBatch * (int)blockDim.x) {
            float4 p[kAdamBatch], m[kAdamBatch], v[kAdamBatch];
            bool seen[kAdamBatch];   // (SEL) somebody saw one of the group's Gaussians
#pragma unroll
            for (int u = 0; u < kAdamBatch; ++u) {
                const int e4 = e0 + u * (int)blockDim.x;
                seen[u] = e4 < n4;
                if (SEL && seen[u]) seen[u] = (vis_s[(e4 << 2) / rest_f] | vis_s[((e4 << 2) + 3) / rest_f]) != 0;
                if (seen[u]) { p[u] = pr4[e4]; m[u] = nt_load4(mr4 + e4); v[u] = nt_load4(vr4 + e4); }
            }
#pragma unroll
            for (int u = 0; u < kAdamBatch; ++u) {
                const int e4 = e0 + u * (int)blockDim.x;
                if (seen[u]) {
                    float gg[4];
                    bool on[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = (e4 << 2) + i, g = e / rest_f;
                        gg[i] = tile[g * stride + 3 + (e - g * rest_f)];
                        on[i] = !SEL || vis_s[g] != 0;
                    }
                    if (SEL) {
                        adam1_sel(on[0], p[u].x, gg[0], m[u].x, v[u].x, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                        adam1_sel(on[1], p[u].y, gg[1], m[u].y, v[u].y, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                        adam1_sel(on[2], p[u].z, gg[2], m[u].z, v[u].z, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                        adam1_sel(on[3], p[u].w, gg[3], m[u].w, v[u].w, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                    } else {
                        adam1(p[u].x, gg[0], m[u].x, v[u].x, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                        adam1(p[u].y, gg[1], m[u].y, v[u].y, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                        adam1(p[u].z, gg[2], m[u].z, v[u].z, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                        adam1(p[u].w, gg[3], m[u].w, v[u].w, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
                    }
                    pr4[e4] = p[u]; nt_store4(m[u], mr4 + e4); nt_store4(v[u], vr4 + e4);
                }
            }
        }
        for (int e = vec_end + threadIdx.x; e < total; e += blockDim.x) {
            const int g = e / rest_f;
            if (SEL && !vis_s[g]) continue;
            float p = pr[e], m = mr[e], v = vr[e];
            adam1(p, tile[g * stride + 3 + (e - g * rest_f)], m, v, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ssr);
            pr[e] = p; mr[e] = m; vr[e] = v;
        }
    }
}

// In-place Adam of one block's slice of the four geometry tensors (groups 0 means[N,3], 1 log_scales[N,3], 2 quats[N,4],
// 5 logit_opacities[N]) from gradients staged in LDS in element order: tile + {0, 3, 6, 10} * kProjThreads.
// SEL: as in adam_sh_tile -- vis_s[g] selects per element (the Gaussian of element e of a tensor: e / width), a group nobody saw is skipped.
template <bool SEL = false>
__device__ __forceinline__ void adam_geo_tile(const float* tile, int rows, int64_t n0, const ProjBwdArgs& a, const int* vis_s = nullptr) {
    constexpr int kSeg = 4;
    const int group[kSeg] = {0, 1, 2, 5}, width[kSeg] = {3, 3, 4, 1}, goff[kSeg] = {0, 3 * kProjThreads, 6 * kProjThreads, 10 * kProjThreads};
    const float isbc2 = a.ad_hyper[0];
    float4 p[kSeg], m[kSeg], v[kSeg];
    bool has[kSeg];
    const int e4 = threadIdx.x;   // (a block's slice of a tensor holds at most kProjThreads 16-byte groups: 4 floats per Gaussian)
#pragma unroll
    for (int sgi = 0; sgi < kSeg; ++sgi) {   // every load first
        const int t = group[sgi], total = rows * width[sgi];
        float *pp = adam_p(a, t) + n0 * width[sgi], *mm = adam_m(a, t) + n0 * width[sgi], *vv = adam_v(a, t) + n0 * width[sgi];
        const bool aligned = ((((uintptr_t)pp | (uintptr_t)mm | (uintptr_t)vv) & 15) == 0);
        has[sgi] = aligned && e4 < (total >> 2);
        if (SEL && has[sgi]) {   // (two Gaussians at most for the widths 3 and 4, four for the opacities)
            has[sgi] = width[sgi] == 1 ? (vis_s[4 * e4] | vis_s[4 * e4 + 1] | vis_s[4 * e4 + 2] | vis_s[4 * e4 + 3]) != 0
                                       : (vis_s[(4 * e4) / width[sgi]] | vis_s[(4 * e4 + 3) / width[sgi]]) != 0;
        }
        if (has[sgi]) {
            p[sgi] = reinterpret_cast<const float4*>(pp)[e4];
            m[sgi] = nt_load4(reinterpret_cast<const float4*>(mm) + e4);
            v[sgi] = nt_load4(reinterpret_cast<const float4*>(vv) + e4);
        }
    }
#pragma unroll
    for (int sgi = 0; sgi < kSeg; ++sgi) {
        const int t = group[sgi], total = rows * width[sgi];
        float *pp = adam_p(a, t) + n0 * width[sgi], *mm = adam_m(a, t) + n0 * width[sgi], *vv = adam_v(a, t) + n0 * width[sgi];
        const float ss = a.ad_hyper[1 + t];
        const float* g = tile + goff[sgi];
        if (has[sgi]) {
            const float4 g4 = *reinterpret_cast<const float4*>(g + 4 * e4);
            if (SEL) {
                const int w = width[sgi];
                adam1_sel(vis_s[(4 * e4) / w] != 0, p[sgi].x, g4.x, m[sgi].x, v[sgi].x, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
                adam1_sel(vis_s[(4 * e4 + 1) / w] != 0, p[sgi].y, g4.y, m[sgi].y, v[sgi].y, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
                adam1_sel(vis_s[(4 * e4 + 2) / w] != 0, p[sgi].z, g4.z, m[sgi].z, v[sgi].z, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
                adam1_sel(vis_s[(4 * e4 + 3) / w] != 0, p[sgi].w, g4.w, m[sgi].w, v[sgi].w, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
            } else {
                adam1(p[sgi].x, g4.x, m[sgi].x, v[sgi].x, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
                adam1(p[sgi].y, g4.y, m[sgi].y, v[sgi].y, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
                adam1(p[sgi].z, g4.z, m[sgi].z, v[sgi].z, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
                adam1(p[sgi].w, g4.w, m[sgi].w, v[sgi].w, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
            }
            reinterpret_cast<float4*>(pp)[e4] = p[sgi];
            nt_store4(m[sgi], reinterpret_cast<float4*>(mm) + e4);
            nt_store4(v[sgi], reinterpret_cast<float4*>(vv) + e4);
        }
        // what the 16-byte groups do not cover: the whole slice when a tensor is not 16-byte aligned, else its last 0-3 floats
        const bool aligned = ((((uintptr_t)pp | (uintptr_t)mm | (uintptr_t)vv) & 15) == 0);
        for (int e = (aligned ? (total & ~3) : 0) + (int)threadIdx.x; e < total; e += blockDim.x) {
            if (SEL && !vis_s[e / width[sgi]]) continue;
            float ps = pp[e], ms = mm[e], vs = vv[e];
            adam1(ps, g[e], ms, vs, a.ad_b1, a.ad_b2, a.ad_eps, isbc2, ss);
            pp[e] = ps; mm[e] = ms; vv[e] = vs;
        }
    }
}


// ---- gradient rows of the wave's Gaussians -------------------------------------------------------------------------
// blend_bwd leaves one 48-byte row per (intersection, quadrant) some pixel took, COMPACT and in slot order (round 6:
// row_base = gs_blend_fwd's scan of the quadrant masks): the rows of a Gaussian are contiguous, the Gaussians of a wave follow
// one another with nothing in between -- the wave's rows are ONE contiguous range [R0, R0 + T), read 64 rows at a time (an
// ITEM), a row per lane, 3 KB of fully used cache lines per item and the next item in flight while this one is added.
// (Rounds 3-5 kept a row per LISTED (intersection, quadrant): 192 bytes per list entry, found through a mask byte per entry;
// a lane gathered up to four predicated rows, an owner lookup through LDS told it whose they were, and on realistic
// footprints -- where 1-3 % of the listed entries are walked -- the pass read masks of rows that did not exist.)
// Each lane leaves its row in LDS; every Gaussian adds the rows of its own range [lo, hi) of the item in row order.  An item
// that lies inside ONE Gaussian's range is not staged at all: the lanes keep partial sums in registers across such items and
// one DPP reduction closes the run (a splat over the whole image holds 10^5 rows).  Fixed order -> reproducible sums, and the
// same bits from project_bwd_kernel and row_sums_kernel.
constexpr int kRowWaveFloats = 64 * 12;   // LDS of one wave: an item's 64 rows

// Depth rounds (a.rblk: gs_rounds_set phase 3): the wave's rows are TWO such ranges -- the slots of the front round's Gaussians lie
// in front of slot GS_ROUND_BASE, those of the back round's behind it, and the Gaussians of one round follow one another inside
// their range.  The walk below runs over the two ranges laid end to end: row j of the wave is row R0 + j of the front range for
// j < Ta and row R0b + (j - Ta) of the back range behind (an item may straddle the seam: every lane forms its own address).
template <class A>
__device__ __forceinline__ void row_sum_wave(const A& a, int nr, int r0, int base, RowSum& s, float* wl) {
    const int lane = lane_id();
#pragma unroll
    for (int i = 0; i < 12; ++i) s.v[i] = 0.f;
    const bool two = a.rblk != nullptr;   // (kernel argument: uniform)
    const bool back = two && (int64_t)base >= a.rblk[GS_ROUND_BASE];
    const int incl = wave_incl_scan_add(back ? 0 : nr);
    int o = incl - nr;
    const int Ta = __builtin_amdgcn_readlane(incl, 63);
    int T = Ta;
    int64_t R0b = 0;
    if (two) {
        const int inb = wave_incl_scan_add(back ? nr : 0);
        if (back) o = Ta + inb - nr;
        T += __builtin_amdgcn_readlane(inb, 63);
        const unsigned long long bb = __ballot(back && nr > 0);
        if (bb) R0b = __shfl(r0, __builtin_ctzll(bb), 64);
    }
    if (T == 0) return;   // wave-uniform
    const unsigned long long fb = __ballot(!back && nr > 0);
    const int64_t R0 = fb ? __shfl(r0, __builtin_ctzll(fb), 64) : 0;
    float4* item = reinterpret_cast<float4*>(wl);
    const int n_items = (T + 63) >> 6;
    // (the third quad of a row holds three live floats: loaded as 12 bytes)
    struct Row { float4 a, b; float cx, cy, cz; };
    auto fetch = [&](Row& d, int it) {
        const int j = 64 * it + lane;
        d.a = d.b = make_float4(0.f, 0.f, 0.f, 0.f); d.cx = d.cy = d.cz = 0.f;
        if (j < T) {
            const float4* rp = a.rows + kRow4 * (j < Ta ? R0 + j : R0b + (j - Ta));
            d.a = rp[0]; d.b = rp[1];
            const float* c = reinterpret_cast<const float*>(rp + 2);
            d.cx = c[0]; d.cy = c[1]; d.cz = c[2];
        }
    };
    auto add = [](RowSum& p, const Row& d) {
        p.v[0] += d.a.x; p.v[1] += d.a.y; p.v[2] += d.a.z; p.v[3] += d.a.w;
        p.v[4] += d.b.x; p.v[5] += d.b.y; p.v[6] += d.b.z; p.v[7] += d.b.w;
        p.v[8] += d.cx; p.v[9] += d.cy; p.v[10] += d.cz;
    };
    // the wave-wide sums of `p` go to lane `owner`
    auto close = [&](RowSum& p, int owner) {
#pragma unroll
        for (int i = 0; i < 11; ++i) {
            const float t = wave_reduce_add_dpp(p.v[i]);
            if (lane == owner) s.v[i] += t;
        }
    };
    Row cur, nxt;
    fetch(cur, 0);
    int it = 0;
    while (it < n_items) {
        if (it + 1 < n_items) fetch(nxt, it + 1);
        const int jb = 64 * it;
        const int lo = max(o, jb) - jb, hi = min(o + nr, jb + 64) - jb;   // this Gaussian's rows inside the item
        const unsigned long long whole = __ballot(nr > 0 && lo == 0 && hi == 64);
        if (whole) {   // wave-uniform: the item lies inside ONE Gaussian's range -- and so do the items up to `last`
            const int owner = __builtin_ctzll(whole);
            const int last = (__shfl(o + nr, owner, 64) >> 6) - 1;   // the last item that is all this Gaussian's
            RowSum p;
#pragma unroll
            for (int i = 0; i < 12; ++i) p.v[i] = 0.f;
            add(p, cur);
            int k = it + 1;
            if (k <= last) { add(p, nxt); ++k; }
            // four items in flight at a time: a wave that holds a splat over the whole image walks 10^4 .. 10^5 rows on its own, and
            // one item per round trip made it the kernel's tail (round 6: 0.29 ms on the heavy-tailed 1 M scene, 0.21 before)
            for (; k + 3 <= last; k += 4) {
                Row b0, b1, b2, b3;
                fetch(b0, k); fetch(b1, k + 1); fetch(b2, k + 2); fetch(b3, k + 3);
                add(p, b0); add(p, b1); add(p, b2); add(p, b3);
            }
            for (; k <= last; ++k) { Row b0; fetch(b0, k); add(p, b0); }
            close(p, owner);
            it = last + 1;
            if (it < n_items) fetch(cur, it);   // (when the run was one item long this is `nxt` again: rare, and cached)
            continue;
        }
        // segments of 16 rows and more: one masked wave reduction each (an owner that adds its rows one by one holds the other
        // 63 lanes for as many LDS round trips); the shorter ones: every owner walks its own rows in LDS
        unsigned long long longs = __ballot(nr > 0 && hi - lo >= 16);
        for (; longs; longs &= longs - 1ull) {
            const int owner = __builtin_ctzll(longs);
            const int slo = __shfl(lo, owner, 64), shi = __shfl(hi, owner, 64);
            const bool in = lane >= slo && lane < shi;
            RowSum p;
            p.v[0] = in ? cur.a.x : 0.f; p.v[1] = in ? cur.a.y : 0.f; p.v[2] = in ? cur.a.z : 0.f; p.v[3] = in ? cur.a.w : 0.f;
            p.v[4] = in ? cur.b.x : 0.f; p.v[5] = in ? cur.b.y : 0.f; p.v[6] = in ? cur.b.z : 0.f; p.v[7] = in ? cur.b.w : 0.f;
            p.v[8] = in ? cur.cx : 0.f; p.v[9] = in ? cur.cy : 0.f; p.v[10] = in ? cur.cz : 0.f;
            close(p, owner);
        }
        if (__any(nr > 0 && hi > lo && hi - lo < 16)) {   // wave-uniform
            item[3 * lane] = cur.a; item[3 * lane + 1] = cur.b; item[3 * lane + 2] = make_float4(cur.cx, cur.cy, cur.cz, 0.f);
            __builtin_amdgcn_wave_barrier();   // (LDS operations of one wave complete in issue order)
            if (hi - lo < 16) {
                for (int r = lo; r < hi; ++r) {
                    const float4 ix = item[3 * r], iy = item[3 * r + 1], iz = item[3 * r + 2];
                    s.v[0] += ix.x; s.v[1] += ix.y; s.v[2] += ix.z; s.v[3] += ix.w;
                    s.v[4] += iy.x; s.v[5] += iy.y; s.v[6] += iy.z; s.v[7] += iy.w;
                    s.v[8] += iz.x; s.v[9] += iz.y; s.v[10] += iz.z;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        cur = nxt;
        ++it;
    }
}

// SUMS: the row sums come from gs_row_sums (a.row_sums) -- an instantiation of its own, so that the row-walking form keeps the
// registers it had (a run-time branch cost it its third wave per SIMD and put the fused form into scratch).
// REG (with ADAM only), a bit mask: 1 -- the scale-ratio regulariser's gradient is added to v_scale; 2 -- the budget regulariser's
// to v_scale and v_opacity (behind the scale-ratio term when both are on) -- likewise instantiations of their own:
// project_bwd_kernel<.., SCALE_REG = true> is mask 1, project_bwd_budget_kernel<DEG, REG> masks 2 and 3.  The two kernel templates
// share their text (gs_project_bwd_body.h) and not a device function: behind a call, inlined or not, the compiler allocated the
// SH4 instantiation of the existing form 68 bytes of scratch.
template <int DEG, bool ADAM, bool SUMS = false, bool SCALE_REG = false>
__global__ __launch_bounds__(kProjThreads) void project_bwd_kernel(const ProjBwdArgs a) {
    constexpr int REG = SCALE_REG ? 1 : 0, CAM = kCamPinhole;
    constexpr bool AA = false, SELECT = false;
#include "gs_project_bwd_body.h"
}
// the fused form under a Gaussian budget (gs_project_bwd_adam_mcmc): REG = 2 the budget term alone, 3 behind the scale-ratio term
template <int DEG, int REG, bool SUMS = false>
__global__ __launch_bounds__(kProjThreads) void project_bwd_budget_kernel(const ProjBwdArgs a) {
    constexpr bool ADAM = true, AA = false, SELECT = false;
    constexpr int CAM = kCamPinhole;
#include "gs_project_bwd_body.h"
}

// the fused form with a depth gradient (gs_project_bwd_adam_depth): REG = 4 | the two regularisers' bits
template <int DEG, int REG>
__global__ __launch_bounds__(kProjThreads) void project_bwd_depth_kernel(const ProjBwdArgs a) {
    constexpr bool ADAM = true, SUMS = false, AA = false, SELECT = false;
    constexpr int CAM = kCamPinhole;
#include "gs_project_bwd_body.h"
}

// the eager (ADAM = false) and the fused (ADAM = true; REG = 0, or 1: the scale-ratio regulariser) form under another camera model
// (gs_project_bwd_cm, gs_project_bwd_adam_cm, gs_project_bwd_adam_reg_cm): the gradient rows are walked (no SUMS form), and the budget
// and depth variants of the fused form do not exist for these models
template <int DEG, bool ADAM, int REG, int CAM>
__global__ __launch_bounds__(kProjThreads) void project_bwd_cm_kernel(const ProjBwdArgs a) {
    static_assert(CAM != kCamPinhole && (REG == 0 || (ADAM && REG == 1)), "pinhole: project_bwd_kernel; REG: the scale-ratio term, fused form only");
    constexpr bool SUMS = false, AA = false, SELECT = false;
#include "gs_project_bwd_body.h"
}

// the eager and the fused form (REG = 0, or 1: the scale-ratio regulariser) in the antialiased mode (gs_project_bwd_aa, gs_project_bwd_adam_aa,
// gs_project_bwd_adam_reg_aa; pinhole): the opacity's gradient is the record's times rho, and v_rho joins v_cov2 inside the chain's VJP.
// The gradient rows are walked (no SUMS form); the budget and depth variants of the fused form do not exist in this mode.
template <int DEG, bool ADAM, int REG>
__global__ __launch_bounds__(kProjThreads) void project_bwd_aa_kernel(const ProjBwdArgs a) {
    static_assert(REG == 0 || (ADAM && REG == 1), "REG: the scale-ratio term, fused form only");
    constexpr bool SUMS = false, AA = true, SELECT = false;
    constexpr int CAM = kCamPinhole;
#include "gs_project_bwd_body.h"
}

// the fused form over the Gaussians the step saw (gs_project_bwd_selective; REG = 0, or 1: the scale-ratio regulariser; pinhole, classic
// mode, gradient rows): a culled Gaussian keeps the bits of its parameters and moments, 16-byte groups nobody saw are neither loaded
// nor stored, and a block without a visible Gaussian leaves behind the row sum (DESIGN.md "Updating only what a step saw")
template <int DEG, int REG>
__global__ __launch_bounds__(kProjThreads) void project_bwd_selective_kernel(const ProjBwdArgs a) {
    static_assert(REG == 0 || REG == 1, "REG: the scale-ratio term");
    constexpr bool ADAM = true, SUMS = false, AA = false, SELECT = true;
    constexpr int CAM = kCamPinhole;
#include "gs_project_bwd_body.h"
}

static size_t proj_lds_bytes(int K, int degree);
// backward: the tile region also holds the four waves' row-sum scratch (row_sum_slots), with or without SH
static size_t proj_bwd_lds_bytes(int K, int degree) {
    const size_t need = sizeof(float) * (32 + kProjThreads + (size_t)(kProjThreads / 64) * kRowWaveFloats);
    const size_t base = proj_lds_bytes(K, degree);
    return base > need ? base : need;
}

static size_t proj_lds_bytes(int K, int degree) {
    // (the SH tile also stages the 11 geometry gradients per Gaussian of the fused Adam: at least 11 floats per thread)
    const size_t tile = (size_t)kProjThreads * (size_t)((3 * K + 1) > 11 ? (3 * K + 1) : 11);
    return sizeof(float) * (32 + kProjThreads + (degree >= 0 ? tile : 0));
}


// ------------------------------------------------------------------------------------------------
// SH-parameter gradients of R views from the per-view pre-clamp colour gradients:
//   v_sh[n][k][:] = sum_r Y_k(dir(mean_n, camera_r)) * v_colors_pre[r][n][:]      (views in order r = 0..R-1)
// The view-parallel step exchanges v_colors_pre (3 floats per Gaussian and view) instead of the 48
// SH gradients per Gaussian; every rank then rebuilds the identical dense SH gradient with this
// kernel (distributed.py).  Same write-out as project_bwd_kernel.
struct ShGradArgs {
    int R, K;
    int64_t N;
    const float *means, *viewmats, *v_colors_pre;
    int64_t view_stride;   // floats between view r and view r+1 of v_colors_pre (3N for a dense [R,N,3]; the payload stride of
    int64_t cam_stride;    // gs_sh_adam_views) and of viewmats (16 for a dense [R,4,4])
    float *v_colors, *v_sh_rest;
    // gs_sh_adam_views: no gradient is written -- sh_0 / sh_rest and their moments are updated in place (ShAdam), gradients
    // scaled by grad_scale first (1/world), and max_radii[n] = max(max_radii[n], max_r radii_norm[r][n])
    float *ad_p[6], *ad_m[6], *ad_v[6];                       // (only [3] = sh_0 and [4] = sh_rest are set: param_names order)
    float ad_b1, ad_b2, ad_eps, ad_isbc2, ad_ss0, ad_ssr;     // betas, eps, 1/sqrt(1-beta2^t), lr/(1-beta1^t) of the two groups
    float grad_scale;
    const float* radii_norm;   // optional: view r's normalised radii at radii_norm + r * view_stride
    float* max_radii;
    const int64_t* guard;
};

__device__ __forceinline__ float* adam_p(const ShGradArgs& a, int t) { return a.ad_p[t]; }
__device__ __forceinline__ float* adam_m(const ShGradArgs& a, int t) { return a.ad_m[t]; }
__device__ __forceinline__ float* adam_v(const ShGradArgs& a, int t) { return a.ad_v[t]; }
__device__ __forceinline__ float sh_adam_isbc2(const ShGradArgs& a) { return a.ad_isbc2; }
__device__ __forceinline__ float sh_adam_ss(const ShGradArgs& a, int t) { return t == 3 ? a.ad_ss0 : a.ad_ssr; }

constexpr int kMaxViews = 64;

template <int DEG, bool ADAM>
__global__ __launch_bounds__(kProjThreads) void sh_grad_views_kernel(const ShGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (ADAM && guard_tripped(a.guard)) return;
    float* cam_pos = smem;                       // [kMaxViews * 3]
    float* tile = smem + kMaxViews * 3;          // [kProjThreads * (3K + 1)]
    const int64_t n0 = (int64_t)blockIdx.x * kProjThreads, n = n0 + threadIdx.x;
    if ((int)threadIdx.x < a.R) {
        Camera tmp;
        const float kid[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        make_camera(a.viewmats + a.cam_stride * threadIdx.x, kid, 1, 1, tmp);
        cam_pos[3 * threadIdx.x] = tmp.pos[0]; cam_pos[3 * threadIdx.x + 1] = tmp.pos[1]; cam_pos[3 * threadIdx.x + 2] = tmp.pos[2];
    }
    __syncthreads();
    constexpr int Ka = (DEG + 1) * (DEG + 1);
    const int row_f = 3 * a.K, stride = row_f + 1;
    float acc[3 * Ka];
#pragma unroll
    for (int i = 0; i < 3 * Ka; ++i) acc[i] = 0.f;
    if (n < a.N) {
        const float mean[3] = {a.means[3 * n], a.means[3 * n + 1], a.means[3 * n + 2]};
        float rad = 0.f;
        for (int r = 0; r < a.R; ++r) {
            const float* v = a.v_colors_pre + (int64_t)r * a.view_stride + 3 * n;
            const float vr = v[0], vg = v[1], vb = v[2];
            if (ADAM && a.radii_norm) rad = fmaxf(rad, a.radii_norm[(int64_t)r * a.view_stride + n]);
            if (vr == 0.f && vg == 0.f && vb == 0.f) continue;   // not visible in view r (x + 0 is exact)
            Camera cam;
            cam.pos[0] = cam_pos[3 * r]; cam.pos[1] = cam_pos[3 * r + 1]; cam.pos[2] = cam_pos[3 * r + 2];
            float ux, uy, uz, Y[kMaxShCoeffs];
            view_dir(mean, cam, ux, uy, uz);
            sh_basis(DEG, ux, uy, uz, Y);
#pragma unroll
            for (int k = 0; k < Ka; ++k) {
                acc[3 * k] += Y[k] * vr; acc[3 * k + 1] += Y[k] * vg; acc[3 * k + 2] += Y[k] * vb;
            }
        }
        if (ADAM && a.max_radii) a.max_radii[n] = fmaxf(a.max_radii[n], rad);
        float* my = tile + threadIdx.x * stride;
#pragma unroll
        for (int i = 0; i < 3 * Ka; ++i) my[i] = ADAM ? acc[i] * a.grad_scale : acc[i];   // (gs_adam_step scales the gradient it reads the same way)
        for (int o = 3 * Ka; o < row_f; ++o) my[o] = 0.f;
    }
    __syncthreads();
    const int rows = (int)min((int64_t)kProjThreads, a.N - n0);
    if (ADAM) {
        if (DEG == 4) adam_sh_tile<25>(tile, rows, 25, n0, a);
        else if (a.K == 16) adam_sh_tile<16>(tile, rows, 16, n0, a);
        else adam_sh_tile<0>(tile, rows, a.K, n0, a);
    } else if (DEG == 4) {
        write_sh_tile_k<25>(tile, rows, 25, n0, a.v_colors, a.v_sh_rest, false);
    } else {
        write_sh_tile(tile, rows, a.K, n0, a.v_colors, a.v_sh_rest, false);
    }
}

// ------------------------------------------------------------------------------------------------
// Row sums of every Gaussian as a kernel of its own (view-parallel step): what project_bwd_kernel's phase 1 computes, with
// the same function -> the same sums bit for bit.  Leaves row_sums[C*N][12] for gs_project_bwd(row_sums = ...) and, from
// them, everything another rank needs of this view BEFORE the long projection backward runs: the clamp-masked pre-clamp
// colour gradient v_colors_pre[f] (rounds 2-4: a second pass over the rows, gs_colors_pre_grad), optionally the
// normalised radii (radius / max_hw, 0 for culled Gaussians: the MAX statistic of update_statistics) and a copy of the view
// matrix -- the three pieces of the all-gather payload of distributed.ViewParallelStep.
struct RowSumsArgs {
    int64_t total;   // C * N
    const int32_t *radii, *tiles_per_gauss, *cum_tiles;
    const float* colors_post;
    const float4* rows;
    const int32_t* row_base;
    const uint8_t* qmask;
    float4* row_sums;
    float *v_colors_pre, *radii_norm, *cam_out;
    const float* viewmats;
    float max_hw;
    const int64_t* guard;
    const int64_t* rblk;   // depth rounds (see ProjBwdArgs)
};

__global__ __launch_bounds__(256) void row_sums_kernel(const RowSumsArgs a) {
    __shared__ __attribute__((aligned(16))) float wl_all[4][kRowWaveFloats];
    if (guard_tripped(a.guard)) return;
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = f < a.total;
    const int radius = in_range ? a.radii[f] : 0;
    const bool vis = radius > 0;
    const int cnt = vis ? a.tiles_per_gauss[f] : 0, base = vis ? a.cum_tiles[f] : 0;
    int r0 = 0, nr = 0;
    if (cnt > 0) { r0 = rows_before(a.row_base, a.qmask, base); nr = rows_before(a.row_base, a.qmask, base + cnt) - r0; }
    float rgb[3] = {0.f, 0.f, 0.f};
    if (vis) { rgb[0] = a.colors_post[3 * f]; rgb[1] = a.colors_post[3 * f + 1]; rgb[2] = a.colors_post[3 * f + 2]; }
    if (a.cam_out && blockIdx.x == 0 && threadIdx.x < 16) a.cam_out[threadIdx.x] = a.viewmats[threadIdx.x];
    RowSum s;
    row_sum_wave(a, nr, r0, base, s, wl_all[threadIdx.x >> 6]);
    if (!in_range) return;
    if (vis) {   // (culled Gaussians: gs_project_bwd does not read their sums)
        float4* rs = a.row_sums + 3 * f;
        rs[0] = make_float4(s.v[0], s.v[1], s.v[2], s.v[3]);
        rs[1] = make_float4(s.v[4], s.v[5], s.v[6], s.v[7]);
        rs[2] = make_float4(s.v[8], s.v[9], s.v[10], 0.f);
    }
    float* d = a.v_colors_pre + 3 * f;   // (project_bwd_kernel's v_colors_pre: masked where the clamp max(c + 0.5, 0) is active)
    d[0] = (vis && rgb[0] > 0.f) ? s.v[8] : 0.f; d[1] = (vis && rgb[1] > 0.f) ? s.v[9] : 0.f; d[2] = (vis && rgb[2] > 0.f) ? s.v[10] : 0.f;
    if (a.radii_norm) a.radii_norm[f] = vis ? (float)radius * (1.f / a.max_hw) : 0.f;   // (update_statistics_kernel's arithmetic)
}

// ------------------------------------------------------------------------------------------------
// Camera gradients (gs_project_bwd_cam): dL/d viewmats rows 0-2 and dL/d camera centre, per camera, from what the projection
// backward leaves per (camera, Gaussian) -- the row sums it hands out as v_means2d / v_conics / v_colors_post.  A kernel of its
// own that recomputes the projection chain (project_bwd_kernel keeps its code and its registers: see the note at its template
// parameters), 15 fp64 terms per visible Gaussian: v_A[9], v_t[3] (project_vjp_cam) and minus the SH direction term [3].
// No atomics: lanes -> wave (shuffles, fixed order) -> the block's four waves through LDS -> ONE plain store of the block's
// partial cam_partials[c][block][16]; cam_sum_kernel adds a camera's partials in a fixed order.  fp64 throughout: the sum runs
// over up to millions of signed terms that cancel to a fraction of a per cent of their absolute sum (DESIGN.md "Camera gradients").
struct ProjCamArgs {
    int K, W, H, activations;
    int64_t N;
    float eps2d, near_p, far_p;
    const float *means, *quats, *scales, *sh_from_1, *viewmats, *Ks, *colors_post;
    int64_t sh_stride;        // floats between two Gaussians' coefficient-1 rows: 3K dense, 3(K-1) in the split layout
    const int32_t* radii;
    const float4* sh_jac;     // optional (gs_project_fwd): the coefficients are then not read
    const float *v_means2d, *v_conics, *v_colors_post;
    const float4* row_sums;   // SUMS: gs_row_sums' [N][12] in their place (C = 1)
    double* cam_partials;     // [C][gridDim.x][16]
    const int64_t* guard;
    // antialiased mode (project_cam_aa_kernel only): the opacities (raw with activations) and project_bwd_aa_kernel's v_op_rec [C*N]
    const float *opacities, *v_op_rec;
};

constexpr int kCamTerms = 15;

// SUMS (gs_cam_grad_sums, the captured step with poses): the three gradients are elements of the Gaussian's row sums -- floats
// 0-1, 4-6 and 8-10, as project_bwd_kernel hands them out -- and the gradient tensors do not exist.
template <int DEG, bool SUMS = false>
__global__ __launch_bounds__(kProjThreads) void project_cam_kernel(const ProjCamArgs a) {
    constexpr int CAM = kCamPinhole;
    constexpr bool AA = false;
#include "gs_project_cam_body.h"
}
// ... under another camera model (gs_project_bwd_cam_cm): v_t = v_pc and v_A = v_pc mean^T + 2 v_covc A Sigma hold for any model once the
// VJP has formed v_pc and v_covc with the model's Jacobian (gs_math.h: project_vjp_impl)
template <int DEG, int CAM>
__global__ __launch_bounds__(kProjThreads) void project_cam_cm_kernel(const ProjCamArgs a) {
    static_assert(CAM != kCamPinhole, "the pinhole model is project_cam_kernel's");
    constexpr bool SUMS = false, AA = false;
#include "gs_project_cam_body.h"
}
// ... in the antialiased mode (gs_project_bwd_cam_aa; pinhole): the VJP with v_rho in it
template <int DEG>
__global__ __launch_bounds__(kProjThreads) void project_cam_aa_kernel(const ProjCamArgs a) {
    constexpr bool SUMS = false, AA = true;
    constexpr int CAM = kCamPinhole;
#include "gs_project_cam_body.h"
}

// One block per camera: every one of the 16 values is walked by 64 threads, each over the camera's partials at a stride of 64
// blocks (two interleaved chains per thread, so that two loads are in flight), and the 64 strided sums are added in order.
// Writes v_viewmats[c] (rows 0-2 = [v_A | v_t], row 3 = 0) and v_campos[c].
constexpr int kCamSumChains = 64;
__global__ __launch_bounds__(16 * kCamSumChains) void cam_sum_kernel(const double* __restrict__ cam_partials, int n_blocks,
                                                                     float* __restrict__ v_viewmats, float* __restrict__ v_campos,
                                                                     const int64_t* __restrict__ guard) {
    __shared__ double part[kCamSumChains][16];
    if (guard_tripped(guard)) return;
    const int c = blockIdx.x, term = threadIdx.x & 15, j = threadIdx.x >> 4;
    const double* src = cam_partials + (int64_t)c * n_blocks * 16 + term;
    double t0 = 0.0, t1 = 0.0;
    for (int b = j; b < n_blocks; b += 2 * kCamSumChains) {
        t0 += src[(int64_t)b * 16];
        if (b + kCamSumChains < n_blocks) t1 += src[(int64_t)(b + kCamSumChains) * 16];
    }
    part[j][term] = t0 + t1;
    __syncthreads();
    if (threadIdx.x < 16) {
        double sum = 0.0;
#pragma unroll 8
        for (int k = 0; k < kCamSumChains; ++k) sum += part[k][term];
        float* vv = v_viewmats + 16 * c;
        if (term < 9) vv[4 * (term / 3) + term % 3] = (float)sum;
        else if (term < 12) vv[4 * (term - 9) + 3] = (float)sum;
        else if (term < 15) v_campos[3 * c + (term - 12)] = (float)sum;
        if (term < 4) vv[12 + term] = 0.f;
    }
}

}  // namespace gs

using namespace gs;

// Above K = 20 the SH tile takes more than 64 KB of LDS (77 KB at K = 25: two blocks per CU instead of three); the kernel's
// dynamic-LDS limit is raised before its first such launch (ensure_lds: once per kernel, a no-op at or below 64 KB)
#define GS_LDS(fn) if (int rc_ = ensure_lds((const void*)fn, lds)) return rc_

static int sh_views_launch(hipStream_t st, int sh_degree, bool adam, const ShGradArgs& a) {
    dim3 grid((unsigned)((a.N + kProjThreads - 1) / kProjThreads));
    const size_t lds = sizeof(float) * (kMaxViews * 3 + (size_t)kProjThreads * (3 * a.K + 1));
#define GS_SHV(D)                                                                                           \
    if (adam) { GS_LDS((sh_grad_views_kernel<D, true>)); hipLaunchKernelGGL((sh_grad_views_kernel<D, true>), grid, dim3(kProjThreads), lds, st, a); }  \
    else { GS_LDS((sh_grad_views_kernel<D, false>)); hipLaunchKernelGGL((sh_grad_views_kernel<D, false>), grid, dim3(kProjThreads), lds, st, a); }
    switch (sh_degree) {
        case 0: GS_SHV(0); break;
        case 1: GS_SHV(1); break;
        case 2: GS_SHV(2); break;
        case 3: GS_SHV(3); break;
        default: GS_SHV(4); break;
    }
#undef GS_SHV
    GS_LAUNCH_CHECK("sh_grad_views_kernel");
    return GS_OK;
}

extern "C" int gs_sh_grad_views(void* stream, int R, int64_t N, int K, int sh_degree, const float* means,
                                const float* viewmats, const float* v_colors_pre, float* v_colors,
                                float* v_sh_rest) {
    GS_REQUIRE(R >= 1 && R <= kMaxViews, "1..64 views");
    GS_REQUIRE(N >= 0 && sh_degree >= 0 && sh_degree <= 4, "N >= 0 and sh_degree in 0..4");
    GS_REQUIRE(K >= (sh_degree + 1) * (sh_degree + 1) && K <= 25, "K must hold (sh_degree+1)^2 coefficients and be <= 25");
    if (N == 0) return GS_OK;
    GS_REQUIRE(means && viewmats && v_colors_pre && v_colors, "null pointer");
    ShGradArgs a = {};
    a.R = R; a.K = K; a.N = N; a.means = means; a.viewmats = viewmats; a.v_colors_pre = v_colors_pre;
    a.view_stride = 3 * N; a.cam_stride = 16;
    a.v_colors = v_colors; a.v_sh_rest = v_sh_rest;
    return sh_views_launch((hipStream_t)stream, sh_degree, false, a);
}

extern "C" int gs_sh_adam_views(void* stream, int R, int64_t N, int K, int sh_degree, const float* means, const float* payload,
                                int64_t payload_stride, float* sh_0, float* sh_0_exp_avg, float* sh_0_exp_avg_sq, float* sh_rest,
                                float* sh_rest_exp_avg, float* sh_rest_exp_avg_sq, float lr_sh_0, float lr_sh_rest, float beta1,
                                float beta2, float eps, int64_t step, float grad_scale, float* max_radii) {
    GS_REQUIRE(R >= 1 && R <= kMaxViews, "1..64 views");
    GS_REQUIRE(N >= 0 && sh_degree >= 0 && sh_degree <= 4, "N >= 0 and sh_degree in 0..4");
    GS_REQUIRE(K >= (sh_degree + 1) * (sh_degree + 1) && K <= 25, "K must hold (sh_degree+1)^2 coefficients and be <= 25");
    GS_REQUIRE(step >= 1, "step counts from 1");
    GS_REQUIRE(payload_stride >= 4 * N + 16, "payload_stride must hold [3N colour gradients | N radii | 16 camera floats]");
    if (N == 0) return GS_OK;
    GS_REQUIRE(means && payload && sh_0 && sh_0_exp_avg && sh_0_exp_avg_sq, "null pointer");
    GS_REQUIRE(K == 1 || (sh_rest && sh_rest_exp_avg && sh_rest_exp_avg_sq), "K > 1 needs sh_rest and its moments");
    ShGradArgs a = {};
    a.R = R; a.K = K; a.N = N; a.means = means;
    a.v_colors_pre = payload; a.radii_norm = max_radii ? payload + 3 * N : nullptr; a.viewmats = payload + 4 * N;
    a.view_stride = payload_stride; a.cam_stride = payload_stride;
    a.max_radii = max_radii; a.grad_scale = grad_scale;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    a.ad_p[3] = sh_0; a.ad_m[3] = sh_0_exp_avg; a.ad_v[3] = sh_0_exp_avg_sq;
    a.ad_p[4] = sh_rest; a.ad_m[4] = sh_rest_exp_avg; a.ad_v[4] = sh_rest_exp_avg_sq;
    a.ad_isbc2 = (float)(1.0 / sqrt(bc2));   // (adam_launch's host arithmetic, gs_adam.hip)
    a.ad_ss0 = (float)((double)lr_sh_0 / bc1); a.ad_ssr = (float)((double)lr_sh_rest / bc1);
    a.ad_b1 = beta1; a.ad_b2 = beta2; a.ad_eps = eps;
    a.guard = current_guard().info;
    return sh_views_launch((hipStream_t)stream, sh_degree, true, a);
}

extern "C" int gs_row_sums(void* stream, int C, int64_t N, const int32_t* radii, const float* colors_post,
                           const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                           float* row_sums, float* v_colors_pre, float* radii_norm, float max_hw, const float* viewmats,
                           float* cam_out) {
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    if (N == 0) return GS_OK;
    GS_REQUIRE(radii && colors_post && tiles_per_gauss && cum_tiles && rows && row_base && qmask && row_sums && v_colors_pre, "null pointer");
    GS_REQUIRE(((uintptr_t)row_sums & 15) == 0, "row_sums must be 16-byte aligned");
    GS_REQUIRE(!radii_norm || max_hw > 0.f, "radii_norm needs a positive image extent");
    GS_REQUIRE(!cam_out || (viewmats && C == 1), "cam_out: the single camera's view matrix");
    RowSumsArgs a;
    a.total = (int64_t)C * N; a.radii = radii; a.tiles_per_gauss = tiles_per_gauss; a.cum_tiles = cum_tiles;
    a.colors_post = colors_post; a.rows = reinterpret_cast<const float4*>(rows); a.row_base = row_base; a.qmask = qmask;
    a.row_sums = reinterpret_cast<float4*>(row_sums); a.v_colors_pre = v_colors_pre; a.radii_norm = radii_norm;
    a.cam_out = cam_out; a.viewmats = viewmats; a.max_hw = max_hw;
    a.guard = current_guard().info;
    a.rblk = current_rounds().phase == 3 ? current_rounds().blk : nullptr;   // (depth rounds: the rows are two ranges)
    hipLaunchKernelGGL(row_sums_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("row_sums_kernel");
    return GS_OK;
}

#define GS_REQUIRE_CAMERA(m) GS_REQUIRE((m) == GS_CAMERA_PINHOLE || (m) == GS_CAMERA_ORTHO || (m) == GS_CAMERA_FISHEYE, \
                                        "camera_model: GS_CAMERA_PINHOLE, GS_CAMERA_ORTHO or GS_CAMERA_FISHEYE")

static int project_fwd(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                       const float* quats, const float* scales, const float* opacities,
                       const float* colors_in, const float* sh_rest, int colors_per_camera,
                       const float* viewmats, const float* Ks, int width, int height,
                       float eps2d, float near_plane, float far_plane, float radius_clip,
                       int tile_culling, int stage, int activations, int32_t* radii,
                       float* means2d, float* depths, float* conics, float* colors_out, float* rec,
                       uint32_t* bbox, int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac, int camera_model,
                       bool aa = false, float* compensations = nullptr) {
    GS_REQUIRE_CAMERA(camera_model);
    GS_REQUIRE(!aa || camera_model == GS_CAMERA_PINHOLE, "the antialiased mode exists for the pinhole model only");
    GS_REQUIRE(!aa || N == 0 || compensations, "compensations must not be NULL");
    GS_REQUIRE(C >= 1 && N >= 0 && width > 0 && height > 0, "C>=1, N>=0, positive image size");
    GS_REQUIRE(sh_degree <= 4, "sh_degree must be <= 4");
    GS_REQUIRE(sh_degree < 0 || (K >= (sh_degree + 1) * (sh_degree + 1) && K <= 25), "K must hold (sh_degree+1)^2 coefficients and be <= 25");
    GS_REQUIRE((width + GS_TILE - 1) / GS_TILE < 65536 && (height + GS_TILE - 1) / GS_TILE < 65536, "tile grid must fit 16 bits per axis");
    if (N == 0) return GS_OK;
    GS_REQUIRE(means && quats && scales && opacities && colors_in && viewmats && Ks, "null input pointer");
    GS_REQUIRE(radii && means2d && depths && conics && colors_out && rec && bbox && tiles_per_gauss, "null output pointer");
    ProjFwdArgs a;
    a.C = C; a.N = N; a.K = K; a.colors_per_camera = colors_per_camera; a.W = width; a.H = height;
    a.tw = (width + GS_TILE - 1) / GS_TILE; a.th = (height + GS_TILE - 1) / GS_TILE;
    a.eps2d = eps2d; a.near_p = near_plane; a.far_p = far_plane; a.radius_clip = radius_clip;
    a.tight = tile_culling != 0; a.activations = activations != 0;
    a.means = means; a.quats = quats; a.scales = scales; a.opacities = opacities; a.colors_in = colors_in;
    a.sh_rest = sh_degree >= 0 ? sh_rest : nullptr;
    a.viewmats = viewmats; a.Ks = Ks; a.radii = radii; a.means2d = means2d; a.depths = depths;
    a.conics = conics; a.colors_out = colors_out; a.rec = reinterpret_cast<float4*>(rec);
    a.bbox = reinterpret_cast<uint4*>(bbox); a.tiles_per_gauss = tiles_per_gauss;
    a.rect_ref = reinterpret_cast<uint2*>(rect_ref);
    a.sh_jac = sh_degree >= 1 ? reinterpret_cast<float4*>(sh_jac) : nullptr;
    a.compensations = compensations;
    dim3 grid((unsigned)((N + kProjThreads - 1) / kProjThreads), (unsigned)C);
    const size_t lds = proj_lds_bytes(K, sh_degree);
    hipStream_t st = (hipStream_t)stream;
    GS_REQUIRE(stage >= 0 && stage <= 2, "stage: 0 = geometry+colour, 1 = geometry, 2 = colour");
#define GS_PF(D, S)                                                                                              \
    { if ((S) != 1) GS_LDS((project_fwd_kernel<D, S>));                                                          \
      hipLaunchKernelGGL((project_fwd_kernel<D, S>), grid, dim3(kProjThreads), (S) == 1 ? proj_lds_bytes(K, -1) : lds, st, a); }
#define GS_PF_DEG(S)                                                      \
    switch (sh_degree) {                                                  \
        case 0: GS_PF(0, S); break;                                       \
        case 1: GS_PF(1, S); break;                                       \
        case 2: GS_PF(2, S); break;                                       \
        case 3: GS_PF(3, S); break;                                       \
        case 4: GS_PF((S) == 1 ? -1 : 4, S); break;   /* (stage 1: no SH) */ \
        default: GS_PF(-1, S); break;                                     \
    }
    // another camera model: a kernel per (model, degree) for the one-launch form, one per model for the geometry stage (which evaluates no
    // colour); the colour stage has no camera model in it and stays the pinhole path's kernel
#define GS_PFC(D, S, M)                                                                                          \
    { if ((S) != 1) GS_LDS((project_fwd_cm_kernel<D, S, M>));                                                    \
      hipLaunchKernelGGL((project_fwd_cm_kernel<D, S, M>), grid, dim3(kProjThreads), (S) == 1 ? proj_lds_bytes(K, -1) : lds, st, a); }
#define GS_PFC_DEG(M)                                                     \
    if (stage == 1) GS_PFC(-1, 1, M) else switch (sh_degree) {            \
        case 0: GS_PFC(0, 0, M); break;                                   \
        case 1: GS_PFC(1, 0, M); break;                                   \
        case 2: GS_PFC(2, 0, M); break;                                   \
        case 3: GS_PFC(3, 0, M); break;                                   \
        case 4: GS_PFC(4, 0, M); break;                                   \
        default: GS_PFC(-1, 0, M); break;                                 \
    }
    // the antialiased mode: as for the camera models -- a kernel per degree for the one-launch form, one for the geometry stage, and the
    // colour stage (no opacity in it) the classic kernel
#define GS_PFA(D, S)                                                                                             \
    { if ((S) != 1) GS_LDS((project_fwd_aa_kernel<D, S>));                                                       \
      hipLaunchKernelGGL((project_fwd_aa_kernel<D, S>), grid, dim3(kProjThreads), (S) == 1 ? proj_lds_bytes(K, -1) : lds, st, a); }
    if (aa && stage != 2) {
        if (stage == 1) GS_PFA(-1, 1) else switch (sh_degree) {
            case 0: GS_PFA(0, 0); break;
            case 1: GS_PFA(1, 0); break;
            case 2: GS_PFA(2, 0); break;
            case 3: GS_PFA(3, 0); break;
            case 4: GS_PFA(4, 0); break;
            default: GS_PFA(-1, 0); break;
        }
    } else
#undef GS_PFA
    if (camera_model == GS_CAMERA_ORTHO && stage != 2) { GS_PFC_DEG(kCamOrtho) }
    else if (camera_model == GS_CAMERA_FISHEYE && stage != 2) { GS_PFC_DEG(kCamFisheye) }
    else if (stage == 0) { GS_PF_DEG(0) } else if (stage == 1) { GS_PF_DEG(1) } else { GS_PF_DEG(2) }
#undef GS_PFC_DEG
#undef GS_PFC
#undef GS_PF_DEG
#undef GS_PF
    GS_LAUNCH_CHECK("project_fwd_kernel");
    return GS_OK;
}

extern "C" int gs_project_fwd(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* opacities,
                              const float* colors_in, const float* sh_rest, int colors_per_camera,
                              const float* viewmats, const float* Ks, int width, int height,
                              float eps2d, float near_plane, float far_plane, float radius_clip,
                              int tile_culling, int stage, int activations, int32_t* radii,
                              float* means2d, float* depths, float* conics, float* colors_out, float* rec,
                              uint32_t* bbox, int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac) {
    return project_fwd(stream, C, N, K, sh_degree, means, quats, scales, opacities, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radius_clip, tile_culling, stage, activations, radii, means2d, depths,
                       conics, colors_out, rec, bbox, tiles_per_gauss, rect_ref, sh_jac, GS_CAMERA_PINHOLE);
}

// gs_project_fwd under the camera model `camera_model` (GS_CAMERA_PINHOLE: that very call)
extern "C" int gs_project_fwd_cm(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                                 const float* quats, const float* scales, const float* opacities,
                                 const float* colors_in, const float* sh_rest, int colors_per_camera,
                                 const float* viewmats, const float* Ks, int width, int height,
                                 float eps2d, float near_plane, float far_plane, float radius_clip,
                                 int tile_culling, int stage, int activations, int32_t* radii,
                                 float* means2d, float* depths, float* conics, float* colors_out, float* rec,
                                 uint32_t* bbox, int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac, int camera_model) {
    return project_fwd(stream, C, N, K, sh_degree, means, quats, scales, opacities, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radius_clip, tile_culling, stage, activations, radii, means2d, depths,
                       conics, colors_out, rec, bbox, tiles_per_gauss, rect_ref, sh_jac, camera_model);
}

// gs_project_fwd in the antialiased mode (pinhole): + compensations [C*N], never NULL
extern "C" int gs_project_fwd_aa(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                                 const float* quats, const float* scales, const float* opacities,
                                 const float* colors_in, const float* sh_rest, int colors_per_camera,
                                 const float* viewmats, const float* Ks, int width, int height,
                                 float eps2d, float near_plane, float far_plane, float radius_clip,
                                 int tile_culling, int stage, int activations, int32_t* radii,
                                 float* means2d, float* depths, float* conics, float* colors_out, float* rec,
                                 uint32_t* bbox, int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac, float* compensations) {
    return project_fwd(stream, C, N, K, sh_degree, means, quats, scales, opacities, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radius_clip, tile_culling, stage, activations, radii, means2d, depths,
                       conics, colors_out, rec, bbox, tiles_per_gauss, rect_ref, sh_jac, GS_CAMERA_PINHOLE, true, compensations);
}

static int project_bwd(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count, int camera_model, bool aa = false, float* v_op_rec = nullptr) {
    GS_REQUIRE_CAMERA(camera_model);
    GS_REQUIRE(camera_model == GS_CAMERA_PINHOLE || !row_sums, "row_sums (the view-parallel step's form) exist for the pinhole model only");
    GS_REQUIRE(!aa || (camera_model == GS_CAMERA_PINHOLE && !row_sums), "the antialiased mode: the pinhole model, the gradient rows walked (no row_sums)");
    GS_REQUIRE(!aa || N == 0 || opacities, "the antialiased mode needs the opacities");
    GS_REQUIRE(!aa || current_rounds().phase == 0, "the antialiased mode is one-round only");
    GS_REQUIRE(C >= 1 && N >= 0 && width > 0 && height > 0, "C>=1, N>=0, positive image size");
    GS_REQUIRE((stat_grad_norm == nullptr) == (stat_count == nullptr) && (!stat_count || (C == 1 && row_sums)),
               "stat_grad_norm / stat_count: both or neither, single camera, together with row_sums");
    GS_REQUIRE(sh_degree <= 4, "sh_degree must be <= 4");
    GS_REQUIRE(sh_degree < 0 || (K >= (sh_degree + 1) * (sh_degree + 1) && K <= 25), "K must hold (sh_degree+1)^2 coefficients and be <= 25");
    if (N == 0) return GS_OK;
    GS_REQUIRE(means && quats && scales && colors_in && viewmats && Ks && radii && colors_post && tiles_per_gauss && cum_tiles, "null input pointer");
    GS_REQUIRE(row_sums || (rows && row_base && qmask), "the gradient rows (rows + row_base + qmask) or their sums (row_sums, from gs_row_sums)");
    GS_REQUIRE(v_means && v_quats && v_scales && v_opacities && v_means2d_abs, "null output pointer");
    GS_REQUIRE(v_colors || sh_degree >= 0, "v_colors may be NULL only with SH colours (gradients rebuilt by gs_sh_grad_views)");
    ProjBwdArgs a;
    a.C = C; a.N = N; a.K = K; a.colors_per_camera = colors_per_camera; a.W = width; a.H = height;
    a.eps2d = eps2d; a.near_p = near_plane; a.far_p = far_plane;
    a.means = means; a.quats = quats; a.scales = scales; a.colors_in = colors_in; a.viewmats = viewmats;
    a.sh_rest = sh_degree >= 0 ? sh_rest : nullptr; a.v_sh_rest = a.sh_rest ? v_sh_rest : nullptr;
    a.Ks = Ks; a.colors_post = colors_post; a.radii = radii; a.tiles_per_gauss = tiles_per_gauss;
    a.cum_tiles = cum_tiles; a.rows = reinterpret_cast<const float4*>(rows); a.row_base = row_base; a.qmask = qmask;
    a.v_means = v_means; a.v_quats = v_quats; a.v_scales = v_scales; a.v_opacities = v_opacities;
    a.v_colors = v_colors; a.v_means2d_abs = v_means2d_abs; a.v_means2d = v_means2d;
    a.v_conics = v_conics; a.v_colors_post = v_colors_post; a.v_colors_pre = sh_degree >= 0 ? v_colors_pre : nullptr;
    GS_REQUIRE(!activations || opacities, "activations need the raw opacities");
    a.opacities = opacities; a.activations = activations != 0;
    a.sh_jac = sh_degree >= 0 ? reinterpret_cast<const float4*>(sh_jac) : nullptr;
    a.guard = current_guard().info;
    a.rblk = current_rounds().phase == 3 ? current_rounds().blk : nullptr;   // (depth rounds: the rows are two ranges)
    a.adam = 0; a.ad_hyper = nullptr; a.ad_applied = nullptr; a.ad_b1 = a.ad_b2 = a.ad_eps = 0.f;
    a.st_max_radii = a.st_grad_norm = a.st_counts = nullptr; a.st_max_hw = (float)(width > height ? width : height);
    a.row_sums = row_sums; a.st_gn_out = stat_grad_norm; a.st_cnt_out = stat_count;
    a.ad_pbase = a.ad_mbase = a.ad_vbase = nullptr;
    for (int t = 0; t < 6; ++t) a.ad_off[t] = 0;
    a.reg_ratio = a.reg_grad = 0.f;
    a.v_op_rec = v_op_rec;
    dim3 grid((unsigned)((N + kProjThreads - 1) / kProjThreads));
    const size_t lds = proj_bwd_lds_bytes(K, sh_degree);
    hipStream_t st = (hipStream_t)stream;
    // One launch per camera: launch c accumulates onto launch c-1 (same thread owns Gaussian n in
    // every launch, stream order serialises them) -> deterministic sum over cameras, no atomics.
    for (int c = 0; c < C; ++c) {
        a.cam = c; a.accumulate = c > 0;
#define GS_PBC(D, M) { GS_LDS((project_bwd_cm_kernel<D, false, 0, M>)); hipLaunchKernelGGL((project_bwd_cm_kernel<D, false, 0, M>), grid, dim3(kProjThreads), lds, st, a); }
#define GS_PB(D)                                                                                                        \
        if (aa) { GS_LDS((project_bwd_aa_kernel<D, false, 0>)); hipLaunchKernelGGL((project_bwd_aa_kernel<D, false, 0>), grid, dim3(kProjThreads), lds, st, a); } else \
        if (camera_model == GS_CAMERA_ORTHO) GS_PBC(D, kCamOrtho) else if (camera_model == GS_CAMERA_FISHEYE) GS_PBC(D, kCamFisheye) else \
        if (row_sums) { GS_LDS((project_bwd_kernel<D, false, true>)); hipLaunchKernelGGL((project_bwd_kernel<D, false, true>), grid, dim3(kProjThreads), lds, st, a); } \
        else { GS_LDS((project_bwd_kernel<D, false, false>)); hipLaunchKernelGGL((project_bwd_kernel<D, false, false>), grid, dim3(kProjThreads), lds, st, a); }
        switch (sh_degree) {
            case 0: GS_PB(0); break;
            case 1: GS_PB(1); break;
            case 2: GS_PB(2); break;
            case 3: GS_PB(3); break;
            case 4: GS_PB(4); break;
            default: GS_PB(-1); break;
        }
#undef GS_PB
#undef GS_PBC
        GS_LAUNCH_CHECK("project_bwd_kernel");
    }
    return GS_OK;
}

extern "C" int gs_project_bwd(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count) {
    return project_bwd(stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                       row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                       v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                       stat_grad_norm, stat_count, GS_CAMERA_PINHOLE);
}

// gs_project_bwd under the camera model `camera_model` (GS_CAMERA_PINHOLE: that very call; the others walk the gradient rows: row_sums NULL)
extern "C" int gs_project_bwd_cm(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count, int camera_model) {
    return project_bwd(stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                       row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                       v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                       stat_grad_norm, stat_count, camera_model);
}

// gs_project_bwd in the antialiased mode (pinhole; opacities never NULL; the gradient rows are walked: row_sums NULL)
extern "C" int gs_project_bwd_aa(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count) {
    return project_bwd(stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                       row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                       v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                       stat_grad_norm, stat_count, GS_CAMERA_PINHOLE, true);
}


extern "C" size_t gs_cam_partials_doubles(int C, int64_t N) {
    if (C < 1 || N < 0) return 0;
    return (size_t)C * (size_t)((N + kProjThreads - 1) / kProjThreads) * 16;
}

// The antialiased mode's partials: gs_cam_partials_doubles' blocks, and behind them C*N floats -- the record-opacity gradient the projection
// backward leaves per (camera, Gaussian) for the camera kernel (ProjBwdArgs::v_op_rec)
extern "C" size_t gs_cam_partials_doubles_aa(int C, int64_t N) {
    if (C < 1 || N < 0) return 0;
    return gs_cam_partials_doubles(C, N) + ((size_t)C * (size_t)N + 1) / 2;
}

static int project_bwd_cam(int camera_model, void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                                  const float* quats, const float* scales, const float* colors_in,
                                  const float* sh_rest, int colors_per_camera, const float* viewmats,
                                  const float* Ks, int width,
                                  int height, float eps2d, float near_plane, float far_plane,
                                  const int32_t* radii, const float* colors_post,
                                  const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                                  const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                                  float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                                  float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                                  const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                                  float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats,
                                  float* v_campos, bool aa = false) {
    GS_REQUIRE_CAMERA(camera_model);
    GS_REQUIRE(C >= 1 && N >= 0, "C>=1, N>=0");
    GS_REQUIRE(v_viewmats && v_campos && (N == 0 || cam_partials), "null camera-gradient pointer");
    GS_REQUIRE(N == 0 || (v_means2d && v_conics && (sh_degree < 1 || v_colors_post)),
               "the camera gradients are formed from v_means2d / v_conics (and v_colors_post with SH degree >= 1): not optional here");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        GS_HIP_CHECK(hipMemsetAsync(v_viewmats, 0, sizeof(float) * 16 * C, st));
        GS_HIP_CHECK(hipMemsetAsync(v_campos, 0, sizeof(float) * 3 * C, st));
        return GS_OK;
    }
    GS_REQUIRE(((uintptr_t)quats & 15) == 0 && ((uintptr_t)v_means2d & 7) == 0 && ((uintptr_t)cam_partials & 7) == 0,
               "quats 16-byte, v_means2d and cam_partials 8-byte aligned");
    if (int rc = project_bwd(stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                             width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                             row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                             v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                             stat_grad_norm, stat_count, camera_model, aa,
                             aa ? reinterpret_cast<float*>(cam_partials + gs_cam_partials_doubles(C, N)) : nullptr))
        return rc;
    ProjCamArgs a;
    a.K = K; a.W = width; a.H = height; a.activations = activations != 0; a.N = N;
    a.eps2d = eps2d; a.near_p = near_plane; a.far_p = far_plane;
    a.means = means; a.quats = quats; a.scales = scales; a.viewmats = viewmats; a.Ks = Ks; a.colors_post = colors_post;
    // coefficient 1 onwards: the sh_rest rows of the split layout, or behind coefficient 0 of the dense block
    const bool split = sh_degree >= 0 && sh_rest != nullptr;
    a.sh_from_1 = split ? sh_rest : colors_in + 3; a.sh_stride = split ? 3 * (int64_t)(K - 1) : 3 * (int64_t)K;
    a.radii = radii; a.sh_jac = sh_degree >= 1 ? reinterpret_cast<const float4*>(sh_jac) : nullptr;
    a.v_means2d = v_means2d; a.v_conics = v_conics; a.v_colors_post = v_colors_post; a.row_sums = nullptr;
    a.cam_partials = cam_partials; a.guard = current_guard().info;
    a.opacities = opacities; a.v_op_rec = aa ? reinterpret_cast<const float*>(cam_partials + gs_cam_partials_doubles(C, N)) : nullptr;
    const int n_blocks = (int)((N + kProjThreads - 1) / kProjThreads);
    dim3 grid((unsigned)n_blocks, (unsigned)C);
#define GS_PC(D)                                                                                                                         \
    if (aa) hipLaunchKernelGGL((project_cam_aa_kernel<D>), grid, dim3(kProjThreads), 0, st, a); else                                     \
    if (camera_model == GS_CAMERA_ORTHO) hipLaunchKernelGGL((project_cam_cm_kernel<D, kCamOrtho>), grid, dim3(kProjThreads), 0, st, a);          \
    else if (camera_model == GS_CAMERA_FISHEYE) hipLaunchKernelGGL((project_cam_cm_kernel<D, kCamFisheye>), grid, dim3(kProjThreads), 0, st, a); \
    else hipLaunchKernelGGL((project_cam_kernel<D>), grid, dim3(kProjThreads), 0, st, a)
    switch (sh_degree) {
        case 1: GS_PC(1); break;
        case 2: GS_PC(2); break;
        case 3: GS_PC(3); break;
        case 4: GS_PC(4); break;
        default: GS_PC(0); break;   // (degree 0 and colour features: no direction term)
    }
#undef GS_PC
    GS_LAUNCH_CHECK("project_cam_kernel");
    hipLaunchKernelGGL(cam_sum_kernel, dim3((unsigned)C), dim3(16 * kCamSumChains), 0, st, (const double*)cam_partials, n_blocks, v_viewmats, v_campos, a.guard);
    GS_LAUNCH_CHECK("cam_sum_kernel");
    return GS_OK;
}

extern "C" int gs_project_bwd_cam(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats, float* v_campos) {
    return project_bwd_cam(GS_CAMERA_PINHOLE, stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                       row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                       v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                       stat_grad_norm, stat_count, cam_partials, v_viewmats, v_campos);
}

// gs_project_bwd_cam in the antialiased mode (pinhole): cam_partials holds gs_cam_partials_doubles_aa(C, N) doubles
extern "C" int gs_project_bwd_cam_aa(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats, float* v_campos) {
    return project_bwd_cam(GS_CAMERA_PINHOLE, stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                       row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                       v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                       stat_grad_norm, stat_count, cam_partials, v_viewmats, v_campos, true);
}

// gs_project_bwd_cam under the camera model `camera_model` (GS_CAMERA_PINHOLE: that very call)
extern "C" int gs_project_bwd_cam_cm(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                              const float* quats, const float* scales, const float* colors_in,
                              const float* sh_rest, int colors_per_camera, const float* viewmats,
                              const float* Ks, int width,
                              int height, float eps2d, float near_plane, float far_plane,
                              const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                              const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats, float* v_scales,
                              float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                              float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                              const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                              float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats, float* v_campos, int camera_model) {
    return project_bwd_cam(camera_model, stream, C, N, K, sh_degree, means, quats, scales, colors_in, sh_rest, colors_per_camera, viewmats, Ks,
                       width, height, eps2d, near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows,
                       row_base, qmask, v_means, v_quats, v_scales, v_opacities, v_colors, v_sh_rest, v_means2d_abs,
                       v_means2d, v_conics, v_colors_post, v_colors_pre, opacities, activations, sh_jac, row_sums,
                       stat_grad_norm, stat_count, cam_partials, v_viewmats, v_campos);
}

// The camera gradients of the single-camera step from gs_row_sums' per-Gaussian sums (the captured step with poses): the kernels and
// the reduction of gs_project_bwd_cam, fed from the sums because the fused projection backward + Adam writes no gradient tensor.
extern "C" int gs_cam_grad_sums(void* stream, int64_t N, int K, int sh_degree, const float* means, const float* quats, const float* scales,
                                const float* sh_rest, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                                float near_plane, float far_plane, const int32_t* radii, const float* colors_post, int activations,
                                const float* sh_jac, const float* row_sums, double* cam_partials, float* v_viewmats, float* v_campos) {
    GS_REQUIRE(N >= 0 && width > 0 && height > 0, "N>=0, positive image size");
    GS_REQUIRE(sh_degree <= 4 && (sh_degree < 0 || (K >= (sh_degree + 1) * (sh_degree + 1) && K <= 25)), "sh_degree <= 4, (degree+1)^2 <= K <= 25");
    GS_REQUIRE(v_viewmats && v_campos && (N == 0 || cam_partials), "null camera-gradient pointer");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        GS_HIP_CHECK(hipMemsetAsync(v_viewmats, 0, sizeof(float) * 16, st));
        GS_HIP_CHECK(hipMemsetAsync(v_campos, 0, sizeof(float) * 3, st));
        return GS_OK;
    }
    GS_REQUIRE(means && quats && scales && viewmats && Ks && radii && colors_post && row_sums, "null input pointer");
    GS_REQUIRE(sh_degree < 1 || sh_jac || sh_rest, "SH degree >= 1 needs sh_jac or the coefficients (sh_rest)");
    GS_REQUIRE(((uintptr_t)quats & 15) == 0 && ((uintptr_t)row_sums & 15) == 0 && ((uintptr_t)cam_partials & 7) == 0,
               "quats and row_sums 16-byte, cam_partials 8-byte aligned");
    ProjCamArgs a;
    a.K = K; a.W = width; a.H = height; a.activations = activations != 0; a.N = N;
    a.eps2d = eps2d; a.near_p = near_plane; a.far_p = far_plane;
    a.means = means; a.quats = quats; a.scales = scales; a.viewmats = viewmats; a.Ks = Ks; a.colors_post = colors_post;
    a.sh_from_1 = sh_rest; a.sh_stride = 3 * (int64_t)(K - 1);   // (the split layout)
    a.radii = radii; a.sh_jac = sh_degree >= 1 ? reinterpret_cast<const float4*>(sh_jac) : nullptr;
    a.v_means2d = a.v_conics = a.v_colors_post = nullptr; a.row_sums = reinterpret_cast<const float4*>(row_sums);
    a.cam_partials = cam_partials; a.guard = current_guard().info;
    a.opacities = a.v_op_rec = nullptr;
    const int n_blocks = (int)((N + kProjThreads - 1) / kProjThreads);
    dim3 grid((unsigned)n_blocks, 1u);
#define GS_PC(D) hipLaunchKernelGGL((project_cam_kernel<D, true>), grid, dim3(kProjThreads), 0, st, a)
    switch (sh_degree) {
        case 1: GS_PC(1); break;
        case 2: GS_PC(2); break;
        case 3: GS_PC(3); break;
        case 4: GS_PC(4); break;
        default: GS_PC(0); break;
    }
#undef GS_PC
    GS_LAUNCH_CHECK("project_cam_kernel (row sums)");
    hipLaunchKernelGGL(cam_sum_kernel, dim3(1u), dim3(16 * kCamSumChains), 0, st, (const double*)cam_partials, n_blocks, v_viewmats, v_campos, a.guard);
    GS_LAUNCH_CHECK("cam_sum_kernel");
    return GS_OK;
}

// Row reduction + SH-bwd + P-bwd + Adam in ONE pass (train-step graph, single camera): gs_project_bwd with the
// reference model's raw parameters (log-scales, logit opacities, split SH), but instead of writing the 59 gradients
// per Gaussian and reading them back in gs_adam_step, every parameter and both of its moments are updated in place
// where the gradient is formed.  params / exp_avg / exp_avg_sq: the flat buffers of gs_adam_step, the six tensors
// of param_names at offsets_host[6] floats.  hyper_dev: gs_adam_hyper.  Only v_means2d_abs (the `.absgrad`
// side channel) is still written; with max_radii / grad_norm_accum / counts given, update_statistics is applied too.
static int project_bwd_adam(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                            const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                            float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                            const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                            float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                            int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                            const float* sh_jac, int reg, float max_ratio, float lambda, double bud_a, double bud_b,
                            const float* row_sums = nullptr, const float* v_depths = nullptr, int camera_model = GS_CAMERA_PINHOLE,
                            bool aa = false, bool selective = false) {
    GS_REQUIRE_CAMERA(camera_model);
    GS_REQUIRE(!selective || (!aa && camera_model == GS_CAMERA_PINHOLE && !(reg & 2) && !row_sums && !v_depths),
               "the selective fused backward: pinhole, classic mode, gradient rows; no budget, row-sums or depth variant of it exists");
    GS_REQUIRE(!aa || (camera_model == GS_CAMERA_PINHOLE && !(reg & 2) && !row_sums && !v_depths),
               "the antialiased mode: the pinhole model; no budget, row-sums or depth variant of the fused backward exists for it");
    GS_REQUIRE(!aa || current_rounds().phase == 0, "the antialiased mode is one-round only");
    GS_REQUIRE(camera_model == GS_CAMERA_PINHOLE || (!(reg & 2) && !row_sums && !v_depths),
               "the budget, row-sums and depth variants of the fused backward exist for the pinhole model only");
    GS_REQUIRE(N >= 0 && width > 0 && height > 0, "N>=0, positive image size");
    GS_REQUIRE(sh_degree >= 0 && sh_degree <= 4 && K >= (sh_degree + 1) * (sh_degree + 1) && K <= 25, "SH colours: 0 <= degree <= 4, (degree+1)^2 <= K <= 25");
    if (N == 0) return GS_OK;
    GS_REQUIRE(params && exp_avg && exp_avg_sq && offsets_host && viewmats && Ks && radii && colors_post && tiles_per_gauss &&
               cum_tiles && v_means2d_abs && hyper_dev, "null pointer");
    GS_REQUIRE(row_sums ? ((uintptr_t)row_sums & 15) == 0 : (rows && row_base && qmask),
               "the gradient rows (rows + row_base + qmask) or their sums (row_sums, 16-byte aligned, from gs_row_sums)");
    ProjBwdArgs a;
    a.C = 1; a.N = N; a.K = K; a.colors_per_camera = 0; a.W = width; a.H = height;
    a.eps2d = eps2d; a.near_p = near_plane; a.far_p = far_plane;
    a.means = params + offsets_host[0]; a.scales = params + offsets_host[1]; a.quats = params + offsets_host[2];
    a.colors_in = params + offsets_host[3]; a.sh_rest = K > 1 ? params + offsets_host[4] : nullptr;
    a.opacities = params + offsets_host[5]; a.activations = 1;
    GS_REQUIRE(((uintptr_t)a.quats & 15) == 0, "the quaternion tensor must be 16-byte aligned");
    a.viewmats = viewmats; a.Ks = Ks; a.colors_post = colors_post; a.radii = radii; a.tiles_per_gauss = tiles_per_gauss;
    a.cum_tiles = cum_tiles; a.rows = reinterpret_cast<const float4*>(rows); a.row_base = row_base; a.qmask = qmask;
    a.v_means = a.v_quats = a.v_scales = a.v_opacities = a.v_colors = a.v_sh_rest = nullptr;
    a.v_means2d_abs = v_means2d_abs; a.v_means2d = a.v_conics = a.v_colors_post = a.v_colors_pre = nullptr;
    a.sh_jac = reinterpret_cast<const float4*>(sh_jac);
    a.guard = current_guard().info;
    a.rblk = current_rounds().phase == 3 ? current_rounds().blk : nullptr;   // (depth rounds: the rows are two ranges)
    a.adam = 1; a.ad_hyper = hyper_dev; a.ad_applied = applied_dev; a.ad_b1 = beta1; a.ad_b2 = beta2; a.ad_eps = eps;
    GS_REQUIRE((max_radii == nullptr) == (grad_norm_accum == nullptr) && (max_radii == nullptr) == (counts == nullptr),
               "the three statistics buffers come together or not at all");
    a.st_max_radii = max_radii; a.st_grad_norm = grad_norm_accum; a.st_counts = counts;
    a.st_max_hw = (float)(width > height ? width : height);
    a.row_sums = row_sums; a.st_gn_out = a.st_cnt_out = nullptr;
    a.ad_pbase = params; a.ad_mbase = exp_avg; a.ad_vbase = exp_avg_sq;
    for (int t = 0; t < 6; ++t) a.ad_off[t] = offsets_host[t];
    a.cam = 0; a.accumulate = 0;
    a.reg_ratio = max_ratio; a.reg_grad = (reg & 1) ? scale_reg_upstream(lambda, N) : 0.f;
    a.bud_ga = (reg & 2) ? budget_reg_upstream(bud_a, N) : 0.f; a.bud_gb = (reg & 2) ? budget_reg_upstream(bud_b, 3 * N) : 0.f;
    a.v_depths = v_depths;
    a.v_op_rec = nullptr;
    dim3 grid((unsigned)((N + kProjThreads - 1) / kProjThreads));
    const size_t lds = proj_bwd_lds_bytes(K, sh_degree);
    hipStream_t st = (hipStream_t)stream;
    // (the row_sums forms -- gs_project_bwd_adam_sums -- are instantiations of their own; the compiler's resource report shows
    //  none of them with scratch: a kernel that declares it makes the runtime provision it -- gs_blend.hip, GS_FWD_TRAIN_WAVES_PER_EU)
#define GS_PBK(...) { GS_LDS((__VA_ARGS__)); hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(kProjThreads), lds, st, a); }
    // (degree 4 with the regulariser under the fisheye: the branch-free form of its radial terms, kCamFisheyeSelect -- with the branch the
    //  compiler reserves 36 bytes of scratch per lane for this one instantiation, which no instruction of it touches)
#define GS_PBC(D, M)                                                                                                                     \
    if (reg == 1) GS_PBK(project_bwd_cm_kernel<D, true, 1, ((D) == 4 && (M) == kCamFisheye) ? kCamFisheyeSelect : (M)>)                   \
    else GS_PBK(project_bwd_cm_kernel<D, true, 0, M>)
#define GS_PB(D)                                                                                                        \
    if (selective) { if (reg == 1) GS_PBK(project_bwd_selective_kernel<D, 1>) else GS_PBK(project_bwd_selective_kernel<D, 0>) } else \
    if (aa) { if (reg == 1) GS_PBK(project_bwd_aa_kernel<D, true, 1>) else GS_PBK(project_bwd_aa_kernel<D, true, 0>) } else \
    if (camera_model == GS_CAMERA_ORTHO) { GS_PBC(D, kCamOrtho) } else if (camera_model == GS_CAMERA_FISHEYE) { GS_PBC(D, kCamFisheye) } else \
    if (v_depths) {                                                                                                     \
        if (reg == 3) GS_PBK(project_bwd_depth_kernel<D, 7>) else if (reg == 2) GS_PBK(project_bwd_depth_kernel<D, 6>)                  \
        else if (reg == 1) GS_PBK(project_bwd_depth_kernel<D, 5>) else GS_PBK(project_bwd_depth_kernel<D, 4>)                           \
    } else if (row_sums) {                                                                                                     \
        if (reg == 3) GS_PBK(project_bwd_budget_kernel<D, 3, true>) else if (reg == 2) GS_PBK(project_bwd_budget_kernel<D, 2, true>)    \
        else if (reg == 1) GS_PBK(project_bwd_kernel<D, true, true, true>) else GS_PBK(project_bwd_kernel<D, true, true>)               \
    } else if (reg == 3) GS_PBK(project_bwd_budget_kernel<D, 3>) else if (reg == 2) GS_PBK(project_bwd_budget_kernel<D, 2>)             \
    else if (reg == 1) GS_PBK(project_bwd_kernel<D, true, false, true>) else GS_PBK(project_bwd_kernel<D, true, false>)
    switch (sh_degree) {
        case 0: GS_PB(0); break;
        case 1: GS_PB(1); break;
        case 2: GS_PB(2); break;
        case 3: GS_PB(3); break;
        default: GS_PB(4); break;
    }
#undef GS_PB
#undef GS_PBC
#undef GS_PBK
    GS_LAUNCH_CHECK("project_bwd_kernel (fused Adam)");
    return GS_OK;
}

extern "C" int gs_project_bwd_adam(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                   const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                   float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                   const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                                   float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                   int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                   const float* sh_jac) {
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 0, 0.f, 0.f, 0.0, 0.0);
}

// ... with the scale-ratio regulariser's gradient in v_scale (its value: gs_scale_reg in front of this call)
extern "C" int gs_project_bwd_adam_reg(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                       const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                       float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                       const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                                       const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                       int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                       const float* sh_jac, float max_ratio, float lambda) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 1, max_ratio, lambda, 0.0, 0.0);
}

// gs_project_bwd_adam / gs_project_bwd_adam_reg under the camera model `camera_model` (GS_CAMERA_PINHOLE: those very calls)
extern "C" int gs_project_bwd_adam_cm(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                   const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                   float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                   const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                                   float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                   int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                   const float* sh_jac, int camera_model) {
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 0, 0.f, 0.f, 0.0, 0.0,
                            nullptr, nullptr, camera_model);
}
extern "C" int gs_project_bwd_adam_reg_cm(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                   const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                   float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                   const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                                   float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                   int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                   const float* sh_jac, float max_ratio, float lambda, int camera_model) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 1, max_ratio, lambda, 0.0, 0.0,
                            nullptr, nullptr, camera_model);
}

// gs_project_bwd_adam / gs_project_bwd_adam_reg in the antialiased mode (pinhole)
extern "C" int gs_project_bwd_adam_aa(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                   const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                   float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                   const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                                   float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                   int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                   const float* sh_jac) {
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 0, 0.f, 0.f, 0.0, 0.0,
                            nullptr, nullptr, GS_CAMERA_PINHOLE, true);
}
extern "C" int gs_project_bwd_adam_reg_aa(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                   const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                   float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                   const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                                   float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                   int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                   const float* sh_jac, float max_ratio, float lambda) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 1, max_ratio, lambda, 0.0, 0.0,
                            nullptr, nullptr, GS_CAMERA_PINHOLE, true);
}

// gs_project_bwd_adam (reg_on = 0) / gs_project_bwd_adam_reg (reg_on = 1) over the Gaussians the step saw: project_bwd_selective_kernel
extern "C" int gs_project_bwd_selective(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                        const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                        float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                        const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                                        const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                        int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                        const float* sh_jac, int reg_on, float max_ratio, float lambda) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    GS_REQUIRE(reg_on == 0 || reg_on == 1, "reg_on is 0 or 1");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, reg_on, max_ratio, lambda, 0.0, 0.0,
                            nullptr, nullptr, GS_CAMERA_PINHOLE, false, true);
}

// ... with the budget regulariser's gradients in v_opacity and v_scale (its value: gs_mcmc_reg in front of this call), behind the
// scale-ratio term when `scale_reg` is set
extern "C" int gs_project_bwd_adam_mcmc(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                        const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                        float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                        const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                                        const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                        int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                        const float* sh_jac, int scale_reg, float max_ratio, float lambda, double a, double b) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    GS_REQUIRE(scale_reg == 0 || scale_reg == 1, "scale_reg is 0 or 1");
    GS_REQUIRE(a == a && b == b, "a or b is NaN");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, 2 | scale_reg,
                            max_ratio, lambda, a, b);
}

// ... from the row sums gs_row_sums left (the captured step with poses: the camera gradient is formed from the same sums in front of
// this call, so the gradient rows are walked once per step), with any of the two regularisers: the same update, bit for bit, as the
// row-walking entries above -- row_sums_kernel and project_bwd_kernel share row_sum_wave.
extern "C" int gs_project_bwd_adam_sums(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                        const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                        float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                        const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* row_sums,
                                        float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                        int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                        const float* sh_jac, int scale_reg, float max_ratio, float lambda, int budget, double a, double b) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    GS_REQUIRE((scale_reg == 0 || scale_reg == 1) && (budget == 0 || budget == 1), "scale_reg and budget are 0 or 1");
    GS_REQUIRE(a == a && b == b, "a or b is NaN");
    GS_REQUIRE(N == 0 || row_sums, "row_sums: gs_row_sums' per-Gaussian sums");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, nullptr, nullptr, nullptr, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, (budget ? 2 : 0) | scale_reg,
                            max_ratio, lambda, a, b, row_sums);
}

// ... with the depth channel's gradient in v_mean: v_depths[N] (gs_depth_grads_z on the step's gradient rows, just before) times row 2 of
// the view matrix, behind the projection's VJP and in front of the regularisers -- the order of gs_project_bwd, gs_depth_grads,
// gs_scale_reg / gs_mcmc_reg, gs_adam_step_dev, hence the same update bit for bit.  An instantiation of its own per (degree, regulariser
// mask): the existing kernels compile as they did.
extern "C" int gs_project_bwd_adam_depth(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                                         const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                                         float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                                         const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                                         const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                                         int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                                         const float* sh_jac, int scale_reg, float max_ratio, float lambda, int budget, double a, double b,
                                         const float* v_depths) {
    GS_REQUIRE(((uintptr_t)params & 3) == 0, "params must be 4-byte aligned");
    GS_REQUIRE((scale_reg == 0 || scale_reg == 1) && (budget == 0 || budget == 1), "scale_reg and budget are 0 or 1");
    GS_REQUIRE(a == a && b == b, "a or b is NaN");
    GS_REQUIRE(N == 0 || (v_depths && ((uintptr_t)v_depths & 3) == 0), "v_depths: gs_depth_grads_z' per-Gaussian depth gradients");
    GS_REQUIRE(current_rounds().phase == 0, "depth gradients are one-round only");
    return project_bwd_adam(stream, N, K, sh_degree, params, exp_avg, exp_avg_sq, offsets_host, viewmats, Ks, width, height, eps2d,
                            near_plane, far_plane, radii, colors_post, tiles_per_gauss, cum_tiles, rows, row_base, qmask, v_means2d_abs,
                            beta1, beta2, eps, hyper_dev, applied_dev, max_radii, grad_norm_accum, counts, sh_jac, (budget ? 2 : 0) | scale_reg,
                            max_ratio, lambda, a, b, nullptr, v_depths);
}
