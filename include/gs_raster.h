/*
 * gs_raster.h -- C ABI of the MI355X (gfx950) Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary for the ONE call the reference makes into its rasterizer:
 *
 *     from gsplat.rendering import rasterization            (/root/reference/model/gaussian.py:8)
 *     rasterization(means, quats, scales, opacities, colors, viewmats, Ks, width, height,
 *                   sh_degree=..., backgrounds=..., absgrad=True, packed=False)
 *                                                           (/root/reference/model/gaussian.py:353-367)
 *
 * gsplat 1.0.0 reaches its CUDA kernels through per-stage torch ops; each entry point below is
 * the stage a binding for this path would call instead (stage names: SURVEY.md section 2.2).
 * Plain pointers and sizes only: every pointer is a DEVICE pointer unless its name ends in
 * `_host`; `stream` is a hipStream_t passed as void*.  All tensors are dense row-major fp32 /
 * int32 / int64.  Every function returns 0 on success and a negative code on failure, in which
 * case gs_last_error() (thread-local) describes it.  Nothing is allocated inside; the caller owns
 * all memory (ownership contract: SURVEY.md section 8b).  Entry points may be called from any
 * host thread.
 *
 * Index vocabulary: C cameras, N Gaussians, K stored SH coefficients per Gaussian, flatten id
 * f = c*N + n, tiles = tile_w*tile_h (16x16 pixel tiles), I = number of (tile, Gaussian)
 * intersections, bucket = 64 consecutive entries of one tile's depth-sorted list.
 */
#ifndef GS_RASTER_H_
#define GS_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_TILE 16           /* tile edge in pixels (gsplat default tile_size=16) */
#define GS_BUCKET 64         /* entries per bucket = one wavefront */
#define GS_UNIT 32           /* quadrant-sublist entries per work unit of gs_blend_bwd (one checkpoint each) */
#define GS_REC_FLOATS 12     /* packed per-(camera,Gaussian) blend record */
#ifndef GS_ROW_FLOATS
#define GS_ROW_FLOATS 12     /* per-intersection gradient row written by gs_blend_bwd */
#endif

/* Walk state of a training forward (gs_blend_fwd -> gs_blend_bwd): int32 words, followed by the chunk counts of the row-base scan.
 * gs_walk_state_ints(n_isects) = GS_WALK_WORDS + n_isects / 8192 + 1 words; 8-byte aligned; cleared by gs_blend_fwd itself. */
#define GS_WALK_UNITS 0      /* work units published (descriptors written) */
#define GS_WALK_STORAGE 1    /* storage units needed = GS_WALK_RANGES x the fullest range's count: what cap_units has to hold */
#define GS_WALK_ROWS 3       /* gradient rows = (intersection, quadrant) pairs some pixel took: what cap_rows has to hold */
#define GS_WALK_FLAGS 4      /* GS_FLAG_UNITS / GS_FLAG_ROWS of this call */
#define GS_WALK_SKIP 5       /* 1: the step guard was tripped when the call started -- its kernels did nothing */
#define GS_WALK_RANGES 32    /* the storage units are handed out from 32 counters, each over its own 1/32 of [0, cap_units) and in */
#define GS_WALK_RANGE0 32    /* a cache line of its own: word GS_WALK_RANGE0 + 32 * r (one counter took 30 k same-address atomics per frame) */
#define GS_WALK_WORDS (GS_WALK_RANGE0 + 32 * GS_WALK_RANGES)
/* Size record ("info block") of the list stages: int64[GS_INFO_WORDS], written by gs_bin_count (the first four words) and
 * gs_bins_count (all of them); the GS_WS_INFO slot of a workspace, info_dev / info_host below. */
#define GS_INFO_ISECTS 0     /* I: (tile, Gaussian) intersections listed */
#define GS_INFO_BUCKETS 1    /* n_buckets */
#define GS_INFO_MAX_TILE 2   /* longest tile list */
#define GS_INFO_FLAGS 3      /* GS_FLAG_* */
#define GS_INFO_COARSE 4     /* two-level binning: I', the coarse-bin entries */
#define GS_INFO_MAX_BIN 5    /* two-level binning: longest bin list */
#define GS_INFO_LIVE 6       /* chunks (depth rounds: tiles the front round left live) */
#define GS_INFO_ONE_ROUND 7  /* one-round I of a call in depth rounds */
#define GS_INFO_WORDS 8
/* Flag bits of an info block (info_dev[GS_INFO_FLAGS], gs_guard_set) */
#define GS_FLAG_ISECTS 1     /* I > cap_isects */
#define GS_FLAG_TILE 2       /* a tile list longer than cap_tile */
#define GS_FLAG_COARSE 4     /* two-level binning: coarse entries > coarse_cap */
#define GS_FLAG_COARSE_LIST 8 /* two-level binning: a bin list longer than coarse_list_cap */
#define GS_FLAG_UNITS 16     /* training forward: the walk opened more work units than cap_units */
#define GS_FLAG_ROWS 32      /* training forward: more gradient rows than cap_rows */
#define GS_FLAG_BACK 64      /* depth rounds, phase 4: the front round left live tiles and no back round was enqueued */
#define GS_FLAG_PEER 128     /* view-parallel step: another rank's guard was tripped (gs_guard_merge) */

#define GS_OK 0
#define GS_ERR_ARG (-1)
#define GS_ERR_HIP (-2)
#define GS_ERR_UNSUPPORTED (-3)

/* Library identity / diagnostics. */
int gs_version(void);
const char* gs_build_flags(void); /* preprocessor flags beyond the product build's ("" = the product library; a diagnostic variant names its own) */
const char* gs_last_error(void);
const char* gs_arch(void); /* "gfx950" */

/* Step guard: lets a whole step (forward, backward, statistics, Adam) be enqueued -- and captured into a
 * hipGraph -- without the host ever reading the list sizes back (SURVEY.md section 8b "Sync").  The caller
 * sizes every intersection-indexed buffer for cap_isects entries (bucket-indexed ones for
 * cap_isects/64 + C*tiles + 1 buckets), launches the sort classes for lists of up to cap_tile entries
 * (gs_bin_emit_sort's max_tile_count = cap_tile) and zeroes info_dev[3] once.  While the guard is set (per host
 * thread; pass NULL to clear), gs_bin_count ORs into info_dev[3]: 1 if I > cap_isects, 2 if a tile list exceeds
 * cap_tile; a training gs_blend_fwd ORs 16 if its walk opens more work units than its cap_units and 32 if it leaves more
 * gradient rows than its cap_rows; and gs_bin_emit_sort, gs_blend_fwd, gs_blend_bwd, gs_project_bwd, gs_update_statistics and
 * gs_adam_step[_dev] return at once on the device when info_dev[3] != 0: a step that does not fit -- and every
 * step enqueued behind it -- is a no-op the host can detect later (read info_dev), re-size for, clear and replay.
 * n_isects / max_tile_count arguments of those entry points may then be the capacities (the passes over the slots -- the clear
 * of the quadrant masks, the row-base scan -- stop at the I the tile scan left in info_dev[0]). */
int gs_guard_set(const int64_t* info_dev, int64_t cap_isects, int64_t cap_tile);
/* The same guard for ONE call (the eager seam: every rasterization() enqueues its list stages and blend speculatively under it):
 * the flags are not sticky across calls -- the call's first flag writer (gs_bins_count's bin scan, else gs_bin_count's tile scan)
 * OVERWRITES info_dev[3], so the info block need not be zeroed between calls. */
int gs_guard_set_call(const int64_t* info_dev, int64_t cap_isects, int64_t cap_tile);

/* Host mirror of the info block (per host thread; NULL clears it): page-locked host memory the device can address
 * (hipHostMalloc / torch pin_memory), int64[8].  While set, gs_bin_count / gs_bins_count have their last kernel write the eight
 * info words there as well, followed by a system-scope fence: a caller that records an event behind the call and waits for it
 * reads the list sizes and flags from plain memory -- no device-to-host copy (a 4 us transfer kernel and the idle gap behind
 * it) on the stream.  The blocking `info_host` argument of those calls is independent of this. */
int gs_info_mirror_set(int64_t* info_host_mapped);
/* The same for the walk record of a training gs_blend_fwd (per host thread; NULL clears it): int64[4] of page-locked, device-
 * addressable host memory; the call's last kernel writes {work units, storage units taken, gradient rows, GS_FLAG_UNITS |
 * GS_FLAG_ROWS} there, followed by a system-scope fence -- the eager seam's backward learns whether the walk fitted its
 * capacities (and what it needed) from plain memory. */
int gs_walk_mirror_set(int64_t* walk_host_mapped);

/* The step guard across ranks (row e: one view per rank, the captured view-parallel step).  A rank whose lists or walk outgrew its
 * capacities must not be the only replica that skips the step.  gs_guard_flag_out writes 1.0f / 0.0f (info_dev[3] != 0) to dst0
 * and dst1 (either may be NULL): the word of this rank's all-gather record and the word of the SUM all-reduce bucket that carry
 * it.  gs_guard_merge ORs GS_FLAG_PEER into info_dev[3] when any of the n floats flags[i * stride] is non-zero (the gathered
 * records' words; the reduced bucket's word): in front of the kernels that apply the step, on every rank -- all replicas skip,
 * or none.  gs_step_applied: applied_dev[0] += 1 unless the guard is tripped (the applied-step count of gs_step_status, for a
 * step whose update is not one of the fused kernels that count themselves). */
int gs_guard_flag_out(void* stream, const int64_t* info_dev, float* dst0, float* dst1);
int gs_guard_merge(void* stream, int64_t* info_dev, const float* flags, int n, int64_t stride);
int gs_step_applied(void* stream, const int64_t* info_dev, int64_t* applied_dev);

/* Depth rounds: refine-on-demand list stages (a per-tile order equal to the stable global sort is
 * contract-equivalent).  On realistic footprints 97-98 % of what the list stages count, emit and sort is never read: a tile
 * saturates a few hundred entries into a list of thousands.  With rounds the frame's Gaussians are split at a depth quantile
 * (gs_round_split): the FRONT round lists, sorts and blends the nearest slab only; the BACK round lists the rest only into the
 * tiles the front round left with live pixels (gs_round_footprints windows every footprint to them) and resumes those tiles'
 * blend from their saved pixel states.  Every depth of the front slab is smaller than every depth behind it, so a tile walks
 * the same entries in the same order as over one list: images, sublists, checkpoints and gradient rows are bit for bit those
 * of the one-round pipeline; only lists nobody reads are never built.  A Gaussian lives in exactly one round; the back round's
 * list entries and gradient-row slots continue behind the front round's (isect_offsets, flatten_ids, slots, qmask, row_base,
 * unit_desc, ckpt, qlist are ONE set of buffers for both), gs_blend_bwd needs no change and the row gather of gs_project_bwd* /
 * gs_row_sums reads a wave's rows as two ranges.
 * gs_rounds_set (per host thread, like gs_guard_set; phase 0 clears it) tells the entry points which round they work for:
 *   phase 1 (front round)  gs_round_footprints, gs_bin_count / gs_bin_emit_sort or gs_bins_count / gs_bins_lists, gs_blend_fwd
 *   phase 2 (back round)   the same calls again, on the same buffers
 *   phase 3 (behind both)  gs_project_bwd, gs_project_bwd_adam, gs_row_sums
 * Per round the caller passes the footprints gs_round_footprints wrote (bbox_round) to the list stages, and to the backward the
 * tiles_per_gauss it wrote (a Gaussian's count in ITS round).  Under phase 1 / 2 the list entry points require C == 1.
 *   rounds_dev[GS_ROUND_WORDS] i64   device block: see GS_ROUND_*; written by gs_round_split and the list stages
 *   tile_live[tiles] u8             1: the front round left the tile with live pixels
 *   tile_state[tiles*4*64*4] f32    pixel states (T, r, g, b) of the live tiles
 *   tile_rec[tiles*8] i32           training: lengths of the quadrant sublists and their part-filled work units (NULL: inference)
 * gs_blend_fwd in phase 1 clears the quadrant masks and the walk state and leaves the row-base scan to phase 2; render_colors /
 * render_alphas are complete after phase 2 (phase 1 writes every tile, phase 2 re-writes the tiles it resumes).  When the
 * front round leaves no live tile (rounds_dev[GS_ROUND_LIVE] == 0) the kernels of the back round return at once.
 *   phase 4 (front round ALONE, under a step guard)  the same calls as phase 1, speculating that the front round finishes the frame:
 * gs_blend_fwd runs its row-base scan itself, and a tile that still has live pixels ORs GS_FLAG_BACK into the guard's flag word --
 * the step is then void like one that outgrew a capacity (every kernel behind is a no-op), and the caller repeats it with both
 * rounds.  What a captured step saves: the ~18 launches of a back round that has nothing to do. */
#define GS_ROUND_BASE 0      /* list entries (= gradient-row slots) of the front round: the back round continues here */
#define GS_ROUND_SPLIT 1     /* depth split as float bits: a Gaussian is in the front round when its depth bits are below */
#define GS_ROUND_LIVE 2      /* tiles the front round left with live pixels */
#define GS_ROUND_FRONT_N 3   /* visible Gaussians in the front round (diagnostic) */
#define GS_ROUND_LISTED_ALL 4 /* what the frame would list in ONE round (sum of tiles_per_gauss); the tile scans of both rounds copy it to info_dev[7] */
#define GS_ROUND_WORDS 8
int gs_rounds_set(int64_t* rounds_dev, uint8_t* tile_live, float* tile_state, int32_t* tile_rec, int phase);
/* Depth split of a frame (C == 1): the smallest depth bin edge d such that the Gaussians nearer than d hold at least `fraction`
 * of the frame's listed intersections (histogram over the float bits >> 19: 16 bins per octave; weights tiles_per_gauss).
 * Writes rounds_dev[GS_ROUND_SPLIT] and zeroes GS_ROUND_BASE / GS_ROUND_LIVE.  hist_ws: 4096 u32 of scratch, ZERO on first use
 * (the call leaves it zero).  fraction >= 1: everything is front. */
int gs_round_split(void* stream, int64_t N, const float* depths, const int32_t* tiles_per_gauss, float fraction,
                   uint32_t* hist_ws, int64_t* rounds_dev);
/* Footprints of the current round (gs_rounds_set phase 1 or 2), in gs_project_fwd's bbox layout: phase 1 keeps the footprints
 * of the front slab and empties the others; phase 2 keeps those of the Gaussians behind the split, windowed to the live tiles
 * (footprints of <= 32 tiles: dead tiles leave the mask; larger ones shrink to the bounding rectangle of their live tiles, and
 * get a mask when that holds <= 32 tiles).  tiles_per_gauss_round[N]: phase 1 writes every count (0 behind the split), phase 2
 * only those of the Gaussians behind the split -- afterwards it holds every Gaussian's count in its own round. */
int gs_round_footprints(void* stream, int64_t N, int tile_w, int tile_h, const uint32_t* bbox, const float* depths,
                        uint32_t* bbox_round, int32_t* tiles_per_gauss_round);

/* The round block into page-locked, device-addressable host memory (int64[GS_ROUND_WORDS]; one tiny launch + a system-scope fence,
 * like gs_step_status): a host that waits for an event behind it -- behind the front round's gs_blend_fwd -- reads
 * GS_ROUND_LIVE from plain memory and does not enqueue the back round at all when the front round left no tile live (the eager
 * seam; a captured step cannot branch on the host and lets the back round's kernels return at once instead). */
int gs_round_status(void* stream, const int64_t* rounds_dev, int64_t* status_host_mapped);

/* Publishes a guarded step's outcome without a copy or an event: one tiny launch writes
 * status[0..3] = info_dev[0..3] ({I, n_buckets, max tile, flags}), status[4] = applied_dev[0] (may be NULL) and -- walk_state
 * (gs_blend_fwd's, may be NULL) -- status[5] = storage units taken, status[6] = gradient rows: what the walk needed; status[7] =
 * tiles the front round of the step left live (under gs_rounds_set phase 3; -1 otherwise).
 * `status` may be page-locked HOST memory (hipHostMalloc'ed, device-accessible): the host then polls plain memory
 * -- the flags are sticky and the applied-step counter monotonic, so a torn read is harmless.
 * loss_ring_dev (optional, with loss3_dev = gs_l1_ssim_fwd's out3): a device ring of ring_len x 3 floats; an APPLIED step
 * n (counted from 1) logs its {l1, 1-ssim, total} in slot (n-1) mod ring_len, a skipped step logs nothing. */
int gs_step_status(void* stream, const int64_t* info_dev, const int64_t* applied_dev, int64_t* status,
                   const float* loss3_dev, float* loss_ring_dev, int ring_len, const int32_t* walk_state);

/* Persistent workspace of both seams, the eager rasterization() and the captured train step (SURVEY.md section 8b "Ownership" /
 * "Sync"; replaces the ~25 per-call allocations a binding would otherwise make and lets the list stages be enqueued BEFORE the
 * list sizes have reached the host).  The layout below is the only description of these buffers: no caller sizes one itself.
 * gs_workspace_query: layout of every intermediate of one rasterization() call (or one train step) that does not escape to the
 * caller, for a call shape and a CAPACITY of intersections.  offsets[GS_WS_SLOTS]: byte offset of each buffer inside its arena (-1: not needed for
 * these flags); slots below GS_WS_LIST_FIRST live in the fixed arena (sized by C, N, image), those below GS_WS_WALK_FIRST in the
 * list arena (sized by cap_isects / coarse_cap: what is LISTED), the others in the walk arena (sized by cap_units / cap_rows:
 * what a training forward WALKS -- checkpoints, quadrant sublists, work units, gradient rows); arena_bytes[3] = bytes of the
 * three arenas.  Every offset is 256-byte aligned.
 * gs_workspace_bind: validates three caller-owned device arenas against a layout and zeroes the info block on `stream`; needed
 * once per (arena triple, layout) -- calls made under gs_guard_set_call leave nothing behind that the next call could trip over.
 * The caller keeps one triple per call in flight on a (device, stream) and hands the sub-pointers to the stage entry points
 * below; a call whose lists outgrow the capacity (info flags, see gs_guard_set) replaces the list arena only and repeats
 * gs_bin_count .. gs_blend_fwd; a training call whose walk outgrows cap_units / cap_rows replaces the walk arena only and repeats
 * gs_blend_fwd. */
#define GS_WS_INFO 0            /* int64[GS_INFO_WORDS]: the size record, see GS_INFO_* */
#define GS_WS_REC 1             /* f32 [C*N][12] */
#define GS_WS_BBOX 2            /* u32 [C*N][4] */
#define GS_WS_TILES_PER_GAUSS 3 /* i32 [C*N] */
#define GS_WS_CUM_TILES 4       /* i32 [C*N] */
#define GS_WS_COLORS_POST 5     /* f32 [C*N][3] */
#define GS_WS_ISECT_OFFSETS 6   /* i32 [C*tiles+1] */
#define GS_WS_BUCKET_OFFSETS 7  /* i32 [C*tiles+1] */
#define GS_WS_TILE_ORDER 8      /* i32 [C*tiles] */
#define GS_WS_QCNT 9            /* i32 [C*tiles*4]              (training) */
#define GS_WS_SH_JAC 10         /* f32 [C*N*9]                  (training: gs_project_fwd -> gs_project_bwd) */
#define GS_WS_LIST_FIRST 11     /* ---- list arena ---- */
#define GS_WS_BIN 11            /* gs_bin_workspace_bytes / gs_bins_workspace_bytes */
#define GS_WS_COARSE_KEYS 12    /* u64 [coarse_cap]             (two-level binning) */
#define GS_WS_KEYS_TMP 13       /* u64 [cap]                    (per-tile pipeline) */
#define GS_WS_SLOT_GID 14       /* i32 [cap]                    (per-tile pipeline, training) */
#define GS_WS_FLATTEN_IDS 15    /* i32 [cap] */
#define GS_WS_SLOTS_BUF 16      /* i32 [cap]                    (training) */
#define GS_WS_ISECT_IDS_BUF 17  /* i64 [cap]                    (GS_WS_ISECT_IDS) */
#define GS_WS_QMASK 18          /* u8  [cap]                    (training) */
#define GS_WS_ROW_BASE 19       /* i32 [cap / 16 + 2]           (training) */
#define GS_WS_WALK_STATE 20     /* i32 [gs_walk_state_ints(cap)] (training: counters of the walk + scan descriptors) */
#define GS_WS_WALK_FIRST 21     /* ---- walk arena (training) ---- */
#define GS_WS_CKPT 21           /* f32 [cap_units][64][4] */
#define GS_WS_QLIST 22          /* i32 [cap_units][32][2] */
#define GS_WS_UNIT_DESC 23      /* i32 [cap_units][4] */
#define GS_WS_ROWS 24           /* f32 [cap_rows][12]           (gs_blend_bwd -> gs_project_bwd) */
#define GS_WS_SLOTS 25
#define GS_WS_TRAIN 1           /* flags: the backward's lists, checkpoints and rows */
#define GS_WS_TWO_LEVEL 2       /*        two-level binning (coarse_cap, bin_shift) instead of the per-tile pipeline */
#define GS_WS_ISECT_IDS 4       /*        gsplat's isect_ids written eagerly */
int gs_workspace_query(int C, int64_t N, int width, int height, int64_t cap_isects, int64_t coarse_cap, int64_t cap_units,
                       int64_t cap_rows, int bin_shift, int flags, int64_t* offsets, int64_t* arena_bytes);
int gs_workspace_bind(void* stream, void* fixed_base, int64_t fixed_bytes, void* list_base, int64_t list_bytes,
                      void* walk_base, int64_t walk_bytes, const int64_t* offsets, const int64_t* arena_bytes);

/* Number of Gaussian groups per camera used by the binning kernels, and the bytes of scratch
 * `workspace` gs_bin_count / gs_bin_emit_sort need for (C, N, tiles). */
int gs_bin_groups(int64_t N);
size_t gs_bin_workspace_bytes(int C, int64_t N, int tile_w, int tile_h);

/* P-fwd + SH-fwd fused (replaces gsplat fully_fused_projection + spherical_harmonics +
 * clamp_min(rgb+0.5, 0); call site /root/reference/model/gaussian.py:353-367).
 * sh_degree 0..4 (gsplat's range) with (sh_degree+1)^2 <= K <= 25, the same for every SH entry point below
 * (gs_project_bwd, gs_project_bwd_adam[_reg], gs_sh_grad_views, gs_sh_adam_views; gs_refine_apply: 1 <= K <= 25).
 * sh_degree >= 0: `colors_in` is shs[N,K,3] and sh_rest is NULL, or -- the reference model's own
 * parameter layout (/root/reference/model/gaussian.py:49-50, cat at :105-107) -- `colors_in` is
 * sh_0[N,1,3] and `sh_rest` is [N,K-1,3] (no concatenated copy is ever made).
 * sh_degree < 0: `colors_in` is already post-activation colour, [N,3] (colors_per_camera=0) or
 * [C,N,3] (=1); sh_rest is ignored.
 * Outputs: radii[C,N] i32 (0 = culled), means2d[C,N,2], depths[C,N], conics[C,N,3],
 * colors_out[C,N,3], rec[C*N*12] (mx, my, A*log2e/2, B*log2e | C*log2e/2, opacity, ext_x, ext_y |
 * r, g, b, 0: conic pre-scaled for exp2, opacity-aware half extents in pixels),
 * bbox[C*N*4] u32 (x0 | x1<<16, y0 | y1<<16: tile rectangle, min inclusive / max exclusive;
 * row-major tile bit mask for rectangles of <= 32 tiles; tile count),
 * tiles_per_gauss[C,N] i32.
 * tile_culling: 0 = gsplat's 3-sigma square (A.3; lists identical to the reference's), 1 = that
 * rectangle intersected with the opacity-aware extent and, for footprints of <= 32 tiles, an exact
 * ellipse-vs-tile test (tiles in which no pixel can reach alpha >= 1/255 are dropped; the rendered
 * image and all gradients are unchanged).
 * rect_ref[C*N*2] u32 (optional, may be NULL; written by stages 0 and 1): gsplat's 3-sigma tile rectangle itself (x0 | x1<<16,
 * y0 | y1<<16; 0 for culled Gaussians) whatever tile_culling did to bbox -- with tile_culling = 1 the caller can render from
 * the short lists and still build gsplat's exact list arrays (a function of this rectangle and `depths`) when somebody reads them.
 * stage: 0 = everything; 1 = geometry only (all outputs except colors_out and the colour quad of
 * rec); 2 = colour only, for the Gaussians a previous stage-1 call marked visible in radii.  Calling
 * 1, then the gs_bin_count kernels, then 2 lets the colour pass overlap the host read-back of I.
 * sh_jac[C*N*9] (optional, may be NULL; written by stages 0 and 2 for visible Gaussians when sh_degree >= 1; opaque to the
 * caller): the 3 x 3 Jacobian d(pre-clamp colour)/d(unit view direction), eight entries as [C*N][8] and the ninth as a plane
 * [C*N] behind them.  Handed to gs_project_bwd /
 * gs_project_bwd_adam it makes the backward independent of the SH coefficients: v_sh = Y(u) (x) v_pre, and the direction
 * term of v_means is sh_jac^T v_pre -- the backward then never streams the 48 coefficients per Gaussian. */
int gs_project_fwd(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                   const float* quats, const float* scales, const float* opacities,
                   const float* colors_in, const float* sh_rest, int colors_per_camera,
                   const float* viewmats, const float* Ks, int width, int height, float eps2d,
                   float near_plane, float far_plane, float radius_clip, int tile_culling, int stage, int activations,
                   int32_t* radii,
                   float* means2d, float* depths, float* conics, float* colors_out, float* rec, uint32_t* bbox,
                   int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac);

/* I-count (replaces the counting half of gsplat isect_tiles + its cumsum and
 * isect_offset_encode).  Writes isect_offsets[C*tiles+1] (exclusive; last = I),
 * bucket_offsets[C*tiles+1] (exclusive scan of ceil(count/64)), info_dev[4] =
 * {I, n_buckets, max entries in one tile, 0}.  If info_host != NULL the four values are copied
 * there and the stream is synchronised (the one host sync of the exact mode).
 * tile_order[C*tiles] (optional, may be NULL): a launch order for gs_blend_fwd, tiles with the longest
 * lists first (a permutation of 0 .. C*tiles-1; the order among lists of similar length is arbitrary). */
int gs_bin_count(void* stream, int C, int64_t N, int tile_w, int tile_h, const uint32_t* bbox,
                 void* workspace, size_t workspace_bytes, int32_t* isect_offsets,
                 int32_t* bucket_offsets, int32_t* tile_order, int64_t* info_dev, int64_t* info_host);

/* I-emit + per-tile depth sort (replaces the emitting half of isect_tiles and the global
 * cub::DeviceRadixSort).  Needs the workspace as left by gs_bin_count and consumes it (the sort's work-list counters
 * are zeroed by the count): one gs_bin_emit_sort per gs_bin_count, in that order.  keys_tmp[I] u64 and
 * slot_gid[I] i32 are scratch.  Outputs: cum_tiles[C*N] (exclusive scan of tiles_per_gauss =
 * first gradient-row slot of each flatten id), isect_ids[I] i64 (cam | tile | depth bits, sorted; may be NULL: it is
 * a function of the other outputs -- cam | tile from isect_offsets, depth bits from depths[flatten_ids] -- and half of the list bytes),
 * flatten_ids[I] i32 (sorted), slots[I] i32 (gradient-row slot of each sorted entry).  Inference lists: pass slot_gid =
 * slots = NULL -- the keys then carry the flatten id itself (no slot map is written or gathered; same order). */
int gs_bin_emit_sort(void* stream, int C, int64_t N, int tile_w, int tile_h, const uint32_t* bbox,
                     const float* depths, void* workspace, size_t workspace_bytes,
                     const int32_t* isect_offsets, int64_t n_isects, int64_t max_tile_count,
                     uint64_t* keys_tmp, int32_t* slot_gid, int32_t* cum_tiles, int64_t* isect_ids,
                     int32_t* flatten_ids, int32_t* slots);

/* Two-level binning: the same outputs as gs_bin_count + gs_bin_emit_sort (bit for bit), built differently.  A bin is
 * 2x2 (bin_shift 1) or 4x4 (2) tiles (0: the library picks from N and the tile grid).  gs_bins_count emits every
 * Gaussian into the bins its tile rectangle touches as a (depth bits << 32 | flatten id) key -- I' entries, 1.4-17 per
 * Gaussian where the tile lists hold 3-190 --, depth-sorts each bin's list in LDS, and counts each tile's entries out
 * of its bin's sorted list; gs_bins_lists repeats that walk and writes the per-tile lists by ordered compaction (ballot
 * + popcount: no atomics, no second sort; depth and tie order are inherited from the bin).  The per-tile pipeline sorts
 * I entries, this one I'; it pays from ~6 tile-list entries per Gaussian upwards (real captures: tens to hundreds).
 *   coarse_keys[coarse_cap] u64   scratch for the bin lists (kept between the two calls)
 *   coarse_list_cap               longest bin list the sort classes launched must take (<= 0: launch every class)
 *   info_dev[GS_INFO_WORDS]       the size record (GS_INFO_*)
 *                                 flags: 1 I > guard capacity | 4 I' > coarse_cap | 8 a bin list > coarse_list_cap;
 *                                 with flags != 0 nothing was emitted: repeat gs_bins_count with the sizes reported
 *   cum_tiles[C*N]                exclusive scan of tiles_per_gauss (first gradient-row slot of each flatten id)
 *   isect_ids                     may be NULL (see gs_bin_emit_sort)
 * workspace: gs_bins_workspace_bytes(C, N, tile_w, tile_h, bin_shift, coarse_cap), same arguments in both calls.
 * If info_host != NULL the eight values are copied there and the stream is synchronised. */
size_t gs_bins_workspace_bytes(int C, int64_t N, int tile_w, int tile_h, int bin_shift, int64_t coarse_cap);
int gs_bins_count(void* stream, int C, int64_t N, int tile_w, int tile_h, int bin_shift, const uint32_t* bbox,
                  const float* depths, void* workspace, size_t workspace_bytes, uint64_t* coarse_keys,
                  int64_t coarse_cap, int64_t coarse_list_cap, int32_t* cum_tiles, int32_t* isect_offsets,
                  int32_t* bucket_offsets, int32_t* tile_order, int64_t* info_dev, int64_t* info_host);
int gs_bins_lists(void* stream, int C, int64_t N, int tile_w, int tile_h, int bin_shift, const uint32_t* bbox,
                  void* workspace, size_t workspace_bytes, const uint64_t* coarse_keys, int64_t coarse_cap,
                  const int32_t* cum_tiles, const int32_t* isect_offsets, int64_t* isect_ids, int32_t* flatten_ids,
                  int32_t* slots, const int64_t* info_dev);

/* B-fwd (replaces gsplat rasterize_to_pixels forward).  backgrounds[C,3] may be NULL.
 * Outputs render_colors[C,H,W,3], render_alphas[C,H,W,1].  One wavefront per 16x16 tile, each
 * lane owning one pixel of each 8x8 quadrant.  Inference: pass ckpt = NULL (and NULL for every
 * list output).  Training (ckpt != NULL) additionally emits what gs_blend_bwd consumes -- sized by what the forward WALKS (a
 * saturated tile abandons the rest of its list), not by what is listed:
 *   qcnt[C*tiles*4]     lengths of the four compacted, depth-ordered quadrant sublists of every tile
 *   unit_desc[cap_units*4] i32   one work unit per GS_UNIT entries of a sublist: (tile*4+quadrant, position of the unit in its
 *                       sublist, storage unit, 0), dense in [0, walk_state[GS_WALK_UNITS])
 *   ckpt[cap_units*64*4] f32     row `storage unit`: the quadrant's 64 pixel states in front of the unit (T -- negative once
 *                       saturated / outside the image -- and accumulated rgb)
 *   qlist[cap_units*32*2] i32    block `storage unit`: the unit's (flatten id, gradient-row slot) pairs
 *   qmask[n_isects] u8  by gradient-row slot: which quadrant rows of an intersection exist.  Cleared by this call (one
 *                       streaming pass), then only the non-zero masks are stored: a scattered one-byte
 *                       store leaves L2 as a 32-byte partial write (profiles/r03_traffic_calibration.json)
 *   row_base[n_isects/16+2] i32  exclusive scan of popcount(qmask) over the slots, sampled every 16 slots (three small launches
 *                       behind the blend): rows_before(s) = row_base[s / 16] + popcount of the masks of slots [16 (s / 16), s);
 *                       the gradient rows of slot s are rows [rows_before(s), rows_before(s + 1)), in quadrant order -- the
 *                       rows of a Gaussian (contiguous slots) and of consecutive Gaussians are contiguous
 *   walk_state[gs_walk_state_ints(n_isects)] i32   counters (GS_WALK_*) and the scan's chunk counts; cleared by this call.
 * Storage units are taken in chunks of 8 per tile from GS_WALK_RANGES counters (a tile's launch slot picks one), each over its
 * own 1/32 of [0, cap_units).  When a range runs out -- the walk needs more than cap_units units, give or take the imbalance -- or
 * leaves more than cap_rows rows, the call is void: GS_FLAG_UNITS / GS_FLAG_ROWS are ORed into walk_state[GS_WALK_FLAGS] and
 * into the step guard's flag word (gs_guard_set), and walk_state[GS_WALK_STORAGE] / [GS_WALK_ROWS] hold what was needed
 * (render_colors / render_alphas are complete either way).  qmask / row_base 16-byte aligned; cap_units >= 256.
 * Inside the forward a pixel's state is one float: T in (1e-4, 1] = live; a finished pixel (stop rule fired / outside the image)
 * carries its final transmittance scaled by 2^64 (exact in fp32; "live" is T <= 1).  Checkpoints do NOT store that form: a live
 * pixel's checkpoint holds T, a finished one holds -1 (gs_blend_bwd looks at the sign only; the final T of a finished pixel comes
 * from render_alphas). */
size_t gs_walk_state_ints(int64_t n_isects);
int gs_blend_fwd(void* stream, int C, int width, int height, const float* rec,
                 const float* backgrounds, const int32_t* isect_offsets, const int32_t* tile_order,
                 const int32_t* flatten_ids, const int32_t* slots, int64_t n_isects, float* render_colors,
                 float* render_alphas, float* ckpt, int32_t* qlist, int32_t* qcnt, uint8_t* qmask,
                 int32_t* unit_desc, int64_t cap_units, int32_t* row_base, int64_t cap_rows, int32_t* walk_state);

/* B-bwd (replaces rasterize_to_pixels backward incl. absgrad).  Gaussian-parallel: eight 8-lane
 * systolic pipelines per wavefront, one GS_UNIT-entry work unit each; no atomics.  Writes one
 * 12-float row per (intersection, quadrant) some pixel took, at rows[(row_base[slot] + rank of the quadrant among the slot's
 * rows)*12]: (v_mx, v_my, |v_mx|, |v_my|, v_A, v_B, v_C, v_opacity, v_r, v_g, v_b, 0); rows[cap_rows*12].
 * The launch covers cap_units work units (pipelines past walk_state[GS_WALK_UNITS] return at once).  v_render_alphas may be NULL.
 * unit_classes (may be NULL): scratch of gs_unit_classes_ints(cap_units, C, width, height) int32, 16-byte aligned.  With it the
 * call first groups the published units by FILL CLASS -- the last unit of a quadrant sublist is part-filled; units of at most 8 /
 * 16 / 24 entries run 1 / 2 / 3 entries per lane instead of 4 -- and every wave takes eight units of one class.  Same rows,
 * bit for bit (a unit writes rows of its own; the order units run in decides nothing). */
size_t gs_unit_classes_ints(int64_t cap_units, int C, int width, int height);
int gs_blend_bwd(void* stream, int C, int width, int height, const float* rec,
                 const int32_t* qlist, const int32_t* qcnt, const int32_t* unit_desc, int64_t cap_units,
                 const float* ckpt, const uint8_t* qmask, const int32_t* row_base, const int32_t* walk_state,
                 const float* render_colors, const float* render_alphas, const float* v_render_colors,
                 const float* v_render_alphas, float* rows, int32_t* unit_classes);

/* Colour features of 1 .. 4 channels (gsplat's colors[N,D] / [C,N,D] with sh_degree = None; channels = D).  The record's colour
 * quad (floats 8..11) and the gradient row's colour quad (floats 8..11) carry up to four channels, zero above D; channels = 3 is
 * gs_blend_fwd / gs_blend_bwd itself.  A call sequence:
 *   forward   gs_project_fwd(sh_degree = -1, stage = 1), gs_rec_colors, the list stages, gs_blend_fwd_ch
 *   backward  gs_blend_bwd_ch, gs_project_bwd(sh_degree = -1, colors_per_camera = 1, v_colors = [C*N*3] scratch) for the geometry
 *             gradients, gs_channel_grads for v_colors
 * Depth rounds are 3-channel only (tile_state holds T, r, g, b): these entry points refuse gs_rounds_set phases other than 0.
 * Every entry point checks channels in {1, 2, 3, 4} and its pointers before it launches anything.
 * gs_rec_colors: rec[C*N*12] floats 8..11 = colors[D] of the Gaussians with radii > 0 (colors[N,D], or [C,N,D] with
 *   colors_per_camera = 1), no clamp; everything else in rec is left as gs_project_fwd(stage = 1) wrote it.
 * gs_blend_fwd_ch: gs_blend_fwd with backgrounds[C,D] (may be NULL) and render_colors[C,H,W,D].  channels = 4 in training mode also
 *   needs ckpt_ext[cap_units*64] f32 (the fourth channel's accumulated value in front of each work unit; the same cap_units as ckpt);
 *   NULL otherwise.
 * gs_blend_bwd_ch: gs_blend_bwd with render_colors / v_render_colors [C,H,W,D]; rows' floats 8..8+D = the channel gradients (zero
 *   above D).  channels = 4 needs the forward's ckpt_ext.
 * gs_channel_grads: v_colors[N,D] (summed over the cameras in camera order) or [C,N,D] (colors_per_camera = 1) = the sums of the
 *   colour quads of each Gaussian's rows (gathered as gs_project_bwd gathers them); zero for culled Gaussians.  Honours the step
 *   guard. */
int gs_rec_colors(void* stream, int C, int64_t N, int channels, const float* colors, int colors_per_camera, const int32_t* radii,
                  float* rec);
int gs_blend_fwd_ch(void* stream, int C, int width, int height, int channels, const float* rec,
                    const float* backgrounds, const int32_t* isect_offsets, const int32_t* tile_order,
                    const int32_t* flatten_ids, const int32_t* slots, int64_t n_isects, float* render_colors,
                    float* render_alphas, float* ckpt, int32_t* qlist, int32_t* qcnt, uint8_t* qmask,
                    int32_t* unit_desc, int64_t cap_units, int32_t* row_base, int64_t cap_rows, int32_t* walk_state,
                    float* ckpt_ext);
int gs_blend_bwd_ch(void* stream, int C, int width, int height, int channels, const float* rec,
                    const int32_t* qlist, const int32_t* qcnt, const int32_t* unit_desc, int64_t cap_units,
                    const float* ckpt, const uint8_t* qmask, const int32_t* row_base, const int32_t* walk_state,
                    const float* render_colors, const float* render_alphas, const float* v_render_colors,
                    const float* v_render_alphas, float* rows, int32_t* unit_classes, const float* ckpt_ext);
int gs_channel_grads(void* stream, int C, int64_t N, int channels, int colors_per_camera, const int32_t* radii,
                     const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                     const uint8_t* qmask, float* v_colors);

/* Colour features of more than four channels (colors[N,D] / [C,N,D], D >= 5): rendered in chunks of four channels -- [0,4), [4,8),
 * ... and a tail of 1 .. 3 -- over ONE projection and ONE set of tile lists, through the 1 .. 4 channel blend above.  A chunk is
 * (first, count): first a multiple of 4, 1 <= count <= 4, first + count <= D.  A call sequence:
 *   forward   gs_project_fwd(sh_degree = -1, stage = 1), the list stages; per chunk: gs_rec_colors_chunk, gs_blend_fwd_ch(count)
 *             into a dense [C,H,W,count] image, gs_chunk_scatter into [C,H,W,D].  Only a chunk blended in training mode leaves a
 *             walk (checkpoints, sublists, row bases), and a walk is valid with the checkpoints of its own launch alone.
 *   backward  per chunk: (gs_rec_colors_chunk + gs_blend_fwd_ch in training mode unless the walk at hand is this chunk's,)
 *             gs_chunk_gather of v_render_colors (and of the image), gs_blend_bwd_ch(count) -- v_render_alphas to ONE chunk, NULL
 *             to the others --, gs_rows_accumulate, gs_channel_grads_chunk; then gs_project_bwd(rows = the accumulator).
 * The row bases and quadrant masks depend on the footprints and alphas alone, so the rows of every chunk's backward are the same
 * rows.  Every entry point checks its chunk, its pointers (non-NULL; 4-byte aligned, 16-byte where whole quads move: rec, rows,
 * acc, qmask always, a D-wide or dense array when count = 4 and D is a multiple of 4) before it launches anything, and honours the
 * step guard -- gs_chunk_scatter / gs_chunk_gather its list flags alone: GS_FLAG_UNITS / GS_FLAG_ROWS, which the training blend in
 * front of a scatter raises, void the walk and not the image that launch completed.
 * gs_rec_colors_chunk: gs_rec_colors from channels [first, first + count) of colors[.., D]; the quad is zero above count.
 * gs_channel_grads_chunk: gs_channel_grads' sums (same order), stored to v_colors[.., D] at channels [first, first + count); the
 *   other channels are not touched.
 * gs_rows_accumulate: acc[n_rows*12] floats 0..7 of each row = (first_chunk ? 0 : acc) + rows; first_chunk also zeroes floats 8..11,
 *   which later calls leave alone.  rows and acc are two buffers.
 * gs_chunk_scatter: dst[p*D + first + k] = src[p*count + k]; gs_chunk_gather: dst[p*count + k] = src[p*D + first + k];
 *   p < n_pixels, k < count. */
int gs_rec_colors_chunk(void* stream, int C, int64_t N, int D, int first, int count, const float* colors, int colors_per_camera,
                        const int32_t* radii, float* rec);
int gs_channel_grads_chunk(void* stream, int C, int64_t N, int D, int first, int count, int colors_per_camera, const int32_t* radii,
                           const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                           const uint8_t* qmask, float* v_colors);
int gs_rows_accumulate(void* stream, int64_t n_rows, const float* rows, float* acc, int first_chunk);
int gs_chunk_scatter(void* stream, int64_t n_pixels, int D, int first, int count, const float* src, float* dst);
int gs_chunk_gather(void* stream, int64_t n_pixels, int D, int first, int count, const float* src, float* dst);

/* Row reduction + SH-bwd + P-bwd fused (replaces the atomics of the blend backward,
 * spherical_harmonics backward and fully_fused_projection backward).  Sums each Gaussian's rows
 * (slots [cum_tiles[f], cum_tiles[f]+tiles_per_gauss[f]) = rows [rows_before(first slot), rows_before(last slot + 1)): row_base + qmask) and
 * pushes the result through the colour and projection VJPs.  Outputs (all fully written):
 * v_means[N,3], v_quats[N,4], v_scales[N,3], v_opacities[N], v_colors: v_shs[N,K,3]
 * (sh_degree>=0; with the split layout v_colors is v_sh_0[N,1,3] and v_sh_rest[N,K-1,3]) or
 * v_colors[N,3]/[C,N,3]; v_means2d_abs[C,N,2] (the `.absgrad` side channel,
 * /root/reference/model/gaussian.py:191).
 * Optional (may be NULL): v_means2d[C,N,2], v_conics[C,N,3], v_colors_post[C,N,3] (gradient of the
 * post-clamp colour), v_colors_pre[C,N,3] (SH colours only: gradient of the pre-clamp colour, zero
 * for culled Gaussians).  With SH colours v_colors (and v_sh_rest) may be NULL: the SH-parameter
 * gradients are then left to gs_sh_grad_views / gs_sh_adam_views (fed by v_colors_pre from here or from
 * gs_row_sums).
 * activations != 0 (both directions): `scales` / `opacities` are the reference model's log-scales and
 * logit opacities (/root/reference/model/gaussian.py:98-103); exp / sigmoid are applied inside and
 * v_scales / v_opacities are gradients w.r.t. those raw parameters.  0 = gsplat's contract.
 * sh_jac (optional, may be NULL): gs_project_fwd's direction Jacobian of the same inputs; with it colors_in / sh_rest are not
 * read (same gradients to rounding: the direction term of v_means is then summed as J^T v_pre instead of per coefficient).
 * row_sums[C*N][12] (optional, may be NULL): the row sums gs_row_sums left -- rows / row_base / qmask are then not read (may be NULL);
 * same results bit for bit.  stat_grad_norm[N] / stat_count[N] (optional, both or neither; C = 1): this view's two additive
 * statistics of /root/reference/model/gaussian.py:188-197, WRITTEN not accumulated -- |absgrad|_2 * max(width, height) and 1 for
 * visible Gaussians, 0 for culled ones (the segments of the view-parallel step's SUM all-reduce, see gs_pack_view_step). */
int gs_project_bwd(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                   const float* quats, const float* scales, const float* colors_in,
                   const float* sh_rest, int colors_per_camera, const float* viewmats,
                   const float* Ks, int width, int height, float eps2d, float near_plane, float far_plane,
                   const int32_t* radii, const float* colors_post, const int32_t* tiles_per_gauss,
                   const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                   float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                   float* v_colors, float* v_sh_rest, float* v_means2d_abs, float* v_means2d,
                   float* v_conics, float* v_colors_post, float* v_colors_pre,
                   const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                   float* stat_grad_norm, float* stat_count);

/* gs_project_bwd plus the camera gradients (rasterization(_camera_grads=True)): the arguments and results of gs_project_bwd,
 * bit for bit (it is called inside), and from what it leaves per (camera, Gaussian) the gradient of the view matrices.  For
 * viewmats[c] = [[A, t], [0, 1]]:
 *   v_viewmats[C,4,4]: rows 0-2 = [v_A | v_t], v_t = sum_n v_pc, v_A = sum_n (v_pc mean^T + 2 v_covc A Sigma) over the camera's
 *     visible Gaussians (v_pc, v_covc: the camera-space gradients of the projection VJP); row 3 = 0.  The projection part only.
 *   v_campos[C,3]: the gradient of the camera centre inverse(viewmat)[:3,3] the SH colours look from (SH degree >= 1; zero
 *     otherwise) = minus the sum of the direction terms of v_means.  The caller carries it to the view matrix through the VJP
 *     of the 4x4 inverse (as gsplat's torch.inverse does) and adds it to v_viewmats.
 * v_means2d, v_conics and (SH degree >= 1) v_colors_post are NOT optional here: the camera terms are recomputed from them by a
 * kernel of its own, 15 fp64 values per visible Gaussian, reduced without atomics -- wave, block, one partial per block in
 * cam_partials[gs_cam_partials_doubles(C, N)] (fp64 scratch, 8-byte aligned, contents undefined before and after), then a
 * fixed-order sum per camera: two calls give the same bits.  Honours the step guard like gs_project_bwd. */
size_t gs_cam_partials_doubles(int C, int64_t N);
int gs_project_bwd_cam(void* stream, int C, int64_t N, int K, int sh_degree, const float* means,
                       const float* quats, const float* scales, const float* colors_in,
                       const float* sh_rest, int colors_per_camera, const float* viewmats,
                       const float* Ks, int width, int height, float eps2d, float near_plane, float far_plane,
                       const int32_t* radii, const float* colors_post, const int32_t* tiles_per_gauss,
                       const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                       float* v_means, float* v_quats, float* v_scales, float* v_opacities,
                       float* v_colors, float* v_sh_rest, float* v_means2d_abs, float* v_means2d,
                       float* v_conics, float* v_colors_post, float* v_colors_pre,
                       const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                       float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats,
                       float* v_campos);

/* Depth render modes (gsplat's render_mode "D", "ED", "RGB+D", "RGB+ED").  The depth of a (camera, Gaussian)
 * is gs_project_fwd's depths[C,N] (camera-space z); it is blended as ONE MORE colour channel, lane j = Dc of the record's colour
 * quad behind Dc = 0 .. 3 colour channels, by gs_blend_fwd (Dc + 1 == 3) or gs_blend_fwd_ch, whose background for that channel is
 * 0.  A call sequence ("RGB+D" with SH colours: j = 3; "D": j = 0 behind gs_project_fwd(stage = 1)):
 *   forward   gs_project_fwd [, gs_rec_colors], gs_rec_depth, the list stages, the blend at Dc + 1 channels [, gs_expected_depth_fwd]
 *   backward  [gs_expected_depth_bwd,] the blend backward, gs_project_bwd / gs_project_bwd_cam [, gs_channel_grads(channels = Dc)],
 *             gs_depth_grads
 * One depth round only: gs_rec_depth and gs_depth_grads refuse gs_rounds_set phases other than 0.  Every entry point checks its
 * lane / channel range, its pointers and their alignment before it launches anything.
 * gs_rec_depth: rec[C*N*12] float 8 + lane = depths[f] for the Gaussians with radii > 0; lane = 0 writes the whole quad (z, 0, 0, 0)
 *   -- the geometry-only projection leaves it unwritten --, lanes 1..3 that float alone.  rec 16-byte aligned.
 * gs_depth_grads (behind gs_project_bwd / gs_project_bwd_cam): v_z of each (camera, Gaussian) = the sum of float 8 + lane of its
 *   gradient rows (gathered as gs_channel_grads gathers them: fixed order, no atomics); v_means[N,3] += v_z * viewmats[c][2][0:3] in
 *   camera order; v_depths[C,N] (optional, may be NULL) = v_z, 0 for culled Gaussians.  With v_viewmats[C,4,4] and cam_partials
 *   (both or neither; cam_partials: gs_depth_partials_doubles(C, N) doubles of scratch, 8-byte aligned, contents undefined before and
 *   after) the depth's dependence on the view matrix is ADDED to what gs_project_bwd_cam wrote: v_viewmats[c][2][0:3] += sum_n v_z
 *   means[n], v_viewmats[c][2][3] += sum_n v_z -- fp64 partials per block, one block per camera adding them in a fixed order, only
 *   the final sums rounded to fp32: two calls give the same bits.  rows / qmask 16-byte aligned.  Honours the step guard.
 * gs_expected_depth_fwd: out_colors[n_pixels][channels] = acc_colors with its LAST channel divided by max(alphas[p], 1e-10) (torch's
 *   clamp(min = 1e-10); an uncovered pixel yields 0); the other channels are copied.
 * gs_expected_depth_bwd: the VJP of that: v_colors = v_out with its last channel divided by max(alpha, 1e-10); v_alphas[p] =
 *   v_alphas_in[p] (may be NULL: 0) - v_out[last] * acc[last] / alpha^2 where alpha >= 1e-10 (equality included, as torch's clamp
 *   backward), + 0 below.  (v_colors, v_alphas) are what the blend backward takes, acc_colors what the blend forward wrote.
 *   Images of 2 / 4 channels are read as 8- / 16-byte pixels and must be aligned so. */
int gs_rec_depth(void* stream, int C, int64_t N, int lane, const float* depths, const int32_t* radii, float* rec);
size_t gs_depth_partials_doubles(int C, int64_t N);
int gs_depth_grads(void* stream, int C, int64_t N, int lane, const float* means, const float* viewmats, const int32_t* radii,
                   const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                   const uint8_t* qmask, float* v_means, float* v_depths, double* cam_partials, float* v_viewmats);
int gs_expected_depth_fwd(void* stream, int64_t n_pixels, int channels, const float* acc_colors, const float* alphas,
                          float* out_colors);
int gs_expected_depth_bwd(void* stream, int64_t n_pixels, int channels, const float* acc_colors, const float* alphas,
                          const float* v_out, const float* v_alphas_in, float* v_colors, float* v_alphas);

/* Row e (view sharding): the row sums of every Gaussian as a pass of its own, and from them everything another rank needs of
 * this view before the long projection backward runs.  row_sums[C*N][12] = the 11 sums gs_project_bwd forms first (same
 * function, same bits; 12th float 0; rows of culled Gaussians are left unwritten) -> gs_project_bwd(..., row_sums);
 * v_colors_pre[C*N*3] = the clamp-masked pre-clamp colour gradient (identical to gs_project_bwd's optional output);
 * radii_norm[C*N] (optional) = radius / max_hw, 0 for culled Gaussians; cam_out[16] (optional, C = 1) = a
 * copy of viewmats[0].  With v_colors_pre / radii_norm / cam_out pointing into one buffer [3N | N | 16] this launch fills a
 * rank's whole all-gather payload of the view-parallel step (gs_sh_adam_views).  Honours the step guard. */
int gs_row_sums(void* stream, int C, int64_t N, const int32_t* radii, const float* colors_post,
                const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                float* row_sums, float* v_colors_pre, float* radii_norm, float max_hw, const float* viewmats, float* cam_out);

/* Row e (view sharding): dense SH-parameter gradients of R views rebuilt from the per-view
 * pre-clamp colour gradients,  v_sh[n][k][:] = sum_r Y_k(dir(means[n], camera r)) * v_colors_pre[r][n][:]
 * (r ascending; the SH VJP of spherical_harmonics backward).  Ranks exchange
 * v_colors_pre[N,3] per view (12 B per Gaussian) instead of the 48 SH gradients (192 B).
 * viewmats[R,4,4]; output layout as gs_project_bwd: v_colors[N,K,3], or split v_colors = v_sh_0[N,1,3]
 * and v_sh_rest[N,K-1,3].  R <= 64. */
int gs_sh_grad_views(void* stream, int R, int64_t N, int K, int sh_degree, const float* means,
                     const float* viewmats, const float* v_colors_pre, float* v_colors,
                     float* v_sh_rest);

/* Row e (view sharding): gs_sh_grad_views + the SH half of gs_adam_step in one pass -- the dense SH gradient (192 B per
 * Gaussian at SH3) is never written or re-read.  payload: the all-gathered per-view records, view r at payload +
 * r * payload_stride floats: [3N pre-clamp colour gradients | N normalised radii | 16 floats of the view matrix] (what
 * gs_row_sums fills; payload_stride >= 4N + 16).  sh_0[N,1,3] / sh_rest[N,K-1,3] and their moments are updated in place with
 * g = grad_scale * sum_r Y(dir(means[n], camera r)) (x) v_colors_pre[r][n] (r ascending: bitwise identical replicas), Adam
 * arithmetic and bias corrections of gs_adam_step(step); max_radii[N] (optional) = max(max_radii, max_r radii[r]).
 * Same update bit for bit as gs_sh_grad_views followed by gs_adam_step over the two SH segments.  Honours the step guard. */
int gs_sh_adam_views(void* stream, int R, int64_t N, int K, int sh_degree, const float* means, const float* payload,
                     int64_t payload_stride, float* sh_0, float* sh_0_exp_avg, float* sh_0_exp_avg_sq, float* sh_rest,
                     float* sh_rest_exp_avg, float* sh_rest_exp_avg_sq, float lr_sh_0, float lr_sh_rest, float beta1, float beta2,
                     float eps, int64_t step, float grad_scale, float* max_radii);

/* ---- "next" row f-1: the loss that feeds v_render_colors ----
 * Fused L1 + (1 - SSIM) of /root/reference/model/gaussian.py:415-453 (torchmetrics SSIM:
 * 11x11 Gaussian window sigma 1.5, K1 0.01, K2 0.03, data_range 1, mean over the interior).
 * render / gt are [H,W,3]; mask [H,W] may be NULL (render := mask*gt + (1-mask)*render).
 * workspace holds gs_loss_workspace_floats(H,W) floats and carries the SSIM derivative maps from
 * the forward to the backward.  out3 = {l1, 1-ssim, (1-lambda)*l1 + lambda*(1-ssim)}.
 * v_total: device scalar d(loss)/d(out3[2]);  v_render[H,W,3] is fully written.
 * clamp_input != 0: `render` is the rasterizer's un-clamped image; torch.clamp(render, 0, 1) of
 * GaussianModel.forward (/root/reference/model/gaussian.py:368) and its backward are applied inside.
 * Sizes: height, width > 10 (the window), height * width <= 2^28, width <= 2^20 and height <= 2^24 (32-bit byte offsets, 24-bit row multiplies);
 * anything else is refused with GS_ERR_ARG before a launch. */
size_t gs_loss_workspace_floats(int height, int width);
int gs_l1_ssim_fwd(void* stream, int height, int width, float lambda_ssim, const float* render,
                   const float* gt, const float* mask, int clamp_input, float* workspace, float* out3);
int gs_l1_ssim_bwd(void* stream, int height, int width, float lambda_ssim, const float* render,
                   const float* gt, const float* mask, int clamp_input, const float* workspace,
                   const float* v_total, float* v_render);

/* The same two entries for a CAPTURED step (the graph's kernel arguments are frozen at capture, the image a step trains on is
 * not): ground truth and mask are read through device memory, slots_dev[0] = gt, slots_dev[1] = mask, which gs_step_inputs
 * writes in front of every replay.  has_mask (known at capture) selects the forward's instantiation; the backward tests the slot. */
int gs_l1_ssim_fwd_slots(void* stream, int height, int width, float lambda_ssim, const float* render,
                         const float* const* slots_dev, int has_mask, int clamp_input, float* workspace, float* out3);
int gs_l1_ssim_bwd_slots(void* stream, int height, int width, float lambda_ssim, const float* render,
                         const float* const* slots_dev, int clamp_input, const float* workspace,
                         const float* v_total, float* v_render);

/* ---- evaluation metrics: what the reference's eval.py:45-55 takes from torchmetrics per held-out view ----
 * render / gt are [H,W,3]; mask [H,W] may be NULL.  c = mask*gt + (1-mask)*render, with render clamped to [0,1] first when
 * clamp_input != 0.  out2 = {mse, ssim}: mse = the mean of (c - gt)^2 over all H*W*3 elements (PeakSignalNoiseRatio(data_range=1.0)
 * is 10 log10(1 / mse); a float data_range does not clamp), ssim = the mean SSIM over the (H-10) x (W-10) interior of the three
 * channels, the statement gs_l1_ssim_fwd uses (the mean itself, not 1 - ssim).  Forward only and without atomics: the same inputs
 * give the same bits (a NaN in a clamped render becomes 0, as in gs_l1_ssim_fwd).  workspace holds gs_metrics_workspace_floats(H,W) floats (two per launched block); every word of it that is
 * read is written by the same call.  Sizes as for gs_l1_ssim_fwd: anything else is refused with GS_ERR_ARG before a launch. */
size_t gs_metrics_workspace_floats(int height, int width);
int gs_image_metrics(void* stream, int height, int width, const float* render, const float* gt, const float* mask,
                     int clamp_input, float* workspace, float* out2);

/* ---- frame finishing: from a render to what a viewer shows or a video file holds, in one pass ----
 * render is the un-clamped blend output [H,W,cin], contiguous; out is [out_height,out_width,3] with the image top-left and every
 * other element zero (the reference's adjust_image_aspect, viewer/viewer_runtime.py:104-116).  gs_frame_finish writes EVERY
 * element of out: nothing has to clear it first.
 *   format GS_FRAME_F32: float, clamp(x, 0, 1) with torch.clamp's values (a NaN stays a NaN; -0 gives +0).
 *          GS_FRAME_U8:  packed RGB bytes floor(fl32(clamp(x, 0, 1) * 255)): one rounded float32 product, then floor
 *                        (RecordManager.export_video, viewer/utils.py:128-129); NaN gives 0, +inf gives 255.
 *   mode   GS_FRAME_RGB:   channels 0-2 of a render with cin = 3 or 4 (alpha, range2 and alpha_min are not looked at).
 *          GS_FRAME_DEPTH: channel cin - 1 of a render with cin = 4 (render_mode "RGB+D" / "RGB+ED") or 1 (a depth image), the
 *                        alpha image [H,W] and the DEVICE pair range2 = {lo, hi}.  A pixel whose alpha is not >= alpha_min is 0;
 *                        any other is g = 1 - clamp(t, 0, 1) on all three channels, t = (d - lo) / (hi - lo) in float32 and
 *                        t = 0 where hi == lo (near is bright); the format then applies to g.
 * gs_frame_range writes {lo, hi} = the min and max of that depth channel over the pixels with alpha >= alpha_min into range2
 * (device, [2]); NaN depths are skipped; {0, 0} when no pixel is covered.  Two stages over the caller's workspace of
 * gs_frame_workspace_floats(H, W) floats (every word read is written by the same call), fixed order, no atomics.
 * Refused with GS_ERR_ARG before a launch: null pointers, non-positive sizes, out smaller than the render, a cin the mode does
 * not take, an unknown mode or format, buffers that are not 16-byte aligned, and sizes whose byte counts (H*W*cin*4, the
 * output's) do not fit 31 bits.  Neither entry looks at the step guard. */
#define GS_FRAME_F32 0
#define GS_FRAME_U8 1
#define GS_FRAME_RGB 0
#define GS_FRAME_DEPTH 1
size_t gs_frame_workspace_floats(int height, int width);
int gs_frame_range(void* stream, int height, int width, int cin, const float* render, const float* alpha, float alpha_min,
                   float* workspace, float* range2);
int gs_frame_finish(void* stream, int height, int width, int cin, const float* render, int mode, int format,
                    const float* alpha, const float* range2, float alpha_min, int out_height, int out_width, void* out);

/* Row a-2: `torch.clamp(render, 0, 1)` of /root/reference/model/gaussian.py:368 as one pass.
 * v_out == NULL: out = clamp(x, 0, 1).  v_out != NULL: out = v_out where 0 <= x <= 1, else 0 (the
 * backward of that clamp).  n floats, 16-byte aligned buffers. */
int gs_clamp01(void* stream, int64_t n, const float* x, const float* v_out, float* out);

/* ---- "next" row f-2: fused Adam over flat buffers (one torch.optim.Adam with six groups in the
 * reference, /root/reference/model/gaussian.py:389-412; defaults: no weight decay / amsgrad).
 * params, exp_avg, exp_avg_sq: flat fp32 device buffers of n elements holding n_segments parameter
 * tensors back to back, each padded to a multiple of 4 elements.  HOST arrays per segment:
 * seg_ends_host (exclusive padded end), seg_lens_host (true element count), seg_grads_host (device
 * pointer of that tensor's contiguous, 16-byte aligned gradient; NULL = skip the segment, as torch
 * skips `p.grad is None`), seg_lrs_host.  step counts from 1.  Gradients are multiplied by
 * grad_scale first (1.0 = torch semantics; 1/world turns a sum over ranks into the mean). */
int gs_adam_step(void* stream, int64_t n, float* params, float* exp_avg, float* exp_avg_sq,
                 int n_segments, const int64_t* seg_ends_host, const int64_t* seg_lens_host,
                 const float* const* seg_grads_host, const float* seg_lrs_host, float beta1,
                 float beta2, float eps, int64_t step, float grad_scale);

/* The same step with two additive statistics riding along in the launch (the view-parallel step's geometry half, row e):
 * stat_dst0[i] += stat_src0[i], stat_dst1[i] += stat_src1[i] for i < stat_n -- the all-reduced |absgrad| norm and visibility
 * count of /root/reference/model/gaussian.py:188-197 into grad_norm_accum / collecting_counts.  stat_n = 0: exactly gs_adam_step.
 * (Both entry points walk only the segments that have a gradient.) */
int gs_adam_step_stats(void* stream, int64_t n, float* params, float* exp_avg, float* exp_avg_sq,
                       int n_segments, const int64_t* seg_ends_host, const int64_t* seg_lens_host,
                       const float* const* seg_grads_host, const float* seg_lrs_host, float beta1, float beta2,
                       float eps, int64_t step, float grad_scale, int64_t stat_n, const float* stat_src0,
                       const float* stat_src1, float* stat_dst0, float* stat_dst1);

/* Replayable form of gs_adam_step for a captured step: bias corrections and learning rates come from the device
 * array hyper_dev[1 + n_segments] = {1/sqrt(1-beta2^t), lr_k/(1-beta1^t)...}, which gs_adam_hyper writes (values
 * travel as kernel arguments of a one-thread launch, so successive steps cannot race on a host buffer).
 * applied_dev (optional): device counter incremented by every launch the step guard did not skip. */
int gs_adam_hyper(void* stream, int n_segments, const float* seg_lrs_host, float beta1, float beta2, int64_t step,
                  float* hyper_dev);
/* gs_adam_hyper + everything else that changes from one replay of a captured step to the next, in ONE launch (values travel
 * as kernel arguments): viewmat_dst[16] <- viewmat_src[16] and K_dst[9] <- K_src[9] (device pointers; a NULL source leaves
 * its destination alone), slots_dev[0] = gt, slots_dev[1] = mask (the POINTERS gs_l1_ssim_*_slots read through; slots_dev
 * may be NULL).  A step on another view costs no copy of its ground-truth image. */
int gs_step_inputs(void* stream, int n_segments, const float* seg_lrs_host, float beta1, float beta2, int64_t step,
                   float* hyper_dev, const float* viewmat_src, float* viewmat_dst, const float* K_src, float* K_dst,
                   const float* gt, const float* mask, const float** slots_dev);
int gs_adam_step_dev(void* stream, int64_t n, float* params, float* exp_avg, float* exp_avg_sq, int n_segments,
                     const int64_t* seg_ends_host, const int64_t* seg_lens_host, const float* const* seg_grads_host,
                     float beta1, float beta2, float eps, float grad_scale, const float* hyper_dev, int64_t* applied_dev);

/* gs_adam_step / gs_adam_step_dev over the Gaussians a step SAW (gsplat's visible_adam; DESIGN.md "Updating only what a step saw"):
 * every segment holds n_rows Gaussians, seg_widths_host[k] floats each (seg_lens_host[k] == n_rows * seg_widths_host[k]; width 0: an
 * empty segment), and radii[n_rows] (device, int32) is the step's projection verdict.  A Gaussian with radii > 0 receives the update
 * of the dense step, same arithmetic and bias corrections; one with radii <= 0 keeps the bits of its parameters and of both moments
 * whatever its gradient holds (it is not read).  A 16-byte quad none of whose Gaussians is visible is neither loaded nor stored; the
 * pad behind a segment is never written.  n == 0 or n_rows == 0: nothing to do.  Honour the step guard like their dense forms. */
int gs_adam_step_visible(void* stream, int64_t n, float* params, float* exp_avg, float* exp_avg_sq,
                         int n_segments, const int64_t* seg_ends_host, const int64_t* seg_lens_host,
                         const float* const* seg_grads_host, const float* seg_lrs_host, float beta1,
                         float beta2, float eps, int64_t step, float grad_scale, int64_t n_rows,
                         const int64_t* seg_widths_host, const int32_t* radii);
int gs_adam_step_visible_dev(void* stream, int64_t n, float* params, float* exp_avg, float* exp_avg_sq, int n_segments,
                             const int64_t* seg_ends_host, const int64_t* seg_lens_host, const float* const* seg_grads_host,
                             float beta1, float beta2, float eps, float grad_scale, const float* hyper_dev, int64_t* applied_dev,
                             int64_t n_rows, const int64_t* seg_widths_host, const int32_t* radii);

/* ---- "next" row f-3: densify / prune on the device (/root/reference/model/gaussian.py:199-349) ----
 * gs_refine_flags: per Gaussian, the reference's decisions.  flags[3][n] (0/1): row 0 the old Gaussian survives the
 * prune (low opacity | max_radii > ratio | largest scale > prune_scale | it was split); row 1 it is split AND its
 * children survive (children: same opacity, scales / (0.8 S)); row 2 it is cloned AND the clone survives.
 * counters[5] (device, zeroed here) = {split, clone, then the reference's cumulative prune counts over [old | new]:
 * low opacity, + large radii, + large scale} -- what densify_and_prune returns as tb_info.
 * gs_refine_apply: given the INCLUSIVE prefix scans of the three flag rows (gs_scan_rows_i32) and
 * their totals (the one host read of the path: they size the new buffers), fills the new flat parameter / exp_avg /
 * exp_avg_sq buffers in the reference's order [surviving old | split children, copy-major | clones]: survivors keep
 * their moments, new Gaussians start at zero; split children get mean + R(q)(s * noise[copy][parent]) and
 * log(s / (0.8 S)).  Flat layout as gs_adam_step: the six tensors of param_names (means, log_scales, quats, sh_0,
 * sh_rest, logit_opacities) at old_offsets_host[6] / new_offsets_host[6] floats.  src_scratch[n_new] i32 and
 * tag_scratch[n_new] i8 are scratch.  noise: [S][n_old][3] standard normal. */
/* Inclusive prefix scan of every row of an int32 [rows][n] array.  workspace: gs_scan_rows_workspace_ints(rows, n) int32. */
size_t gs_scan_rows_workspace_ints(int rows, int64_t n);
int gs_scan_rows_i32(void* stream, int rows, int64_t n, const int32_t* in, int32_t* out, int32_t* workspace);
int gs_refine_flags(void* stream, int64_t n, int num_splits, float densify_grad_thresh, float densify_scale_thresh,
                    float prune_radii_ratio_thresh, float prune_scale_thresh, float min_opacity,
                    const float* grad_norm_accum, const float* counts, const float* max_radii, const float* log_scales,
                    const float* logit_opacities, int32_t* flags, int64_t* counters);
int gs_refine_apply(void* stream, int64_t n_old, int num_splits, int K, const int32_t* flags, const int32_t* flags_incl,
                    int64_t tot_old, int64_t tot_child, int64_t tot_clone, const float* noise, const float* old_params,
                    const float* old_exp_avg, const float* old_exp_avg_sq, const int64_t* old_offsets_host, float* new_params,
                    float* new_exp_avg, float* new_exp_avg_sq, const int64_t* new_offsets_host, int32_t* src_scratch,
                    int8_t* tag_scratch);

/* ---- training under a Gaussian budget: the MCMC densification (Kheradmand et al., 2024) on the flat Adam buffers ----
 * (csrc/gs_mcmc.hip; easy_gaussian_splatting_amd/mcmc.py; DESIGN.md "Training to a budget").  No entry allocates; n == 0 launches
 * nothing.
 * gs_mcmc_weights: o = sigmoid(logit) in fp64; dead[i] = !(o > min_opacity) (0 everywhere when grow = 1);
 * weights[i] = dead ? 0 : max(1, floor(o 2^24)).
 * gs_mcmc_cdf: inclusive prefix sum of the uint32 weights into int64 (exact, whatever the block order).
 * workspace: gs_mcmc_cdf_workspace_longs(n) int64.
 * gs_mcmc_sample: draw j takes t = mulhi64((uint64) bits[j], total), total = cdf[n-1], and src[j] = min{i : cdf[i] > t};
 * counts[n] (zeroed here) counts the draws per source.  Relocate (dead / dead_incl given, dead_incl the inclusive scan of dead by
 * gs_scan_rows_i32, n_slots == n, bits[n]): the number of draws is the dead total, read on the device; dst[rank] = i for the dead
 * Gaussians in index order.  Grow (dead = dead_incl = NULL): n_draws_host draws, dst[j] = n + j.  No draws when total == 0.
 * src[n_slots] / dst[n_slots] are -1 beyond what is written; n_draws_dev[1] receives the number of draws.
 * gs_mcmc_relocation_values: for R = clamp(ratio[i], 1, 51): o' = 1 - (1 - o)^(1/R), s' = s o / D,
 * D = sum_{i=1..R} sum_{k<i} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1), in fp64; opacities[n], scales[n][3], unclamped results.
 * gs_mcmc_apply: in place on the flat buffers of gs_adam_step (offsets_host[6]: means, log_scales, quats, sh_0, sh_rest,
 * logit_opacities; floats; rows 0 .. n_rows-1 exist in every segment).  First every Gaussian i < n with counts[i] > 0 gets the
 * values above for R = min(counts[i] + 1, 51), o' clamped to [min_opacity, 1 - 2^-23], stored as logit(o') and log(s'); then
 * every draw j < min(n_draws_dev[0], max_draws) copies its six parameter rows src[j] -> dst[j].  The Adam moments of every row
 * rewritten (sources and destinations, all six segments) restart at zero.
 * gs_mcmc_noise: means[i] += strength g(o_i) R(q_i) diag(s_i^2) R(q_i)^T z_i in fp64, one rounding at the store;
 * g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))), q normalised (wxyz), s = exp(log_scales), z[n][3] standard normal.
 * Every pointer 16-byte aligned (the segments of the flat buffers are). */
int gs_mcmc_weights(void* stream, int64_t n, const float* logit_opacities, double min_opacity, int grow, uint32_t* weights,
                    int32_t* dead);
size_t gs_mcmc_cdf_workspace_longs(int64_t n);
int gs_mcmc_cdf(void* stream, int64_t n, const uint32_t* weights, int64_t* cdf, int64_t* workspace);
int gs_mcmc_sample(void* stream, int64_t n, int64_t n_slots, const int64_t* cdf, const int64_t* bits, const int32_t* dead,
                   const int32_t* dead_incl, int64_t n_draws_host, int32_t* src, int32_t* dst, int32_t* counts,
                   int64_t* n_draws_dev);
int gs_mcmc_relocation_values(void* stream, int64_t n, const float* opacities, const float* scales, const int32_t* ratio,
                              float* new_opacities, float* new_scales);
int gs_mcmc_apply(void* stream, int64_t n, int64_t n_rows, int K, double min_opacity, const int32_t* src, const int32_t* dst,
                  const int32_t* counts, const int64_t* n_draws_dev, int64_t max_draws, float* params, float* exp_avg,
                  float* exp_avg_sq, const int64_t* offsets_host);
int gs_mcmc_noise(void* stream, int64_t n, double strength, const float* log_scales, const float* quats,
                  const float* logit_opacities, const float* z, float* means);

/* Counter-based noise, for the captured step (DESIGN.md "Training to a budget"): the normals of Gaussian n at optimizer step t
 * under a 64-bit seed are a pure function of (seed, t, n) -- one Philox4x32-10 block with counter (n lo, n hi, t lo, t hi) and key
 * (seed lo, seed hi), multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85 -- so a step the guard skipped
 * draws the same normals when it is replayed.  From the block's words x0..x3, in fp64: u_i = (x_i + 0.5) 2^-32,
 * z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1), z2 = sqrt(-2 ln u2) cos(2 pi u3), each rounded to float32
 * once: the z of gs_mcmc_noise.
 * gs_mcmc_normals: z_out[n][3] = those normals (16-byte aligned).
 * gs_mcmc_step_inputs: a one-thread launch that writes rec_dev[GS_MCMC_REC_WORDS] int64 (16-byte aligned) = {the bits of the
 * double `strength`, step, seed, 0}; the values travel as kernel arguments, as gs_adam_hyper's.
 * gs_mcmc_noise_step: gs_mcmc_noise with strength, step and seed read from rec_dev and the normals drawn in the kernel -- no z
 * array; the same means, bit for bit, as gs_mcmc_normals + gs_mcmc_noise.  Honours the step guard. */
#define GS_MCMC_REC_WORDS 4
int gs_mcmc_normals(void* stream, int64_t n, int64_t step, uint64_t seed, float* z_out);
int gs_mcmc_step_inputs(void* stream, double strength, int64_t step, uint64_t seed, int64_t* rec_dev);
int gs_mcmc_noise_step(void* stream, int64_t n, const int64_t* rec_dev, const float* log_scales, const float* quats,
                       const float* logit_opacities, float* means);

/* Budget regulariser (mcmc.MCMCStrategy.regularization): reg = a mean_N sigmoid(logit_n) + b mean_3N exp(log_scale_nk) over ALL N
 * Gaussians, o and s in fp64; d reg / d logit_n = fl32(a / N) o_n (1 - o_n) and d reg / d log_scale_nk = fl32(b / (3 N)) s_nk, each
 * rounded to float32 once.
 * gs_mcmc_reg: gs_scale_reg's contract -- reg_ws[gs_mcmc_reg_workspace_floats(N)] f32, 16-byte aligned, reg_ws[0] = reg, the rest
 *   scratch; loss3 (optional): loss3[2] += reg; v_logit_opacities[N] / v_log_scales[N*3] (each optional): += the gradient.  The
 *   sums run in a fixed order without float atomics (replays give the same bits).  Honours the step guard.  N = 0: no launch.
 * gs_project_bwd_adam_mcmc: gs_project_bwd_adam with both gradients added for every in-range Gaussian in front of the update (read
 *   from the parameters before it) -- behind the scale-ratio regulariser's when scale_reg = 1 (max_ratio, lambda as in
 *   gs_project_bwd_adam_reg).  Same update, bit for bit, as gs_project_bwd, [gs_scale_reg,] gs_mcmc_reg into its gradients,
 *   gs_adam_step_dev. */
size_t gs_mcmc_reg_workspace_floats(int64_t N);
int gs_mcmc_reg(void* stream, int64_t N, const float* logit_opacities, const float* log_scales, double a, double b, float* loss3,
                float* reg_ws, float* v_logit_opacities, float* v_log_scales);
int gs_project_bwd_adam_mcmc(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                             const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                             float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                             const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                             const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                             int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac,
                             int scale_reg, float max_ratio, float lambda, double a, double b);

/* gs_project_bwd + gs_adam_step_dev in one pass, for the reference's own single-camera step with the model's raw
 * parameters (log-scales, logit opacities, split SH: activations as in gs_project_bwd(..., activations = 1)): no
 * gradient is written; each parameter element and its two moments are updated in place where its gradient is
 * formed (saves writing and re-reading 59 floats per Gaussian).  params / exp_avg / exp_avg_sq and offsets_host[6]
 * (means, log_scales, quats, sh_0, sh_rest, logit_opacities; floats) describe the flat buffers of gs_adam_step.
 * Same update, bit for bit, as gs_project_bwd followed by gs_adam_step_dev.  Honours the step guard.
 * max_radii / grad_norm_accum / counts (optional, all three or none): gs_update_statistics is applied in the same pass.
 * sh_jac (optional): as in gs_project_bwd. */
int gs_project_bwd_adam(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                        const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                        float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                        const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask,
                        float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev, int64_t* applied_dev,
                        float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac);

/* Scale-ratio regulariser (the reference's use_scale_regularization / max_scale_ratio / lambda_scale): with s = exp(log_scales[n]),
 *   reg = mean over ALL N Gaussians (visible or not) of  max(max_k s_k / min_k s_k, max_ratio) - max_ratio,
 * and the loss gains lambda * reg.  Gradient w.r.t. the log-scales as torch autograd forms it in fp32: it passes where the ratio
 * is >= max_ratio (equality included), tied maxima / minima share their part evenly, upstream lambda * (1 / N).
 * gs_scale_reg: reg_ws[gs_scale_reg_workspace_floats(N)] f32, 16-byte aligned -- reg_ws[0] = reg, the rest is scratch; loss3
 *   (optional, {l1, 1 - ssim, total} of gs_l1_ssim_fwd*): loss3[2] += lambda * reg; v_log_scales[N*3] (optional): += the gradient.
 *   The sum runs in a fixed order without float atomics (replays give the same bits).  Honours the step guard.  N = 0: no launch.
 * gs_project_bwd_adam_reg: gs_project_bwd_adam with the regulariser's gradient added to every in-range Gaussian's log-scale
 *   gradient in front of the update (read from the parameters before it); the value comes from gs_scale_reg, called before it
 *   with v_log_scales = NULL.  Same update, bit for bit, as gs_project_bwd, gs_scale_reg into its v_scales, gs_adam_step_dev. */
size_t gs_scale_reg_workspace_floats(int64_t N);
int gs_scale_reg(void* stream, int64_t N, const float* log_scales, float max_ratio, float lambda, float* loss3, float* reg_ws,
                 float* v_log_scales);
int gs_project_bwd_adam_reg(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                            const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                            float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                            const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                            const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                            int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac,
                            float max_ratio, float lambda);

/* gs_project_bwd_adam (reg_on = 0) / gs_project_bwd_adam_reg (reg_on = 1) over the Gaussians the step SAW (DESIGN.md "Updating only
 * what a step saw"): a Gaussian with radii > 0 receives the update of the dense entry, bit for bit; one the camera culled keeps the
 * bits of its six parameters and of both moments, the regulariser's term included (it is not computed).  16-byte groups that hold
 * culled Gaussians only are neither loaded nor stored, and a block without a visible Gaussian skips its SH staging and both Adam
 * walks.  v_means2d_abs, the statistics, the step guard and applied_dev as in the dense entries.  Pinhole, classic mode, gradient
 * rows (no row-sums form), SH degrees 0-4. */
int gs_project_bwd_selective(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                             const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                             float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                             const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                             const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                             int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac,
                             int reg_on, float max_ratio, float lambda);

/* Row e: this rank's contribution to the SUM all-reduce of the view-parallel step in one pass: the four
 * geometry gradients and this view's two additive statistics (|absgrad|_2 * max_hw, visibility count)
 * packed into flat = [means 3N | log_scales 3N | quats 4N | logit_opacities N | grad_norm N | count N],
 * every segment padded to a multiple of 4 floats (flat holds 4*ceil(3N/4)*2 + 4N + 3*4*ceil(N/4) floats).
 * v_means = v_scales = v_quats = v_opacities = NULL: gs_project_bwd has written its four gradients into those segments of
 * `flat` itself (they are plain output pointers there); only the two statistics segments are filled in. */
int gs_pack_view_step(void* stream, int64_t n, float max_hw, const float* v_means, const float* v_scales,
                      const float* v_quats, const float* v_opacities, const int32_t* radii, const float* absgrad,
                      float* flat);

/* Row a-3: the consumer of the side channels, `GaussianModel.update_statistics`
 * (/root/reference/model/gaussian.py:188-197), as one launch for the reference's single camera:
 * for radii[i] > 0: max_radii = max(max_radii, radii/max_hw); grad_norm_accum += |absgrad[i]|_2 * max_hw;
 * counts += 1.  absgrad is [N,2]. */
int gs_update_statistics(void* stream, int64_t n, float max_hw, const int32_t* radii, const float* absgrad,
                         float* max_radii, float* grad_norm_accum, float* counts);

/* ---- initial scales: exact k-nearest-neighbour distances of a point cloud, what the reference's
 * constructor takes from sklearn's NearestNeighbors (/root/reference/model/utils.py:8-11; the original 3DGS code: distCUDA2) ----
 * points is [N][3] float32 in the caller's order; dists is [N][k] float32: row i holds the k smallest of { |p_i - p_j| : j != i }
 * in ascending order.  Self is excluded by INDEX, not by distance: coincident points are neighbours at exactly 0.0f, and no
 * floor is applied.  Exact: the Morton order and the boxes decide how fast the search goes, never what it returns -- a row is
 * the k smallest of sqrt(fl(fl(fl(dx dx) + dy dy) + dz dz)), dx = fl(x_i - x_j), whatever `order` is.  No atomics: the same
 * input gives the same bits.  Two stages with the caller's sort between them:
 *   gs_knn_codes   codes[N] int64 = the 63-bit Morton code (21 bits per axis) of each point inside the cloud's bounding box; an
 *                  axis of zero extent contributes 0.
 *   (the caller)   order[N] int32 = the point indices sorted by code, a permutation of 0..N-1 (an entry outside [0, N) is
 *                  skipped, never dereferenced; the points it should have named then miss from every row).
 *   gs_knn_dists   gathers the points in that order, boxes every GS_KNN_LEAF consecutive points (a leaf) and every GS_KNN_FANOUT
 *                  consecutive leaves, and searches: one lane per query, a box skipped when no lane of the wave is strictly
 *                  closer to it than to its k-th best so far.
 * workspace: gs_knn_workspace_bytes(N) bytes, 256-byte aligned, scratch (every word read is written by the same call; the two
 * stages of one cloud may share it or not); points, dists, codes and order need only their element alignment.
 * Everything runs on `stream` without a synchronisation.  Every loop runs to a count known before it starts: a NaN or an
 * infinity among the coordinates gives a meaningless row and nothing worse.
 * Refused with GS_ERR_ARG before a launch: k outside [1, GS_KNN_MAX_K], N < k + 1 (gs_knn_codes: N < 2), N > GS_KNN_MAX_N = 2^30
 * (positions in the padded sorted array and point indices are int32), null pointers, a misaligned workspace;
 * gs_knn_workspace_bytes returns 0 for an N outside [1, GS_KNN_MAX_N]. */
#define GS_KNN_LEAF 64            /* points per leaf = one wavefront of queries */
#define GS_KNN_FANOUT 64          /* leaves per node of the second level */
#define GS_KNN_MAX_K 8
#define GS_KNN_MAX_N 1073741824
size_t gs_knn_workspace_bytes(int64_t N);
int gs_knn_codes(void* stream, int64_t N, const float* points, void* workspace, int64_t* codes);
int gs_knn_dists(void* stream, int64_t N, int k, const float* points, const int32_t* order, float* dists, void* workspace);

/* ---- Pose refinement in the captured step (DESIGN.md "Poses in the captured step"): pose.CameraDeltas' per-view correction
 * delta = {omega[3], tau[3]}, viewmat = [[exp([omega]x), tau], [0, 1]] @ w2c, composed, differentiated and stepped on the device.
 * The math is csrc/gs_pose.h: closed-form Rodrigues in fp64 with series below theta = 0.1, every entry rounded to fp32 once;
 * delta == 0 gives w2c bit for bit.
 * gs_pose_step_inputs: a one-thread launch in front of a step (as gs_mcmc_step_inputs: the values travel as kernel arguments) that
 *   writes rec_dev[GS_POSE_REC_FLOATS] f32, 16-byte aligned = {raw w2c[16], lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step), the
 *   bits of the int32 view index, 0}.  The raw matrix: w2c_dev (device, 16 floats, read by the launch) or w2c_host (16 values, copied
 *   at the call) or neither -- the record keeps the one it holds.  0 <= view < n_views <= GS_POSE_MAX_VIEWS, step >= 1.
 * gs_pose_compose: viewmat_out[16] = the corrected matrix of the record's view from deltas[n_views][6]; in front of gs_project_fwd.
 * gs_cam_grad_sums: the camera gradients of gs_project_bwd_cam for C = 1 -- v_viewmats[16] (rows 0-2 = [v_A | v_t], row 3 = 0) and
 *   v_campos[3], the same kernels, the same fp64 fixed-order reduction through cam_partials[gs_cam_partials_doubles(1, N)] -- formed
 *   from the per-Gaussian row sums gs_row_sums leaves (row_sums[N][12]: floats 0-1 = v_means2d, 4-6 = v_conics, 8-10 = v_colors_post)
 *   in place of the gradient tensors, which a step that applies Adam inside its projection backward never writes.  Reads the
 *   parameters (activations as in gs_project_bwd; sh_rest: the split layout's coefficients 1.., needed with sh_degree >= 1 when
 *   sh_jac is NULL), so it runs BEFORE gs_project_bwd_adam* updates them.  Honours the step guard.
 * gs_project_bwd_adam_sums: gs_project_bwd_adam / _reg / _mcmc (scale_reg, budget: 0 or 1, with their parameters) fed from the same
 *   row_sums in place of rows / row_base / qmask -- the gradient rows are then walked once per step, by gs_row_sums.  The same
 *   update, bit for bit, as the row-walking entries.
 * gs_pose_adam: one launch behind it.  v_delta[6] = the chain from {v_viewmats, v_campos} to the view's 6-vector in fp64 (the
 *   camera centre's term through the general 3x3 inverse, the product with w2c, the left Jacobian of SO(3)), rounded to fp32 once
 *   and left readable; then Adam (gs_adam_step's arithmetic per element) over ALL n_views x 6 corrections with the gradient v_delta
 *   on the view's row and exactly 0 on every other row -- what torch.optim.Adam over the whole tensor does: idle rows decay their
 *   moments and move.  Honours the step guard: a voided step leaves deltas, moments and v_delta as they were. */
#define GS_POSE_REC_FLOATS 20
#define GS_POSE_REC_SS 16
#define GS_POSE_REC_ISBC2 17
#define GS_POSE_REC_VIEW 18
#define GS_POSE_MAX_VIEWS 1048576
int gs_pose_step_inputs(void* stream, int view, int n_views, const float* w2c_dev, const float* w2c_host, float lr, float beta1,
                        float beta2, int64_t step, float* rec_dev);
int gs_pose_compose(void* stream, int n_views, const float* rec_dev, const float* deltas, float* viewmat_out);
int gs_cam_grad_sums(void* stream, int64_t N, int K, int sh_degree, const float* means, const float* quats, const float* scales,
                     const float* sh_rest, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                     float near_plane, float far_plane, const int32_t* radii, const float* colors_post, int activations,
                     const float* sh_jac, const float* row_sums, double* cam_partials, float* v_viewmats, float* v_campos);
int gs_project_bwd_adam_sums(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                             const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                             float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                             const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* row_sums, float* v_means2d_abs,
                             float beta1, float beta2, float eps, const float* hyper_dev, int64_t* applied_dev, float* max_radii,
                             float* grad_norm_accum, float* counts, const float* sh_jac, int scale_reg, float max_ratio, float lambda,
                             int budget, double a, double b);
int gs_pose_adam(void* stream, int n_views, const float* rec_dev, float* deltas, float* exp_avg, float* exp_avg_sq,
                 const float* v_viewmats, const float* v_campos, float* v_delta, float beta1, float beta2, float eps);

/* ---- Per-view exposure compensation (DESIGN.md "Exposure in the captured step"): exposure.ExposureTable's learnable 3x4 colour
 * affine per training image, table[n_views][3][4] row-major = [A | b], applied to the UN-clamped render in front of the loss:
 * out[p] = A render[p] + b.  The math is csrc/gs_exposure.h (shared with the host tests), in fp32 with one fixed order of fused
 * multiply-adds per channel i:
 *     out_i = fma(A_i2, c_2, fma(A_i1, c_1, fma(A_i0, c_0, b_i)))
 * -- three roundings; at [I | 0] the input comes back exactly (a -0 as +0).  Images are [height][width][3] f32, 16-byte aligned.
 * gs_exposure_step_inputs: a one-thread launch in front of a step (as gs_pose_step_inputs: the values travel as kernel arguments)
 *   that writes rec_dev[GS_EXPOSURE_REC_FLOATS] f32, 16-byte aligned = {lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step), the bits
 *   of the int32 view index, 0}.  0 <= view < n_views <= GS_EXPOSURE_MAX_VIEWS and step >= 1: anything else is GS_ERR_ARG before
 *   any launch.
 * gs_exposure_apply: out = the affine of a view applied to render.  The view: the record's when rec_dev is non-NULL (the captured
 *   step), else `view` (eager).  out may not alias render.
 * gs_exposure_bwd: v_image holds dL/d out on entry and dL/d render = A^T v on exit, in place, per channel j
 *     fma(A_2j, v_2, fma(A_1j, v_1, A_0j * v_0));
 *   v_affine12[3][4] row-major = {dA_ij = sum_p v_i[p] render_j[p], db_i = sum_p v_i[p]} of the gradient as it came in.  Every
 *   product is formed exactly in fp64 from its fp32 factors; the sums are fp64 in a fixed order -- per thread over its grid-stride
 *   pixels, over the wave, over the block's waves, then one pass over the per-block partials[gs_exposure_partials_doubles(height,
 *   width)] -- and rounded to fp32 once.  No atomics: two runs give the same bits.
 * gs_exposure_adam: Adam (gs_adam_step's arithmetic per element) over ALL n_views x 12 entries with the gradient v_affine12 on the
 *   record's row and exactly 0 on every other row -- torch.optim.Adam over the whole table: idle rows decay their moments and move.
 *   Honours the step guard: a voided step leaves the table and the moments untouched. */
#define GS_EXPOSURE_REC_FLOATS 4
#define GS_EXPOSURE_REC_SS 0
#define GS_EXPOSURE_REC_ISBC2 1
#define GS_EXPOSURE_REC_VIEW 2
#define GS_EXPOSURE_MAX_VIEWS 1048576
int gs_exposure_step_inputs(void* stream, int view, int n_views, float lr, float beta1, float beta2, int64_t step, float* rec_dev);
int gs_exposure_apply(void* stream, int height, int width, int n_views, const float* rec_dev, int view, const float* table,
                      const float* render, float* out);
size_t gs_exposure_partials_doubles(int height, int width);
int gs_exposure_bwd(void* stream, int height, int width, int n_views, const float* rec_dev, int view, const float* table,
                    const float* render, float* v_image, double* partials, float* v_affine12);
int gs_exposure_adam(void* stream, int n_views, const float* rec_dev, float* table, float* exp_avg, float* exp_avg_sq,
                     const float* v_affine12, float beta1, float beta2, float eps);

/* ---- Per-view bilateral grids (DESIGN.md "Bilateral grids in the captured step"): bilagrid.BilateralGrids' learnable low-resolution
 * 3-D grid of 3x4 colour affines per training image, grids[n_views][12][grid_l][grid_y][grid_x] f32 (channel k = 4 i + j is entry
 * (i, j) of [A | b]), sliced at each pixel's position and at the luminance of the UN-clamped render's own colour c and applied to it:
 *     luma = fma(0.114, c_2, fma(0.587, c_1, 0.299 c_0))
 *     (gx, gy, gz) = ((x + 0.5) / width * (grid_x - 1), (y + 0.5) / height * (grid_y - 1), clamp(luma, 0, 1) * (grid_l - 1))
 *     M = the trilinear interpolation of the 12 channels at (gx, gy, gz),   out = M[:, :3] c + M[:, 3]
 * -- torch's grid_sample(mode="bilinear", align_corners=True, padding_mode="border").  The math is csrc/gs_bilagrid.h (shared with
 * the host tests): the cell is min(floor(g), n - 2) per axis, never outside the slab whatever the render holds; the interpolation
 * is lerps fma(t, b - a, a) along x, then y, then z (equal nodes interpolate to themselves); the apply is gs_exposure_apply's chain.
 * At [I | 0] in every node the input comes back exactly (a -0 as +0).  Images are [height][width][3] f32; images, grids and v_slab
 * 16-byte aligned.  2 <= grid_x, grid_y <= GS_BILAGRID_MAX_XY, 2 <= grid_l <= GS_BILAGRID_MAX_L, 1 <= n_views <=
 * GS_BILAGRID_MAX_VIEWS, n_views * 12 * grid_l * grid_y * grid_x < 2^31, 3 * height * width < 2^31: anything else is GS_ERR_ARG before
 * any launch.
 * gs_bilagrid_step_inputs: gs_exposure_step_inputs for the grids' own Adam: rec_dev[GS_BILAGRID_REC_FLOATS] f32, 16-byte aligned =
 *   {lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step), the bits of the int32 view index, 0}.
 * gs_bilagrid_apply: out = the slice of a view's slab applied to render.  The view: the record's when rec_dev is non-NULL (the
 *   captured step), else `view` (eager).  out may not alias render.
 * gs_bilagrid_bwd: v_image holds dL/d out on entry and dL/d render on exit, in place:
 *     M[:, :3]^T v + (0.299, 0.587, 0.114) v_luma,   v_luma = (grid_l - 1) sum_i v_i ((M_z1 - M_z0)_i . [c; 1]) for 0 < luma < 1, else 0
 *   (M_z0, M_z1: the bilinear interpolants on the cell's two luminance planes); v_slab[12][grid_l][grid_y][grid_x], fully written =
 *   the adjoint of the interpolation applied to v_out [c; 1]^T, summed over the pixels.  No atomics: a block owns (spatial cell,
 *   chunk of its pixels, luminance node) and sums its pixels' terms -- exact fp64 products of the fp32 factors times fp64 weights --
 *   per thread, over the wave, over the block's waves in order into partials[gs_bilagrid_partials_doubles(...)]; a second kernel
 *   adds, per node, the partials of the at most four cells that touch it (cell rows, then columns, then chunks ascending) and
 *   rounds to fp32 once.  Two runs give the same bits.
 * gs_bilagrid_tv: tv = (1 / n_views) sum over the axes a in {l, y, x} of sum((forward difference along a)^2) / count_a, count_a
 *   the differences along a in one view's slab; the sum in fp64 in a fixed order (tv_ws[GS_BILAGRID_TV_DOUBLES] doubles of scratch).
 *   tv_out (optional): tv_out[0] = tv; loss3 (optional): loss3[2] += tv_weight * tv, the product rounded on its own (as gs_scale_reg
 *   enters the total); v_grids (optional) [n_views][12][grid_l][grid_y][grid_x], fully written = fl32(tv_weight * d tv / d grids),
 *   plus v_slab (optional) on the view's slab (the record's view, else `view`).  Reads the grids only.  Honours the step guard.
 * gs_bilagrid_adam: Adam (gs_adam_step's arithmetic per element) over ALL numel = n_views * 12 * grid_l * grid_y * grid_x elements
 *   with the gradient v_grids -- torch.optim.Adam over the whole parameter: idle views decay their moments and move.  Honours the
 *   step guard: a voided step leaves the grids and the moments untouched. */
#define GS_BILAGRID_REC_FLOATS 4
#define GS_BILAGRID_REC_SS 0
#define GS_BILAGRID_REC_ISBC2 1
#define GS_BILAGRID_REC_VIEW 2
#define GS_BILAGRID_MAX_VIEWS 1048576
#define GS_BILAGRID_MAX_XY 64
#define GS_BILAGRID_MAX_L 16
#define GS_BILAGRID_TV_DOUBLES 1024
int gs_bilagrid_step_inputs(void* stream, int view, int n_views, float lr, float beta1, float beta2, int64_t step, float* rec_dev);
int gs_bilagrid_apply(void* stream, int height, int width, int n_views, int grid_x, int grid_y, int grid_l, const float* rec_dev,
                      int view, const float* grids, const float* render, float* out);
size_t gs_bilagrid_partials_doubles(int height, int width, int grid_x, int grid_y, int grid_l);
int gs_bilagrid_bwd(void* stream, int height, int width, int n_views, int grid_x, int grid_y, int grid_l, const float* rec_dev,
                    int view, const float* grids, const float* render, float* v_image, double* partials, float* v_slab);
int gs_bilagrid_tv(void* stream, int n_views, int grid_x, int grid_y, int grid_l, const float* grids, float tv_weight,
                   const float* rec_dev, int view, const float* v_slab, float* loss3, float* tv_out, float* v_grids, double* tv_ws);
int gs_bilagrid_adam(void* stream, int64_t numel, const float* rec_dev, float* grids, float* exp_avg, float* exp_avg_sq,
                     const float* v_grids, float beta1, float beta2, float eps);

/* ---- Depth supervision (DESIGN.md "Depth supervision in the captured step"): depth_loss.depth_loss / DepthSupervision -- gsplat's
 * trainer's depth term on the expected depth of the RGB+ED render.  For a frame of P = height * width pixels, the math of
 * csrc/gs_depth_loss.h (shared with the host tests):
 *     d = acc_z / max(alpha, 1e-10)                               the prediction (gs_math.h expected_depth)
 *     valid = t > 0 and t finite                                  the target t[height][width] f32: NaN, inf, 0 and negatives = none
 *     w = valid * (1 - m)                                         m: the mask at the pixel (1 excludes it), 0 without a mask
 *     e = d - t  (GS_DEPTH_MODE_DEPTH)   or   disp(d) - 1 / t  (GS_DEPTH_MODE_DISPARITY),   disp(d) = d > 0 ? 1 / d : 0
 *     value = sum(w |e|) / sum(w),   exactly 0 when sum(w) == 0
 *     d value / d d = w sign(e) / sum(w) * {depth: 1; disparity: d > 0 ? -1 / d^2 : 0},   sign(0) = 0
 * Every product w |e| is formed exactly in fp64 from its fp32 factors; the two sums are fp64 in a fixed order -- per thread over
 * its grid-stride pixels, over the wave, over the block's waves, then one pass over the per-block
 * partials[gs_depth_loss_partials_doubles(height, width)] -- and value and 1 / sum(w) are rounded to fp32 once.  No atomics: two
 * runs give the same bits.  A frame without a valid pixel gives value 0 and gradients 0, never a NaN.
 * rec_dev[GS_DEPTH_REC_FLOATS] f32, 16-byte aligned: {lambda_depth, the bits of the int32 mode, the target's 64-bit address (two
 * words), value, 1 / sum(w), 0, 0}.  Images, the target and the depth maps are 16-byte aligned, the mask 4-byte; anything else, a
 * null pointer, an output that aliases an input or an unknown mode is GS_ERR_ARG before any launch.  Every kernel that runs INSIDE
 * a step -- split, finish, join, fwd, bwd, gs_depth_grads_z, gs_project_bwd_adam_depth -- honours the step guard: a voided step
 * leaves value and 1 / sum(w), the images and the gradients as they were.
 * gs_depth_step_inputs: a one-wave launch in front of a step, outside its guarded sequence (as gs_exposure_step_inputs: the values
 *   travel as kernel arguments; four lanes write), that writes words 0-3 of the record.  It does NOT look at the guard: a voided
 *   step is replayed behind a staging launch of its own.  The target is read IN PLACE by the kernels below: it stays alive until
 *   they have run.
 * gs_depth_loss_split / _fwd / _join / _bwd take {lambda_depth, mode, target} from the record when `target` is NULL (the captured
 *   step) and from their arguments otherwise; the mask is slot 1 of img_slots (gs_step_inputs' {gt, mask} addresses) when img_slots
 *   is non-NULL, else `mask` (NULL: none).
 * gs_depth_loss_split: ONE pass over the 4-channel blend colors4[height][width][4] = {r, g, b, acc_z} and alphas: image3 = the
 *   first three channels bit for bit, depth = d, and the partials.
 * gs_depth_loss_finish: a one-block launch behind it -- in the step behind gs_l1_ssim_fwd*, which writes loss3 -- that writes value
 *   and 1 / sum(w) into the record and (loss3 non-NULL) loss3[2] += lambda_depth * value, the product rounded on its own (as
 *   gs_scale_reg enters the total); lambda_depth from the record when `staged` is 1.
 * gs_depth_loss_fwd: the same sums and the finish from a depth map (the eager form: depth = what gs_expected_depth_fwd returned), mode and target
 *   by value; the same pixel-to-thread assignment, hence the same bits.
 * gs_depth_loss_join: ONE pass behind the image loss's backward: v_colors4[p] = {v_render[p], v_acc} and v_alphas[p] = v_alpha with
 *   (v_acc, v_alpha) = expected_depth_vjp(lambda_depth / sum(w) * d value / d d ...), the gradients gs_blend_bwd_ch takes at 4
 *   channels.  Reads value's 1 / sum(w) from the record.
 * gs_depth_loss_bwd: v_depth[p] = v_loss[0] * d value / d d (v_loss: the upstream gradient, one float on the device).
 * gs_depth_grads_z: gs_depth_grads' fixed-order gather alone: v_depths[C][N] = the sum of lane `lane` of the colour quad of each
 *   Gaussian's gradient rows, 0 for culled ones; no gradient is touched.  One round only, like gs_depth_grads.
 * gs_project_bwd_adam_depth: gs_project_bwd_adam / _reg / _mcmc (scale_reg, budget: 0 or 1, with their parameters) with
 *   v_depths[N] * viewmats[0][2][0:3] added to the means gradient behind the projection's VJP (gs_math.h depth_vjp_mean) -- the
 *   same update, bit for bit, as gs_project_bwd, gs_depth_grads onto its v_means, the regularisers, gs_adam_step_dev. */
#define GS_DEPTH_MODE_DEPTH 0
#define GS_DEPTH_MODE_DISPARITY 1
#define GS_DEPTH_REC_FLOATS 8
#define GS_DEPTH_REC_LAMBDA 0
#define GS_DEPTH_REC_MODE 1
#define GS_DEPTH_REC_TARGET 2
#define GS_DEPTH_REC_VALUE 4
#define GS_DEPTH_REC_INV_W 5
int gs_depth_step_inputs(void* stream, float lambda_depth, int mode, const float* target, float* rec_dev);
size_t gs_depth_loss_partials_doubles(int height, int width);
int gs_depth_loss_split(void* stream, int height, int width, float* rec_dev, float lambda_depth, int mode, const float* target,
                        const float* mask, const int64_t* img_slots, const float* colors4, const float* alphas, float* image3,
                        float* depth, double* partials);
int gs_depth_loss_finish(void* stream, int height, int width, float* rec_dev, float lambda_depth, int staged, const double* partials,
                         float* loss3);
int gs_depth_loss_fwd(void* stream, int height, int width, float* rec_dev, int mode, const float* target, const float* mask,
                      const float* depth, double* partials);
int gs_depth_loss_join(void* stream, int height, int width, const float* rec_dev, float lambda_depth, int mode, const float* target,
                       const float* mask, const int64_t* img_slots, const float* colors4, const float* alphas, const float* depth,
                       const float* v_render, float* v_colors4, float* v_alphas);
int gs_depth_loss_bwd(void* stream, int height, int width, const float* rec_dev, int mode, const float* target, const float* mask,
                      const float* depth, const float* v_loss, float* v_depth);
int gs_depth_grads_z(void* stream, int C, int64_t N, int lane, const int32_t* radii, const int32_t* tiles_per_gauss,
                     const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_depths);
int gs_project_bwd_adam_depth(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                              const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                              float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                              const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                              const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                              int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac,
                              int scale_reg, float max_ratio, float lambda, int budget, double a, double b, const float* v_depths);

/* Camera models (rasterization(camera_model=...); DESIGN.md "Camera models").  Only the projection knows the camera model: the mean
 * goes to camera space (x, y, z) and is culled on z (near / far) as for the pinhole, cov2 = J cov_c J^T + eps2d I with the model's map
 * and Jacobian, and everything behind cov2 -- determinant cull, radius, conic, screen cull, tile rectangle, tight culling, and every
 * stage that consumes means2d / conics / depths / radii / the footprint -- is unchanged.  The SH view direction stays mean - camera centre.
 *   GS_CAMERA_PINHOLE  (fx x / z + cx, fy y / z + cy), J with the FOV clamp: the entry points without `_cm`
 *   GS_CAMERA_ORTHO    (fx x + cx, fy y + cy), J = [[fx, 0, 0], [0, fy, 0]], no clamp
 *   GS_CAMERA_FISHEYE  ideal equidistant, no distortion terms: (fx x k + cx, fy y k + cy), k = theta / r, theta = atan2(r, z),
 *                      r^2 = x^2 + y^2; J = [[fx (k + x^2 g), fx x y g, -fx x / d^2], [fy x y g, fy (k + y^2 g), -fy y / d^2]] with
 *                      d^2 = r^2 + z^2, g = (z / d^2 - k) / r^2; no clamp; k, g and (in the VJP) dg/dr come from a series in
 *                      (r / z)^2 below (r / z)^2 < 1/256, so a Gaussian on the optical axis is an ordinary visible one
 * The `_cm` entry points take the arguments of the entry point they are named after plus `camera_model` last; with GS_CAMERA_PINHOLE
 * they are that entry point (same kernels).  The other models: gs_project_fwd_cm stage 2 (colour only) launches the pinhole path's
 * kernel (the stage has no camera model in it); gs_project_bwd_cm / gs_project_bwd_cam_cm walk the gradient rows (row_sums, stat_grad_norm
 * and stat_count NULL); the fused backward + Adam exists plain and with the scale-ratio regulariser -- there is no budget, row-sums
 * or depth variant of it. */
#define GS_CAMERA_PINHOLE 0
#define GS_CAMERA_ORTHO 1
#define GS_CAMERA_FISHEYE 2
int gs_project_fwd_cm(void* stream, int C, int64_t N, int K, int sh_degree, const float* means, const float* quats,
                      const float* scales, const float* opacities, const float* colors_in, const float* sh_rest,
                      int colors_per_camera, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                      float near_plane, float far_plane, float radius_clip, int tile_culling, int stage, int activations,
                      int32_t* radii, float* means2d, float* depths, float* conics, float* colors_out, float* rec, uint32_t* bbox,
                      int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac, int camera_model);
int gs_project_bwd_cm(void* stream, int C, int64_t N, int K, int sh_degree, const float* means, const float* quats,
                      const float* scales, const float* colors_in, const float* sh_rest, int colors_per_camera,
                      const float* viewmats, const float* Ks, int width, int height, float eps2d, float near_plane, float far_plane,
                      const int32_t* radii, const float* colors_post, const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                      const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats,
                      float* v_scales, float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                      float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre, const float* opacities,
                      int activations, const float* sh_jac, const float* row_sums, float* stat_grad_norm, float* stat_count,
                      int camera_model);
int gs_project_bwd_cam_cm(void* stream, int C, int64_t N, int K, int sh_degree, const float* means, const float* quats,
                          const float* scales, const float* colors_in, const float* sh_rest, int colors_per_camera,
                          const float* viewmats, const float* Ks, int width, int height, float eps2d, float near_plane,
                          float far_plane, const int32_t* radii, const float* colors_post, const int32_t* tiles_per_gauss,
                          const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means,
                          float* v_quats, float* v_scales, float* v_opacities, float* v_colors, float* v_sh_rest,
                          float* v_means2d_abs, float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                          const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                          float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats, float* v_campos,
                          int camera_model);
int gs_project_bwd_adam_cm(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                           const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                           float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                           const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                           const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                           int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac,
                           int camera_model);
int gs_project_bwd_adam_reg_cm(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                               const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                               float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                               const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                               const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps,
                               const float* hyper_dev, int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                               const float* sh_jac, float max_ratio, float lambda, int camera_model);

/* Antialiased mode (rasterization(rasterize_mode="antialiased"); DESIGN.md "Antialiased mode").  A property of the projection alone, pinhole
 * model only: with cov2_0 = J cov_c J^T taken BEFORE eps2d joins its diagonal and cov2 = cov2_0 + eps2d I (what the cull, the radius and the
 * conic are formed from, unchanged),
 *   rho = sqrt(max(0, det(cov2_0) / det(cov2)))  in [0, 1),    op_eff = opacity * rho   (the activated opacity with activations),
 * and everything behind the projection that took the opacity takes op_eff: the blend record, the opacity-aware extents, the tight
 * rectangle and the per-tile mask.  radii, means2d, conics, depths and the 3-sigma rectangle are those of the classic call.  rho = 0 (a
 * rank-deficient covariance) is an opacity of 0.  Backward: the row sum's gradient of the record's opacity v_eff gives v_opacity = v_eff
 * rho and v_rho = v_eff opacity, and v_rho joins v_cov2 in front of the chain's VJP through
 *   d rho / d cov2_0 = (adj(cov2_0) - rho^2 adj(cov2)) / (2 (rho + 1e-6) det(cov2)).
 * The `_aa` entry points take the arguments of the entry point they are named after; gs_project_fwd_aa additionally `compensations`
 * ([C*N], rho, 0 where culled; never NULL; stage 2 -- colour only -- launches the classic kernel and leaves it alone).  `opacities` is
 * never NULL in the backward entries; row_sums, stat_grad_norm and stat_count are NULL (the gradient rows are walked); one depth round.
 * gs_project_bwd_cam_aa's cam_partials holds gs_cam_partials_doubles_aa(C, N) doubles: the block partials, and behind them the C*N
 * record-opacity gradients the projection backward leaves for the camera kernel.  The fused backward + Adam exists plain and with the
 * scale-ratio regulariser -- there is no budget, row-sums or depth variant of it. */
size_t gs_cam_partials_doubles_aa(int C, int64_t N);
int gs_project_fwd_aa(void* stream, int C, int64_t N, int K, int sh_degree, const float* means, const float* quats,
                      const float* scales, const float* opacities, const float* colors_in, const float* sh_rest,
                      int colors_per_camera, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                      float near_plane, float far_plane, float radius_clip, int tile_culling, int stage, int activations,
                      int32_t* radii, float* means2d, float* depths, float* conics, float* colors_out, float* rec, uint32_t* bbox,
                      int32_t* tiles_per_gauss, uint32_t* rect_ref, float* sh_jac, float* compensations);
int gs_project_bwd_aa(void* stream, int C, int64_t N, int K, int sh_degree, const float* means, const float* quats,
                      const float* scales, const float* colors_in, const float* sh_rest, int colors_per_camera,
                      const float* viewmats, const float* Ks, int width, int height, float eps2d, float near_plane, float far_plane,
                      const int32_t* radii, const float* colors_post, const int32_t* tiles_per_gauss, const int32_t* cum_tiles,
                      const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means, float* v_quats,
                      float* v_scales, float* v_opacities, float* v_colors, float* v_sh_rest, float* v_means2d_abs,
                      float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre, const float* opacities,
                      int activations, const float* sh_jac, const float* row_sums, float* stat_grad_norm, float* stat_count);
int gs_project_bwd_cam_aa(void* stream, int C, int64_t N, int K, int sh_degree, const float* means, const float* quats,
                          const float* scales, const float* colors_in, const float* sh_rest, int colors_per_camera,
                          const float* viewmats, const float* Ks, int width, int height, float eps2d, float near_plane,
                          float far_plane, const int32_t* radii, const float* colors_post, const int32_t* tiles_per_gauss,
                          const int32_t* cum_tiles, const float* rows, const int32_t* row_base, const uint8_t* qmask, float* v_means,
                          float* v_quats, float* v_scales, float* v_opacities, float* v_colors, float* v_sh_rest,
                          float* v_means2d_abs, float* v_means2d, float* v_conics, float* v_colors_post, float* v_colors_pre,
                          const float* opacities, int activations, const float* sh_jac, const float* row_sums,
                          float* stat_grad_norm, float* stat_count, double* cam_partials, float* v_viewmats, float* v_campos);
int gs_project_bwd_adam_aa(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                           const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height, float eps2d,
                           float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                           const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                           const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps, const float* hyper_dev,
                           int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts, const float* sh_jac);
int gs_project_bwd_adam_reg_aa(void* stream, int64_t N, int K, int sh_degree, float* params, float* exp_avg, float* exp_avg_sq,
                               const int64_t* offsets_host, const float* viewmats, const float* Ks, int width, int height,
                               float eps2d, float near_plane, float far_plane, const int32_t* radii, const float* colors_post,
                               const int32_t* tiles_per_gauss, const int32_t* cum_tiles, const float* rows, const int32_t* row_base,
                               const uint8_t* qmask, float* v_means2d_abs, float beta1, float beta2, float eps,
                               const float* hyper_dev, int64_t* applied_dev, float* max_radii, float* grad_norm_accum, float* counts,
                               const float* sh_jac, float max_ratio, float lambda);

/* Packed meta and sparse gradient rows (rasterization(packed=True, sparse_grad=True)).  The pipeline stays dense;
 * these compact what a call hands out.  The visible pairs are the (c, n) with radii[c][n] > 0 in row-major order (camera-major,
 * Gaussian ascending); the seen Gaussians are the n some camera saw, ascending.  Eager-path kernels: the step guard does not
 * apply.  C*N + N < 2^31.  No atomics; every store is checked against the totals.
 * gs_pack_flags: flags[C*N (+ N)] (0/1) = the pair flags and -- want_seen -- behind them the seen flags; incl = the inclusive
 *   scan of flags taken as ONE row (gs_scan_rows_i32; scan_workspace: gs_scan_rows_workspace_ints(1, C*N (+ N)) int32), so
 *   incl[i] - 1 is the packed row of visible pair i and incl[C*N + n] - nnz - 1 the rank of seen Gaussian n.  Its last kernel
 *   writes {nnz, nu} (nu = 0 without want_seen) to totals_host_mapped -- int64[2] of page-locked, device-addressable host
 *   memory -- followed by a system-scope fence: a caller that records an event behind the call and waits for it reads both from
 *   plain memory.  C >= 1, N >= 1.
 * gs_pack_gather: one launch; camera_ids / gaussian_ids (int64 [nnz]), radii_out [nnz], means2d_out [nnz][2], depths_out [nnz],
 *   conics_out [nnz][3], opacities_out [nnz] = the dense arrays at the visible pairs.  opacities is [N] (broadcast over the
 *   cameras) or, opacities_per_camera != 0, [C][N].  nnz as gs_pack_flags reported it.
 * gs_pack_take: rows of `words` (1..4) 32-bit words: out[incl[i] - base - 1][:] = src[i][:] for every i < n_src at which the
 *   scan steps (incl[i] > incl[i-1]; incl[-1] = base), ids_out[...] = i (int64; either of {src, out} / ids_out may be NULL).
 *   Pairs: incl, base 0, n_src C*N, n_out nnz.  Seen Gaussians: incl + C*N, base nnz, n_src N, n_out nu.  Rows are aligned to
 *   4, 8, 4, 16 bytes.
 * gs_pack_remap: out[i] = incl[flatten_ids[i]] - 1, the packed row of the listed pair (every listed entry is a visible pair;
 *   an index outside [0, pairs) yields -1 instead of a read). */
int gs_pack_flags(void* stream, int C, int64_t N, const int32_t* radii, int want_seen, int32_t* flags, int32_t* incl,
                  int32_t* scan_workspace, int64_t* totals_host_mapped);
int gs_pack_gather(void* stream, int C, int64_t N, int64_t nnz, const int32_t* radii, const int32_t* incl, const float* means2d,
                   const float* depths, const float* conics, const float* opacities, int opacities_per_camera,
                   int64_t* camera_ids, int64_t* gaussian_ids, int32_t* radii_out, float* means2d_out, float* depths_out,
                   float* conics_out, float* opacities_out);
int gs_pack_take(void* stream, int64_t n_src, int64_t n_out, int words, const int32_t* incl, int32_t base, const void* src,
                 void* out, int64_t* ids_out);
int gs_pack_remap(void* stream, int64_t n, int64_t pairs, const int32_t* flatten_ids, const int32_t* incl, int32_t* out);

/* Blend-weight scores (rendering.blend_weights, importance.py): how much each Gaussian contributed to an image.  The
 * blend TAKES the pair (pixel p, Gaussian n) of camera c when the pixel is live, sigma >= 0, alpha = min(0.999, opacity exp(-sigma))
 * >= 1/255 and T' = fma(-alpha, T, T) > 1e-4 (opacity: what the blend record holds); a taken pair has the weight w = alpha T.
 * Per (c, n): weight_sum = the sum of w over the taken pixels, weight_max = their maximum (0: none), hits = their number.
 * A call sequence: a training-mode gs_blend_fwd / gs_blend_fwd_ch (any channel count; one depth round), gs_blend_scores,
 * gs_score_reduce [, gs_score_accumulate].  No atomics anywhere: two runs agree bit for bit.
 * gs_blend_scores: replays the walk the forward left (qlist, qcnt, unit_desc, the T plane of ckpt, qmask, row_base, walk_state)
 *   through the work-unit pipelines of gs_blend_bwd -- unit_classes as there: may be NULL -- and evaluates sigma, alpha, w and T' with
 *   the backward's (= the forward's) instruction sequence: the taken set and every w are the forward's bit for bit.  It reads neither
 *   an image nor a colour.  Writes one 4-float row (weight sum, weight max, taken pixels as int32, 0) per (intersection, quadrant)
 *   some pixel took into score_rows[cap_rows*4], at the index of the pair's gradient row (row_base[slot] + rank of the quadrant) --
 *   the rows region gs_blend_bwd writes (cap_rows*12 floats) holds them.  Nothing is written when the step guard is tripped or
 *   the walk is void (GS_FLAG_UNITS / GS_FLAG_ROWS in walk_state[GS_WALK_FLAGS]).  16-byte aligned: rec, qlist, unit_desc, ckpt,
 *   qmask, score_rows, unit_classes.
 * gs_score_reduce: weight_sum / weight_max (f32) and hits (i32), each [C*N] and fully written: the rows of every Gaussian gathered
 *   as gs_channel_grads gathers them and folded in a fixed order; zeros for culled Gaussians (radii <= 0), Gaussians without rows
 *   and a void walk.  Honours the step guard.
 * gs_score_accumulate: one launch; folds a [C*N] triple and radii into per-Gaussian running totals, the cameras in order:
 *   total_weight_sum f64 [N] += weight_sum; total_weight_max f32 [N] = max; total_hits i64 [N] += hits; views_seen i32 [N] +=
 *   (radii > 0); views_hit i32 [N] += (hits > 0).  Honours the step guard. */
int gs_blend_scores(void* stream, int C, int width, int height, const float* rec, const int32_t* qlist,
                    const int32_t* qcnt, const int32_t* unit_desc, int64_t cap_units, const float* ckpt,
                    const uint8_t* qmask, const int32_t* row_base, const int32_t* walk_state, float* score_rows,
                    int64_t cap_rows, int32_t* unit_classes);
int gs_score_reduce(void* stream, int C, int64_t N, const int32_t* radii, const int32_t* tiles_per_gauss,
                    const int32_t* cum_tiles, const float* score_rows, int64_t cap_rows, const int32_t* row_base,
                    const uint8_t* qmask, const int32_t* walk_state, float* weight_sum, float* weight_max, int32_t* hits);
int gs_score_accumulate(void* stream, int C, int64_t N, const float* weight_sum, const float* weight_max,
                        const int32_t* hits, const int32_t* radii, double* total_weight_sum, float* total_weight_max,
                        int64_t* total_hits, int32_t* views_seen, int32_t* views_hit);

/* ---- k-means on the device (kmeans.py, compress.py; DESIGN.md "Exporting a trained model"): Lloyd's assignment and update for
 * N points x[N][D] and K centroids [K][D], float32.  The definition is csrc/gs_kmeans.h, one k-ascending fmaf chain per sum:
 *   score(x, c) = fmaf(-2, dot(x, c), dot(c, c)),  label(x) = the smallest index among the centroids of minimal score (a NaN score
 *   never wins; none wins: label 0),  dist2(x) = chain_k fmaf(d_k, d_k, acc) with d_k = x_k - c_label,k.
 * The results are that function of the input bit for bit, whatever the tiling (the product runs on the f32-input MFMA
 * v_mfma_f32_32x32x2_f32, whose result IS the chain).  No atomics: the same input gives the same bits.  No synchronisation.
 * gs_kmeans_assign: labels int32[N] in [0, K), dist2 float[N]; two launches (centroids k-major with their norms into the workspace,
 *   then the fused product + argmin: no score is stored).  workspace: gs_kmeans_workspace_bytes(N, K, D) bytes, 256-byte aligned,
 *   scratch (every word read is written by the same call).
 * gs_kmeans_update: one launch.  order int32[N] = the point indices sorted by label with a STABLE sort, seg int32[K+1] = the segment
 *   offsets of the labels in it (both from the caller's sort / bincount + cumsum).  Cluster j's members order[seg[j] .. seg[j+1]) are
 *   summed in that order in fp64, one accumulator per (cluster, dimension): centroids[j][d] = (float)(sum / count), counts[j] = the
 *   number of members.  An empty cluster keeps its centroid's bits.  A segment is clamped to [0, N] and an entry of order outside
 *   [0, N) is skipped and not counted, never dereferenced.
 * Refused with GS_ERR_ARG before a launch: N outside [1, GS_KMEANS_MAX_N], K outside [1, GS_KMEANS_MAX_K], D outside
 * [1, GS_KMEANS_MAX_D], null pointers, a misaligned workspace; gs_kmeans_workspace_bytes returns 0 for such sizes. */
#define GS_KMEANS_MAX_D 128
#define GS_KMEANS_MAX_K 16777216      /* 2^24: labels and the padded k-major copy are indexed in int32 / int64 */
#define GS_KMEANS_MAX_N 1073741824    /* 2^30: point indices are int32 */
size_t gs_kmeans_workspace_bytes(int64_t N, int64_t K, int D);
int gs_kmeans_assign(void* stream, int64_t N, int64_t K, int D, const float* x, const float* centroids, int32_t* labels,
                     float* dist2, void* workspace);
int gs_kmeans_update(void* stream, int64_t N, int64_t K, int D, const float* x, const int32_t* order, const int32_t* seg,
                     float* centroids, int32_t* counts);

/* ---- a triangle mesh out of rendered depth (mesh.py): TSDF fusion of pinhole views into a dense volume and
 * marching tetrahedra over it.  The definition is csrc/gs_tsdf.h; every result is that function of the input bit for bit.  No
 * atomics: the same input gives the same bits.  Eager-path kernels: the step guard does not apply.
 * The volume: dims = {nx, ny, nz} voxels (host array), samples at origin + i * h per axis (origin: host array), linear index
 * ix + nx * (iy + ny * iz); tsdf float[n] (fresh: 1), weight float[n] (fresh: 0), color float[n][3] (fresh: 0) or NULL.
 * Every dimension >= 2, h > 0 and 7 * nx * ny * nz < 2^31: anything else is GS_ERR_ARG before a launch, as are null pointers and
 * the argument errors named below.
 * gs_tsdf_integrate: one launch folds one view in.  viewmat_dev float[16] (world -> camera, row-major) and K_dev float[9] (fx, fy,
 *   cx, cy; no skew) are DEVICE memory: a render loop needs no host synchronisation.  image float[H][W][image_stride] is read in
 *   place -- the buffer rasterization(render_mode="RGB+ED") returns --, the depth in channel depth_channel, the colour in the three
 *   channels from color_channel (or -1 and color == NULL: depth only); alphas float[H][W] or NULL.  A voxel the view does not
 *   reach (gs_tsdf.h) keeps all its bits.  trunc > 0 finite, max_weight > 0 (may be +inf), depth_max may be +inf, H*W*stride < 2^31, W and H <= 2^24.
 * gs_mt_flags: edge_flags int32[7n] (zeroed here; 1: the edge (owner voxel, kind) -- index owner * 7 + kind - 1 -- carries a vertex),
 *   tri_counts int32[n] (the triangles of the cell whose lowest corner the voxel is), their inclusive scans edge_incl / tri_incl
 *   (gs_scan_rows_i32; scan_workspace: gs_mt_scan_workspace_ints(dims) int32), and {vertices, faces} into totals_host_mapped --
 *   int64[2] of page-locked, device-addressable host memory -- followed by a system-scope fence, as gs_pack_flags does it: the one
 *   host read of an extraction.  min_weight > 0.  A volume with more than 2^31 - 1 triangles overflows tri_incl: the caller checks
 *   0 <= faces <= 12 n.
 * gs_mt_vertices: vertices float[n_vertices][3] and -- with color -- colors float[n_vertices][3], numbered by (owner, kind)
 *   ascending.  gs_mt_faces: faces int32[n_faces][3], ordered by (cell, tetrahedron, triangle), (v1 - v0) x (v2 - v0) pointing
 *   from inside (tsdf < 0) to outside.  One launch each, none when the total is 0; no store leaves the exactly-sized outputs. */
int gs_tsdf_integrate(void* stream, const int32_t dims[3], const float origin[3], float h, float trunc, float depth_max,
                      float min_alpha, float max_weight, const float* viewmat_dev, const float* K_dev, int W, int H,
                      const float* image, int image_stride, int depth_channel, int color_channel, const float* alphas,
                      float* tsdf, float* weight, float* color);
size_t gs_mt_scan_workspace_ints(const int32_t dims[3]);
int gs_mt_flags(void* stream, const int32_t dims[3], float min_weight, const float* tsdf, const float* weight,
                int32_t* edge_flags, int32_t* edge_incl, int32_t* tri_counts, int32_t* tri_incl, int32_t* scan_workspace,
                int64_t* totals_host_mapped);
int gs_mt_vertices(void* stream, const int32_t dims[3], const float origin[3], float h, const float* tsdf, const float* color,
                   const int32_t* edge_flags, const int32_t* edge_incl, int64_t n_vertices, float* vertices, float* colors);
int gs_mt_faces(void* stream, const int32_t dims[3], const float* tsdf, const int32_t* tri_counts, const int32_t* tri_incl,
                const int32_t* edge_incl, int64_t n_vertices, int64_t n_faces, int32_t* faces);

/* ---- regularising normals for meshing (normals.py): the normal of every Gaussian in camera space, and the
 * consistency loss between the blended normals and the normals of the rendered depth.  The definition is csrc/gs_normals.h; every
 * normal and every gradient is that function of the input bit for bit, the value its terms summed in fp64 in a fixed order.  No
 * atomics: the same input gives the same bits.  Eager-path kernels: the step guard does not apply.
 * gs_gauss_normals_fwd: means float[N][3], quats float[N][4] (wxyz, not normalised), scales float[N][3] (raw or activated: only
 *   their order counts), viewmats float[C][16] (world -> camera, row-major, DEVICE memory) -> normals float[C][N][3], the column of
 *   R(q / |q|) along the smallest scale, in camera space, faced towards the camera.  gs_gauss_normals_bwd: v_normals float[C][N][3]
 *   -> v_quats float[N][4], written whole, the cameras summed in their order; means and scales receive nothing (the axis and the
 *   facing are piecewise constant).  0 <= N < 2^31, C >= 1; N == 0 launches nothing.
 * gs_normal_loss_fwd: render4 float[H][W][4], 16-byte aligned, read in place -- channels 0..2 the blended normal Nb, channel 3 the
 *   expected z-depth, what rasterization(render_mode="RGB+ED") returns --, alphas float[H][W], mask float[H][W] or NULL (1 excludes
 *   a pixel), K_dev float[9] in DEVICE memory (fx, fy, cx, cy; no skew).  A pixel is valid when it is interior, it and its four
 *   neighbours have alpha >= min_alpha and a finite depth > 0, and the cross product of the central differences has a finite
 *   squared length >= 1e-30.  rec_dev float[GS_NORMAL_REC_FLOATS]: value = sum(w (1 - dot(Nb, n_d))) / sum(w), w = valid * (1 -
 *   mask), and 1 / sum(w), both exactly 0 when nothing counts; partials double[gs_normal_loss_partials_doubles(H, W)].
 *   depth_normals float[H][W][3] or NULL: n_d where the pixel is valid (the mask aside), zeros elsewhere.  rec_dev and partials may
 *   both be NULL when only depth_normals is wanted.  One image pass over GS_NORMAL_TILE_W x GS_NORMAL_TILE_H tiles and a one-block finish.
 * gs_normal_loss_bwd: v_loss: the upstream gradient of the value, one float on the device; rec_dev: what the forward wrote.
 *   v_render4 float[H][W][4], 16-byte aligned, EVERY element written: channels 0..2 the gradient of Nb, channel 3 the gradient of the
 *   depth (exact zeros with detach_depth = 1); zeros where nothing arrives.  Alphas receive no gradient (validity is a threshold).
 * H * W * 4 >= 2^31, a NaN min_alpha and null or misaligned pointers are GS_ERR_ARG before any launch. */
#define GS_NORMAL_TILE_W 64
#define GS_NORMAL_TILE_H 8
#define GS_NORMAL_REC_FLOATS 4
#define GS_NORMAL_REC_VALUE 0
#define GS_NORMAL_REC_INV_W 1
int gs_gauss_normals_fwd(void* stream, int64_t N, int C, const float* means, const float* quats, const float* scales,
                         const float* viewmats, float* normals);
int gs_gauss_normals_bwd(void* stream, int64_t N, int C, const float* means, const float* quats, const float* scales,
                         const float* viewmats, const float* v_normals, float* v_quats);
size_t gs_normal_loss_partials_doubles(int height, int width);
int gs_normal_loss_fwd(void* stream, int height, int width, const float* K_dev, float min_alpha, const float* render4,
                       const float* alphas, const float* mask, float* rec_dev, double* partials, float* depth_normals);
int gs_normal_loss_bwd(void* stream, int height, int width, const float* K_dev, float min_alpha, int detach_depth,
                       const float* render4, const float* alphas, const float* mask, const float* rec_dev, const float* v_loss,
                       float* v_render4);

#ifdef __cplusplus
}
#endif
#endif /* GS_RASTER_H_ */
