// gs_blend_shared.h -- what the kernels that follow a training walk have in common: gs_blend.hip (the walk itself and the blend
// backward) and gs_scores.hip (the blend-weight scores, a replay of the same walk).  Moved here from gs_blend.hip unchanged.
#pragma once
#include "gs_common.h"

namespace gs {

// Work unit of the backward: kUnit consecutive entries of one quadrant sublist (half a 64-entry bucket), with a
// checkpoint of the quadrant's 64 pixel states in front of it.
constexpr int kUnit = GS_UNIT;
// words of the walk state (include/gs_raster.h: GS_WALK_*)
constexpr int kWalkUnits = GS_WALK_UNITS, kWalkStorage = GS_WALK_STORAGE, kWalkRows = GS_WALK_ROWS,
              kWalkFlags = GS_WALK_FLAGS, kWalkSkip = GS_WALK_SKIP;

// -DGS_EXACT_MATH (tools/acc64_ab.py; never in the product build): correctly rounded exp2 and division in BOTH blend kernels
// instead of the hardware approximations (v_exp_f32 / v_rcp_f32: ~1 ulp) -- the other half of the A/B on rows that cancel.
#ifdef GS_EXACT_MATH
__device__ __forceinline__ float fast_exp2(float x) { return (float)exp2((double)x); }
__device__ __forceinline__ float fast_rcp(float x) { return (float)(1.0 / (double)x); }
#else
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#endif

constexpr int kBwdWaves = 4;
constexpr int kPipeLanes = 8;                       // lanes per systolic pipeline (two pipelines share a 16-lane DPP row)
constexpr int kPerLane = kUnit / kPipeLanes;        // 4 entries per lane in a full unit (bwd_wave<E>: E = 1 .. 4)
static_assert(kPerLane == 4, "bwd_wave is instantiated for 1 .. 4 entries per lane");
constexpr int kUnitsPerWave = 64 / kPipeLanes;      // 8
// (Round 5 bounded half-quadrant -- 8 x 4 pixel -- work units with a timing build: -15 to -23 us for this kernel at the 1.55 x
//  unit count they would have, before twice the rows in the row sum; not built.  HISTORY.md, profiles/r05_halfq_bound.txt.)
constexpr int kUnitPixels = 64;
constexpr int kBwdSteps = kUnitPixels + kPipeLanes - 1;      // 71

__device__ __forceinline__ float dpp_row_shr1(float v) {
    // lane r of each 16-lane row receives lane r-1's value; lane 0 keeps its own
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, false));
}

// The fill classes of the published work units (unit_classes_kernel, gs_blend.hip): a header of kClsHdrInts counters -- units of
// class c at [c], c = 1 .. 4 -- and behind it the descriptors: class 4 at [0, cap_units), classes 3, 2, 1 in regions of
// unit_class_region() descriptors each.  unit_classes_launch clears the counters and groups the units (two launches; the buffer
// is gs_unit_classes_ints int32, 16-byte aligned).
constexpr int kClsHdrInts = 16;
int64_t unit_class_region(int C, int width, int height);
int unit_classes_launch(hipStream_t st, const int32_t* walk_state, const int4* unit_desc, const int32_t* qcnt, int cap_units,
                        int cls_cap, int32_t* unit_classes, const int64_t* guard);

}  // namespace gs
