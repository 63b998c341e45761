"""The reference's train step as ONE replayable hipGraph (SURVEY.md section 8b "Sync").

`TrainStepGraph.step(data, gt_img)` runs, for the reference's single camera per iteration
(/root/reference/train.py:36-58, 93-157):

    activations + projection + SH colour -> tile lists -> per-tile sort -> blend forward ->
    clamp + L1 + (1 - SSIM) forward / backward -> blend backward -> projection / SH backward ->
    update_statistics -> Adam step (-> gradients dropped)

through the C ABI of include/gs_raster.h directly -- the same kernels, in the same order, on the same
inputs as `model(data)` / `LossComputer` / `loss.backward()` / `update_statistics` / `FusedAdam.step` issue
them, so the two paths agree bit for bit (tests/test_gpu_train_graph.py) -- but

* every buffer lives in a persistent workspace -- the intermediates in the three arenas of the library's own layout
  (`gs_workspace_query`, as the eager seam's: `_SLOTS`) -- sized by CAPACITY -- of LISTED intersections (keys, sorted lists, quadrant
  masks, row bases: 13-25 bytes each) and of what the forward WALKS (work units with their checkpoints and sublists, gradient
  rows; round 6: rounds 1-5 sized those by the list capacity, 355 bytes per listed entry, 25 GB at 2 M Gaussians on a realistic
  footprint of which 1.6 % was ever walked) -- high-water marks + margin; nothing is allocated per step and the host never reads a
  size back: the list kernels, the statistics and Adam run under the library's step guard (`gs_guard_set`) -- a step whose lists
  outgrow the capacity is a device-side no-op, and so is every step queued behind it;
* the whole sequence is captured once into a hipGraph and replayed: per step the host enqueues the input
  copies, one tiny launch that carries Adam's bias corrections / learning rates as kernel arguments, and the
  graph;
* overflow is detected lazily and without any runtime call: the last launch of every step writes {I, max tile
  list, flags, applied-step count} into page-locked host memory the device can address, which the host polls as
  plain memory; the runner then grows the workspace, re-captures and replays the steps that were skipped, in
  order, with the inputs it kept for them -- the trajectory is exactly the one an unlimited workspace would
  have taken.  (Copy + event based polling between replays of the same graph faulted on this ROCm build.)

A change of N (densify_and_prune), of the parameter storage (reset_opacities), of the active SH degree or of
the image size re-builds the workspace and re-captures.

Training to a Gaussian budget (`mcmc=MCMCStrategy(..., noise="counter")`): the budget regulariser joins the loss total and the
gradients (gs_mcmc_reg / gs_project_bwd_adam_mcmc), and the noise runs behind Adam inside the guarded sequence with draws that are a
pure function of (seed, step, Gaussian) (gs_mcmc_noise_step) -- a skipped step that is replayed draws what it would have drawn.
Relocate / grow stay between the steps: `strategy.after_step(step, runner)`.

Refining camera poses (`poses=pose.CameraDeltas(n_views)`, `step(..., view_index=i)`): the corrected view matrix is composed on the
device in front of the projection (gs_pose_compose), the camera gradient is formed from the step's gradient rows beside the fused
kernel (gs_row_sums + gs_cam_grad_sums; gs_project_bwd_cam without fuse_adam), and one launch chains it to the view's 6-vector and
applies dense Adam to all corrections under the step guard (gs_pose_adam).  DESIGN.md "Poses in the captured step".

Compensating per-view exposure (`exposure=exposure.ExposureTable(n_views)`, `step(..., view_index=i)`): the view's 3x4 colour affine is
applied to the render in front of the loss (gs_exposure_apply), the loss gradient is taken back to the raw render in place while the
12 sums of the view's row are formed (gs_exposure_bwd), and one launch applies dense Adam to the whole table under the step guard
(gs_exposure_adam).  DESIGN.md "Exposure in the captured step".

Correcting per-view appearance (`bilagrid=bilagrid.BilateralGrids(n_views)`, `step(..., view_index=i)`): the view's bilateral grid of
colour affines is sliced and applied to the render in front of the loss (gs_bilagrid_apply), the loss gradient is taken back to the
raw render in place -- through the luminance guide too -- while the slice's adjoint fills the view's slab (gs_bilagrid_bwd), the
total variation of all grids enters the loss and the gradient (gs_bilagrid_tv), and one launch applies dense Adam to every grid
under the step guard (gs_bilagrid_adam).  DESIGN.md "Bilateral grids in the captured step".

Supervising depth (`depth=depth_loss.DepthSupervision(lambda_depth, mode)`, `gt_depth=t`, `step(..., gt_depth=t)`): the projection's
depth rides the blend as a fourth channel (gs_rec_depth, gs_blend_fwd_ch), one pass splits the [H,W,4] buffer into the image the loss
kernels read and the expected-depth map while it forms the depth term's sums (gs_depth_loss_split / _finish), one pass behind the
image loss's backward joins v_render and the depth term's gradient into the 4-channel blend backward's inputs (gs_depth_loss_join),
and the depth lane's gradient reaches the means through gs_depth_grads (gs_depth_grads_z + gs_project_bwd_adam_depth with fuse_adam).
DESIGN.md "Depth supervision in the captured step".
"""
from __future__ import annotations

import ctypes as ct
import math
import os
import time
from collections import deque
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _native as nat
from .optim import FusedAdam
from . import rendering
from . import workspace as WS
from .rendering import _SH_JAC, _sort_class


_TILE = nat.GS_TILE
# the projection parameters of the captured step, forward and backward: `rendering.rasterization()`'s defaults
EPS2D, NEAR_PLANE, FAR_PLANE, RADIUS_CLIP = 0.3, 0.01, 1e10, 0.0

# Name in `buf` -> (slot of the library's workspace layout, shape of the view; a str: a dimension of the call, see `_lay`).  (-1,) is all the
# layout gives the slot, 256-byte padding included: lengths only the library knows (scratch, slack words) -- read as a whole, garbage at the end.
_SLOTS = {
    "info": (WS.INFO, (nat.GS_INFO_WORDS,)), "rec": (WS.REC, ("N", nat.GS_REC_FLOATS)), "bbox": (WS.BBOX, ("N", 4)), "qcnt": (WS.QCNT, ("quads",)),
    "tiles_per_gauss": (WS.TILES_PER_GAUSS, (1, "N")), "cum_tiles": (WS.CUM_TILES, ("N",)), "colors_post": (WS.COLORS_POST, (1, "N", 3)),
    "isect_offsets": (WS.ISECT_OFFSETS, (-1,)), "bucket_offsets": (WS.BUCKET_OFFSETS, (-1,)), "tile_order": (WS.TILE_ORDER, ("tiles",)),
    "sh_jac": (WS.SH_JAC, (-1,)), "ws": (WS.BIN, (-1,)), "coarse_keys": (WS.COARSE_KEYS, ("cap_coarse",)), "keys_tmp": (WS.KEYS_TMP, ("cap",)),
    "slot_gid": (WS.SLOT_GID, ("cap",)), "flatten_ids": (WS.FLATTEN_IDS, ("cap",)), "slots": (WS.SLOTS, ("cap",)), "qmask": (WS.QMASK, (-1,)),
    "row_base": (WS.ROW_BASE, (-1,)), "walk_state": (WS.WALK_STATE, (-1,)), "ckpt": (WS.CKPT, ("cap_units", 64, 4)),
    "qlist": (WS.QLIST, ("cap_units", nat.GS_UNIT, 2)), "unit_desc": (WS.UNIT_DESC, ("cap_units", 4)), "rows": (WS.ROWS, ("cap_rows", nat.GS_ROW_FLOATS))}


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _refuse_camera_grads(data) -> None:
    if data is not None and isinstance(data.get("w2c"), Tensor) and data["w2c"].requires_grad:
        raise ValueError("TrainStepGraph: data['w2c'] requires grad, but the captured step hands no camera gradient to autograd: "
                         "detach it and refine poses INSIDE the step -- TrainStepGraph(..., poses=pose.CameraDeltas(n_views)) with "
                         "step(..., view_index=i) and the uncorrected data['w2c'] -- or in the eager loop (model(data) with "
                         "pose.CameraDeltas)")


def _pose_view(poses, view_index, exposure=None, bilagrid=None) -> Optional[int]:
    """The view a step refines, validated before anything reaches the device: required with `poses`, `exposure` or `bilagrid` (one
    index for all), refused without."""
    if poses is None and exposure is None and bilagrid is None:
        if view_index is not None:
            raise ValueError("TrainStepGraph.step: view_index given, but the runner was built without `poses` and without `exposure`")
        return None
    if view_index is None:
        if poses is None and exposure is None:
            raise ValueError("TrainStepGraph.step: the runner corrects appearance (bilagrid=BilateralGrids): every step needs view_index=i, "
                             "the grid of `bilagrid.grids` that belongs to the step's target image")
        if poses is None:
            raise ValueError("TrainStepGraph.step: the runner compensates exposure (exposure=ExposureTable): every step needs view_index=i, "
                             "the row of `exposure.affine` that belongs to the step's target image")
        raise ValueError("TrainStepGraph.step: the runner refines poses (poses=CameraDeltas): every step needs view_index=i, the row of "
                         "`poses.deltas` that corrects data['w2c']")
    i = int(view_index)
    for what, owner, table in (("poses", poses, "deltas"), ("exposure", exposure, "affine"), ("bilagrid", bilagrid, "grids")):
        if owner is not None and not 0 <= i < int(getattr(owner, table).shape[0]):
            raise ValueError(f"TrainStepGraph.step: view_index {i} outside the {int(getattr(owner, table).shape[0])} views of `{what}`")
    return i


# The variants of the fused projection backward + Adam exist one at a time: (option, the entry or kernel that a combination with it
# lacks), in the order in which the refusals fire.  `{where}`: the non-default setting the option was combined with.
_ONE_VARIANT = (
    ("`mcmc`", "the fused projection backward + Adam with the budget regulariser (gs_project_bwd_adam_mcmc: project_bwd_budget_kernel) "
               "does not exist {where} yet"),
    ("`poses`", "the fused projection backward + Adam from the row sums and the camera gradient from them (gs_project_bwd_adam_sums, "
                "gs_cam_grad_sums: project_cam_kernel<DEG, SUMS = true>) do not exist {where} yet; refine poses in the eager loop "
                "(rasterization(..., _camera_grads=True))"),
    ("`depth`", "the fused projection backward + Adam with the depth gradient (gs_project_bwd_adam_depth: project_bwd_depth_kernel) "
                "does not exist {where} yet"),
    ("rounds='on'", "one depth round only: the fused projection backward over the two row ranges of a two-round step (project_bwd_kernel "
                    "with ProjBwdArgs.rblk) is not instantiated {where} yet"))
# What is non-default -> (where its variant stands, what it cannot be combined with)
_REFUSED = {
    "camera_model": ("for this camera model", _ONE_VARIANT),
    "rasterize_mode": ("in the antialiased mode", (("camera_model", "the antialiased projection and its fused backward + Adam (gs_project_fwd_aa, "
                                                    "gs_project_bwd_adam_aa: project_bwd_aa_kernel) exist for the pinhole model only"),) + _ONE_VARIANT),
    "depth": ("", (("`poses`", "the camera gradient of the depth term is not formed inside the captured step; supervise depth on fixed "
                               "cameras, or refine poses in the eager loop"),
                   ("rounds='on'", "the depth lane's gradient gather is one-round only (gs_rec_depth / gs_depth_grads); leave rounds at "
                                   "'auto' (it resolves to off) or 'off'")))}


# `visible_adam`: (what it was combined with, the variant of the selective kernel that would serve it), in the order the refusals fire
_NO_SELECTIVE = (("`mcmc`", "budget-regulariser (project_bwd_budget_kernel)"), ("`poses`", "row-sums (project_bwd_kernel<.., SUMS = true>)"),
                 ("`depth`", "depth-gradient (project_bwd_depth_kernel)"), ("camera_model", "camera-model (project_bwd_cm_kernel)"),
                 ("rasterize_mode", "antialiased (project_bwd_aa_kernel)"))


def _refuse_combinations(model, camera_model, rasterize_mode, mcmc, poses, depth, rounds, visible_adam: bool = False) -> str:
    """TrainStepGraph(camera_model=..., rasterize_mode=..., depth=...): validates the three, resolves the mode against the model's
    attribute and refuses, before any device work, what `_REFUSED` lists for each that is not at its default.  Returns the mode."""
    given = {"camera_model": camera_model != "pinhole", "`mcmc`": mcmc is not None, "`poses`": poses is not None, "`depth`": depth is not None,
             "rounds='on'": rounds == "on"}

    def refuse(setting: str, what: str) -> None:
        where, options = _REFUSED[setting]
        for option, missing in options:
            if given[option]:
                option = f"camera_model={camera_model!r}" if option == "camera_model" else option
                raise ValueError(f"TrainStepGraph({what}) with {option} -- " + missing.format(where=where))

    if camera_model not in rendering.CAMERA_MODELS:
        raise ValueError(f"TrainStepGraph: camera_model: one of {sorted(rendering.CAMERA_MODELS)} (got {camera_model!r})")
    if camera_model != "pinhole":
        refuse("camera_model", f"camera_model={camera_model!r}")
    model_mode = getattr(model, "rasterize_mode", "classic")
    if rasterize_mode is None:
        rasterize_mode = model_mode
    if rasterize_mode not in rendering.RASTERIZE_MODES:
        raise ValueError(f"TrainStepGraph: rasterize_mode: one of {sorted(rendering.RASTERIZE_MODES)} (got {rasterize_mode!r})")
    if rasterize_mode != model_mode:   # (what model(data) would render with in the eager loop, and every evaluation of the model)
        raise ValueError(f"TrainStepGraph: the model's rasterize_mode is {model_mode!r}, but the runner was asked for "
                         f"rasterize_mode={rasterize_mode!r}; set model.rasterize_mode first")
    if rasterize_mode != "classic":
        refuse("rasterize_mode", "rasterize_mode='antialiased'")
    if depth is not None:
        from .depth_loss import DepthSupervision
        if not isinstance(depth, DepthSupervision):
            raise TypeError("TrainStepGraph(depth=...): a depth_loss.DepthSupervision")
        refuse("depth", "depth=...")
    if visible_adam:
        given.update({"rasterize_mode": rasterize_mode != "classic"})
        for option, variant in _NO_SELECTIVE:
            if given[option]:
                option = {"camera_model": f"camera_model={camera_model!r}", "rasterize_mode": "rasterize_mode='antialiased'"}.get(option, option)
                raise ValueError(f"TrainStepGraph(visible_adam=True) with {option} -- the fused projection backward + Adam over the visible "
                                 f"Gaussians (gs_project_bwd_selective: project_bwd_selective_kernel) has no {variant} variant yet")
    return rasterize_mode


@dataclass(slots=True)
class _Pending:
    """One step as it is queued: what `_stage_inputs` hands to the device in front of the graph, and what an overflow recovery
    replays.  `self.pending` holds the steps issued but not yet confirmed applied; `self._staged` is the one staged last -- the
    defaults of a later `step()` that brings no `data`, `gt_img` or `gt_depth`.  Inputs are kept by reference (`step`)."""
    t: int                       # Adam's step count
    lrs: List[float]             # the learning rates of the optimizer's groups as they stood at the call
    w2c: Tensor
    K: Tensor
    gt: Tensor                   # the target image: the tensor the loss kernels read in place, kept alive until the step is applied
    mask: Optional[Tensor]
    inputs_ready: bool = False   # `step(inputs_ready=)`
    conv: Any = None             # an event behind the runner's own conversion / copy of a target on the caller's stream
    ready_event: Any = None      # `step(ready_event=)`
    host_src: Any = None         # `step(host_src=)`
    # the per-feature values a replay re-stages like t and the learning rates; None: the runner was built without the feature
    pose: Optional[Tuple[int, int]] = None               # (view, pose step count)
    exposure: Optional[Tuple[int, int, float]] = None    # (view, exposure step count, learning rate)
    bilagrid: Optional[Tuple[int, int, float]] = None    # (view, the grids' step count, learning rate)
    depth: Optional[Tuple[Tensor, float]] = None         # (target, lambda_depth)


class TrainStepGraph:
    poses = exposure = bilagrid = depth = mcmc = None   # the optional features: off until the constructor is handed one

    def __init__(self, model, optimizer: FusedAdam, loss_computer, data: Dict[str, Any], gt_img: Tensor,
                 mask: Optional[Tensor] = None, margin: float = 1.3, use_graph: bool = True, check_every: int = 16,
                 fuse_adam: bool = True, handback: str = "eager", copy_targets: bool = False, rounds: str = "auto",
                 round_fraction: float = 0.125, mcmc=None, mcmc_reg: Tuple[float, float] = (0.01, 0.01), poses=None,
                 pose_lr: float = 1e-3, pose_betas: Tuple[float, float] = (0.9, 0.999), pose_eps: float = 1e-15, exposure=None,
                 exposure_lr: float = 1e-2, exposure_betas: Tuple[float, float] = (0.9, 0.999), exposure_eps: float = 1e-15, bilagrid=None,
                 bilagrid_lr: float = 2e-3, bilagrid_betas: Tuple[float, float] = (0.9, 0.999), bilagrid_eps: float = 1e-15,
                 bilagrid_tv: float = 10.0, depth=None, gt_depth: Optional[Tensor] = None, camera_model: str = "pinhole",
                 rasterize_mode: Optional[str] = None, visible_adam: bool = False):
        """`mcmc`: an `mcmc.MCMCStrategy(model, ..., noise="counter")` -- the step then trains under its Gaussian budget: `mcmc_reg` =
        (opacity_reg, scale_reg) of `strategy.regularization()` enters the loss (out["mcmc_reg"]) and the update, and the strategy's
        noise runs behind Adam inside the step, at noise_lr x the means learning rate of that step.  None (default): nothing changes.
        `handback`: when the caller's stream is ordered behind a step.
        "eager" (default): on return from every `step()` -- whatever the caller enqueues next (a read of the outputs, an eval
        render that reads the parameters, `densify_and_prune`) sees the finished step, no thought required.
        "lazy": only when the caller touches the returned outputs (`out["loss3"]`, ...), calls `fence()` or `finish()`.
        A loop that looks at nothing between steps then leaves its own stream idle, and the wait every step performs on
        entry (below) costs nothing; with the eager form that wait sits behind the previous step's hand-back on the caller's
        stream -- two cross-queue signal hops, 24 us of idle GPU per step in the kernel trace of the bench loop.  Parameters
        and statistics are NOT intercepted: a lazy caller that reads them between steps calls `fence()` first.
        `poses`: a `pose.CameraDeltas(n_views)` on the runner's device -- the step then refines the cameras: `data["w2c"]` is the
        UNCORRECTED matrix, `step(..., view_index=i)` names the row of `poses.deltas` that corrects it (the build's own view:
        `data.get("view_index", 0)`), the step renders with the corrected matrix (out["viewmat"]), and behind the model's update one
        launch chains the camera gradient to that row (out["v_delta"]) and applies Adam(pose_lr, pose_betas, pose_eps) to ALL rows in
        place in `poses.deltas.data` -- `torch.optim.Adam(poses.parameters())`'s dense update: idle rows decay their moments and
        move -- under the step guard.  The moments and the pose step count: `runner.pose_state` (`pose.PoseAdamState`, with
        `state_dict` / `load_state_dict`).  `poses.deltas` must keep its storage while the runner lives.  None (default): nothing
        changes, launch for launch.
        `data["w2c"]` itself never requires grad here: one that does raises `ValueError` (here and in `step`) -- the captured step
        hands nothing to autograd (INTEGRATION.md "Refining camera poses").
        `exposure`: an `exposure.ExposureTable(n_views)` on the runner's device -- the step then compensates per-view exposure:
        `step(..., view_index=i)` names the row of `exposure.affine` (the same index `poses` uses when both are given), the loss reads
        the affine of that row applied to the un-clamped render (out["exposed"]), the gradient of the raw render is A^T times the loss
        gradient, and beside the pose update one launch applies Adam(exposure_lr, exposure_betas, exposure_eps) to ALL rows in place in
        `exposure.affine.data` -- the 12 sums of the step (out["v_affine"]) on the view's row, zeros on the others -- under the step
        guard.  `runner.exposure_lr` is a plain attribute, staged every step outside the graph: a schedule is an assignment between
        steps.  The moments and the step count: `runner.exposure_state` (`exposure.ExposureAdamState`).  `exposure.affine` must keep
        its storage while the runner lives.  None (default): nothing changes, launch for launch.
        `bilagrid`: a `bilagrid.BilateralGrids(n_views)` on the runner's device -- the step then corrects per-view appearance:
        `step(..., view_index=i)` names the grid (the same index `poses` uses), the loss reads the slice of that grid applied to the
        un-clamped render (out["exposed"]) plus `bilagrid_tv` times the total variation of ALL grids (out["bilagrid_tv"]), the
        gradient of the raw render includes the part through the luminance guide, and beside the pose update one launch applies
        Adam(bilagrid_lr, bilagrid_betas, bilagrid_eps) to every element of `bilagrid.grids.data` with the step's dense gradient
        (out["v_grids"]: the slice's adjoint on the view's slab plus the TV gradient everywhere) under the step guard.
        `runner.bilagrid_lr` is a plain attribute, staged every step outside the graph.  The moments and the step count:
        `runner.bilagrid_state` (`bilagrid.BilagridAdamState`).  `bilagrid.grids` must keep its storage while the runner lives.  Not
        together with `exposure` (`ValueError`): two colour models in front of one loss.  None (default): nothing changes, launch
        for launch.
        `depth`: a `depth_loss.DepthSupervision(lambda_depth, mode)` -- the step then supervises the expected depth of its render
        (gsplat's RGB+ED) against `gt_depth`, a float32 [H, W] map on the runner's device in which zero, negative, NaN and inf pixels
        mean "no measurement": `lambda_depth * depth_loss` joins the loss total (out["depth_loss"]: the unweighted value;
        out["render_depth"]: the expected-depth map [H, W]), under the step's mask when it has one, and its gradient reaches the means,
        the opacities and the 2-D geometry through a 4-channel blend backward.  `step(..., gt_depth=t)` hands a step its target: read
        in place, defaulting to the previous step's, cloned under `copy_targets=True`, and kept by the pending entry so that an
        overflow recovery replays a skipped step with its own -- the rules of `gt_img`.  `runner.lambda_depth` is a plain attribute,
        staged every step outside the graph.  Works with a mask, the scale regulariser, `mcmc`, `exposure` and `bilagrid` (which read
        and write the 3-channel image and its gradient as always).  Refused before any device work: a missing `gt_depth` or one of
        another shape (`ValueError`); `rounds="on"` (`ValueError`: the depth lane's gather is one-round only; "auto" resolves to off);
        `poses` (`ValueError`: the camera gradient of the depth term is not formed); `ViewParallelGraphStep` (`ValueError`);
        `HostFeed` on such a runner (`NotImplementedError`).  None (default): nothing changes, launch for launch.
        `camera_model`: "pinhole" (default: nothing changes, launch for launch), "ortho" or "fisheye" (`rasterization(camera_model=...)`)
        -- the step then projects with gs_project_fwd_cm and updates with gs_project_bwd_adam_cm / gs_project_bwd_adam_reg_cm.  Works
        with a mask, the scale regulariser, `exposure`, `bilagrid` and `HostFeed` (none of them touches the projection backward), always
        in one depth round ("auto" resolves to off).  Refused before any device work (`ValueError`): `mcmc`, `poses`, `depth`,
        `rounds="on"` and `ViewParallelGraphStep` -- each needs a variant of the fused projection backward that exists for the
        pinhole model only.
        `rasterize_mode`: None (default: the model's `rasterize_mode` attribute), "classic" (nothing changes, launch for launch) or
        "antialiased" (`rasterization(rasterize_mode=...)`); a value other than the model's attribute raises `ValueError` -- the model
        renders its evaluations with the attribute.  The antialiased step projects with gs_project_fwd_aa and updates with
        gs_project_bwd_adam_aa / gs_project_bwd_adam_reg_aa.  Works with a mask, the scale regulariser, `exposure`, `bilagrid` and
        `HostFeed`, always in one depth round ("auto" resolves to off).  Refused before any device work (`ValueError`): `mcmc`, `poses`,
        `depth`, `rounds="on"`, a camera model other than pinhole and `ViewParallelGraphStep` -- each needs a variant of the fused
        projection backward that exists for the classic mode only.
        `visible_adam`: True -- the step updates only the Gaussians it SAW, `radii > 0` under the step's camera (gsplat's
        `visible_adam`; DESIGN.md "Updating only what a step saw"): a seen Gaussian receives the dense update, bias corrections from the
        one step count included; a culled one keeps the bits of its six parameters and of both moments -- no decay, no move along a
        stale first moment, no scale-regulariser term.  The loss values in `out`, the statistics and the step guard are the dense
        step's.  With `fuse_adam` the step updates with gs_project_bwd_selective, without it with gs_adam_step_visible_dev on the step's
        radii.  Works with a mask, the scale regulariser, `exposure`, `bilagrid`, `HostFeed`, `rounds` in any setting and a re-capture
        after a refinement.  Refused before any device work (`ValueError`): `mcmc`, `poses`, `depth`, a camera model other than
        pinhole, `rasterize_mode="antialiased"` and `ViewParallelGraphStep` -- each needs a selective variant of its own fused kernel.
        False (default): nothing changes, launch for launch."""
        rounds = os.environ.get("GS_TG_ROUNDS", rounds)
        self.visible_adam = bool(visible_adam)
        self.antialiased = _refuse_combinations(model, camera_model, rasterize_mode, mcmc, poses, depth, rounds, self.visible_adam) == "antialiased"
        self.camera_model = rendering.CAMERA_MODELS[camera_model]
        self.depth = depth
        if depth is not None:
            from .depth_loss import MODES
            if gt_depth is None:
                raise ValueError("TrainStepGraph(depth=...): the runner needs its first target, gt_depth=[H, W] float32")
            if tuple(gt_depth.shape) != (int(data["height"]), int(data["width"])):
                raise ValueError(f"TrainStepGraph(depth=...): gt_depth of shape {tuple(gt_depth.shape)}, expected "
                                 f"{(int(data['height']), int(data['width']))}")
            self.lambda_depth, self._depth_mode = float(depth.lambda_depth), MODES.index(depth.mode)
        if bilagrid is not None:
            from .bilagrid import BilagridAdamState, BilateralGrids
            if exposure is not None:
                raise ValueError("TrainStepGraph: `exposure` and `bilagrid` together -- two colour models in front of one loss are ambiguous; "
                                 "a bilateral grid contains the global affine")
            if not isinstance(bilagrid, BilateralGrids):
                raise TypeError("TrainStepGraph(bilagrid=...): a bilagrid.BilateralGrids")
            g = bilagrid.grids
            if g.device != model.means.device or g.dtype != torch.float32 or not g.is_contiguous() or g.dim() != 5 or g.shape[1] != 12:
                raise ValueError("TrainStepGraph(bilagrid=...): `bilagrid.grids` must be a contiguous float32 [n_views, 12, L, Hg, Wg] on the "
                                 "model's device")
            if not 1 <= g.shape[0] <= nat.GS_BILAGRID_MAX_VIEWS:
                raise ValueError("TrainStepGraph(bilagrid=...): 1 .. GS_BILAGRID_MAX_VIEWS views")
            self.bilagrid_lr, self.bilagrid_eps, self.bilagrid_tv = float(bilagrid_lr), float(bilagrid_eps), float(bilagrid_tv)
            self.bilagrid_betas = (float(bilagrid_betas[0]), float(bilagrid_betas[1]))
            self.bilagrid_state = BilagridAdamState(bilagrid)
            # runner-owned, outside the workspace layout, alive across re-builds: the record, the view's slab, the dense gradient, the
            # TV value and its scratch (the image and the partials are sized by the frame: `_build`)
            f32g = dict(dtype=torch.float32, device=g.device)
            self._bilagrid_bufs = {"bilagrid_rec": torch.zeros((nat.GS_BILAGRID_REC_FLOATS,), **f32g),
                                   "v_slab": torch.zeros(tuple(g.shape[1:]), **f32g), "v_grids": torch.zeros(tuple(g.shape), **f32g),
                                   "bilagrid_tv": torch.zeros((1,), **f32g),
                                   "bilagrid_tv_ws": torch.zeros((nat.GS_BILAGRID_TV_DOUBLES,), dtype=torch.float64, device=g.device)}
        self.bilagrid = bilagrid
        if exposure is not None:
            from .exposure import ExposureAdamState, ExposureTable
            if not isinstance(exposure, ExposureTable):
                raise TypeError("TrainStepGraph(exposure=...): an exposure.ExposureTable")
            a = exposure.affine
            if a.device != model.means.device or a.dtype != torch.float32 or not a.is_contiguous() or tuple(a.shape[1:]) != (3, 4):
                raise ValueError("TrainStepGraph(exposure=...): `exposure.affine` must be a contiguous float32 [n_views, 3, 4] on the model's device")
            if not 1 <= a.shape[0] <= nat.GS_EXPOSURE_MAX_VIEWS:
                raise ValueError("TrainStepGraph(exposure=...): 1 .. GS_EXPOSURE_MAX_VIEWS views")
            self.exposure_lr, self.exposure_eps = float(exposure_lr), float(exposure_eps)
            self.exposure_betas = (float(exposure_betas[0]), float(exposure_betas[1]))
            self.exposure_state = ExposureAdamState(exposure)
            # runner-owned, outside the workspace layout, alive across re-builds: the record and the 12 sums (the image and the
            # partials are sized by the frame: `_build`)
            self._exposure_bufs = {"exposure_rec": torch.zeros((nat.GS_EXPOSURE_REC_FLOATS,), dtype=torch.float32, device=a.device),
                                   "v_affine": torch.zeros((12,), dtype=torch.float32, device=a.device)}
        self.exposure = exposure
        if poses is not None:
            from .pose import CameraDeltas, PoseAdamState
            if not isinstance(poses, CameraDeltas):
                raise TypeError("TrainStepGraph(poses=...): a pose.CameraDeltas")
            d = poses.deltas
            if d.device != model.means.device or d.dtype != torch.float32 or not d.is_contiguous() or d.dim() != 2 or d.shape[1] != 6:
                raise ValueError("TrainStepGraph(poses=...): `poses.deltas` must be a contiguous float32 [n_views, 6] on the model's device")
            if not 1 <= d.shape[0] <= nat.GS_POSE_MAX_VIEWS:
                raise ValueError("TrainStepGraph(poses=...): 1 .. GS_POSE_MAX_VIEWS views")
            self.pose_lr, self.pose_betas, self.pose_eps = float(pose_lr), (float(pose_betas[0]), float(pose_betas[1])), float(pose_eps)
            self.pose_state = PoseAdamState(poses)
            # runner-owned, outside the workspace layout, alive across re-builds: the record (its first 16 floats: the raw view matrix,
            # the step's static camera input), the camera gradient and the 6-vector's
            f32d = dict(dtype=torch.float32, device=d.device)
            self._pose_bufs = {"pose_rec": torch.zeros((nat.GS_POSE_REC_FLOATS,), **f32d), "v_viewmats": torch.zeros((1, 4, 4), **f32d),
                               "v_campos": torch.zeros((1, 3), **f32d), "v_delta": torch.zeros((6,), **f32d)}
        self.poses = poses
        # (option, prefix of its `<prefix>_lr` / `<prefix>_state`, table, Adam state) of the per-view tables the step updates
        self._tables = [(option, prefix, getattr(owner, table), getattr(self, prefix + "_state")) for option, prefix, owner, table in
                        (("poses", "pose", poses, "deltas"), ("exposure", "exposure", exposure, "affine"), ("bilagrid", "bilagrid", bilagrid, "grids"))
                        if owner is not None]
        build_view = _pose_view(poses, data.get("view_index", 0) if self._tables else None, exposure, bilagrid)   # the build's own view
        self.mcmc = mcmc
        if mcmc is not None:
            if getattr(mcmc, "noise", None) != "counter":
                raise ValueError("TrainStepGraph(mcmc=...): the strategy must draw counter-based noise, MCMCStrategy(..., noise='counter') -- "
                                 "a skipped step that is replayed has to draw the normals it would have drawn")
            if mcmc.model is not model:
                raise ValueError("TrainStepGraph: the MCMCStrategy works on another model than the one the runner trains")
            self.mcmc_reg = (float(mcmc_reg[0]), float(mcmc_reg[1]))
        _refuse_camera_grads(data)
        if data.get("camera_model", camera_model) != camera_model:   # (what model(data) would render with in the eager loop)
            raise ValueError(f"TrainStepGraph: data['camera_model'] is {data['camera_model']!r}, but the runner was asked for "
                             f"camera_model={camera_model!r}")
        if handback not in ("eager", "lazy"):
            raise ValueError("handback: 'eager' or 'lazy'")
        self.handback = handback
        # rounds: depth rounds of the list stages (include/gs_raster.h "Depth rounds": the front slab of the frame is listed, sorted
        # and blended first, the rest only into tiles it has not finished; same images, sublists and gradient rows bit for bit).
        # "auto" (default): on when the build-time probe finds that the frame lists several times what its blend walks
        # (realistic footprints: 20-50 x) -- the two-round pipeline costs ~0.1 ms of extra launches, which a scene that walks most
        # of what it lists never earns back; "on" / "off" force it.  round_fraction: the share of the listed intersections in
        # front of the depth split.
        if rounds not in ("auto", "on", "off"):   # (GS_TG_ROUNDS in the environment overrides the argument: read at the top)
            raise ValueError("rounds: 'auto', 'on' or 'off'")
        self.rounds_mode, self.round_fraction = rounds, float(os.environ.get("GS_TG_ROUND_FRACTION", round_fraction))
        if (depth is not None or self.camera_model != nat.GS_CAMERA_PINHOLE or self.antialiased) and rounds == "auto":
            rounds = self.rounds_mode = "off"   # (one round: see `depth`, `camera_model`, `rasterize_mode`)
        self.rounds_on = rounds == "on"
        self._live_sum = self._live_n = 0   # tiles the front round left live, summed over the polled steps since the last build
        # "auto" only: the captured step holds the FRONT round alone (gs_rounds_set phase 4), speculating that it finishes every
        # frame -- a hipGraph cannot skip the ~18 launches of a back round that has nothing to do (0.09 ms).  A frame that does
        # leave tiles live voids its step on the device (GS_FLAG_BACK) like a capacity overflow; the runner then re-builds with
        # both rounds and replays.
        self.front_only = False
        # copy_targets: every step takes a private copy of its target image (and mask) instead of reading the caller's tensors in
        # place -- for loaders that recycle ONE device staging buffer (`gt_buf.copy_(next)`): a target is read until its step is
        # RETIRED (the loss forward and backward of the replay, and again if an overflow recovery replays the step up to
        # `check_every` steps later), not only until `step()` returns.  Costs the copy the in-place read saved (25 MB at 1080p).
        self.copy_targets = bool(copy_targets)
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("TrainStepGraph drives optim.FusedAdam (flat parameter / moment buffers)")
        if not getattr(loss_computer, "clamp_input", False) or not getattr(loss_computer, "fused", True):
            raise ValueError("TrainStepGraph needs LossComputer(fused=True, clamp_input=True)")
        # the scale-ratio regulariser (LossComputer(model=..., lambda_scale=...) with use_scale_regularization): its value joins the
        # loss total and its gradient the log-scales' (gs_scale_reg / gs_project_bwd_adam_reg); R and lambda are read once, here
        self.scale_reg = getattr(loss_computer, "model", None) is not None and bool(getattr(model, "USE_SCALE_REGULARIZATION", False))
        if self.scale_reg:
            if loss_computer.model is not model:
                raise ValueError("TrainStepGraph: the LossComputer regularises another model than the one it trains")
            r = model.MAX_SCALE_RATIO
            self.max_scale_ratio = float(r.detach().cpu()) if isinstance(r, Tensor) else float(r)   # (a 0-d tensor from a checkpoint)
            self.lambda_scale = float(loss_computer.lambda_scale)
        self.model, self.opt, self.lc = model, optimizer, loss_computer
        self.margin, self.use_graph, self.check_every = float(margin), bool(use_graph), int(check_every)
        # fuse_adam: gs_project_bwd_adam -- the projection / SH backward applies Adam in place where each gradient is
        # formed (no gradient tensors, no separate optimizer pass); same update bit for bit
        self.fuse_adam = bool(fuse_adam)
        self.dev = model.means.device
        self.W, self.H = int(data["width"]), int(data["height"])
        self.has_mask = mask is not None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        # The step runs on a stream of its own, fenced against the caller's current stream on both sides.  (Replays on
        # the legacy NULL stream -- torch's default -- interleaved with other work on that stream end in GPU memory
        # faults on this ROCm build; DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 also avoids them.  A dedicated stream does not
        # need the runtime knob.)
        self.stream = torch.cuda.Stream(self.dev)
        self.cap = 0
        self.cap_units = self.cap_rows = 0   # capacities of what the forward walks: work units (storage units), gradient rows
        self.cap_floor = 0   # capacity carried over a rebuild: the probe sees ONE view, the steps before saw them all
        self.walk_floor = (0, 0)
        self.seen_isects = 0  # largest intersection count the status words have shown since the last (re-)build
        self.seen_tile = 0    # ... and the longest tile list
        self.seen_units = self.seen_rows = 0   # ... and the most storage units / gradient rows a step's walk took
        self.probed_walk = (0, 0)
        self._walk_history_void = False
        self.binning = None
        self.probed = (0, 0)
        self.cap_tile = _sort_class(0)
        self.pending: deque = deque()     # steps issued but not yet confirmed applied: `_Pending` records
        # {I, n_buckets, max tile, flags, applied} of the latest finished step, written by the device (gs_step_status)
        self.status = torch.zeros((8,), dtype=torch.int64, pin_memory=True)
        self.confirmed = 0                # steps known to be applied
        self.issued = 0
        self.stats = {"captures": 0, "overflows": 0, "replayed_steps": 0, "rebuilds": 0}
        self._pool: Dict[str, Tensor] = {}
        self.lease = WS.Lease(None, self.dev)   # private, never in `workspace.pool`: the graph bakes its addresses in
        self._warm = set()     # (binning mode, tile-sort class) pairs that have run EAGERLY in this runner (warm-up steps)
        self._key = None
        self.confirmed_at_build = 0
        if depth is not None:
            # runner-owned, alive across re-builds: the record {lambda, mode, target address, value, 1 / sum(w)}
            self._depth_bufs = {"depth_rec": torch.zeros((nat.GS_DEPTH_REC_FLOATS,), dtype=torch.float32, device=self.dev)}
        # the build's own step: the view of `data`, each table's step count + 1 and its rate, the first depth target and its weight
        self._build(self._next_step(data["w2c"], data["K"], gt_img, mask,
                                    pose=(build_view, self.pose_state.step + 1) if poses is not None else None,
                                    exposure=(build_view, self.exposure_state.step + 1, self.exposure_lr) if exposure is not None else None,
                                    bilagrid=(build_view, self.bilagrid_state.step + 1, self.bilagrid_lr) if bilagrid is not None else None,
                                    depth=(self._depth_image(gt_depth, (self.H, self.W)), self.lambda_depth) if depth is not None else None))

    # ------------------------------------------------------------------------------------------ workspace
    def _state_key(self, W: Optional[int] = None, H: Optional[int] = None):
        """What the captured graph is specialised on.  `W` / `H`: the size of the frame about to be rendered (the
        reference takes it per frame from `Frame.to_data`, e.g. multi-camera COLMAP sets); default = the built size."""
        m = self.model
        return (m.means.shape[0], self.opt.flat_param.data_ptr(), m.max_radii.data_ptr(), m.grad_norm_accum.data_ptr(),
                m.collecting_counts.data_ptr(), m.active_sh_degree, getattr(m, "tile_culling", "tight"),
                self.W if W is None else int(W), self.H if H is None else int(H))

    def _lrs(self) -> List[float]:
        return [float(grp["lr"]) for grp, _ in self.opt._plist]

    def _next_step(self, w2c: Tensor, K: Tensor, gt: Tensor, mask: Optional[Tensor], **staged) -> _Pending:
        """The record a (re-)build stages for its probe and warm-up: the step that would come next, at t = the optimizer's step
        count + 1 and the learning rates as they stand -- consumed by nobody."""
        return _Pending(max(self.opt._step, 0) + 1, self._lrs(), w2c, K, gt, mask if self.has_mask else None, **staged)

    def _build(self, staged: _Pending, min_cap: int = 0, min_cap_tile: int = 0, projected=None, min_walk=(0, 0)):
        """(Re-)allocates the workspace for the model as it is now, stages `staged`, learns the capacities from one blocking probe
        of the list sizes if needed, warms every kernel up eagerly and captures the step.
        `projected` = (I, longest tile list, storage units, gradient rows) carried over from the steps before a refinement (`step()`): no probe, no
        warm-up step -- the re-build is allocation + capture and never touches the device's queue.  (A projection that
        does not hold trips the step guard like any overflow; `_recover` then probes.)"""
        m, dev, L = self.model, self.dev, nat.lib()
        t_build = time.perf_counter()
        self.N = N = m.means.shape[0]
        self.K = 1 + m.sh_rest.shape[1]
        W, H = self.W, self.H
        self.tw, self.th = math.ceil(W / _TILE), math.ceil(H / _TILE)
        self.tiles = tiles = self.tw * self.th
        f32 = dict(dtype=torch.float32, device=dev)
        b = self.buf = {}
        b["viewmats"] = torch.empty((1, 4, 4), **f32)
        b["Ks"] = torch.empty((1, 3, 3), **f32)
        # {gt, mask} POINTERS of the step about to run (gs_step_inputs writes them, the loss entries read through them): the
        # target image of a step is the caller's own tensor -- kept alive by the pending entry --, never copied
        b["img_slots"] = torch.zeros((2,), dtype=torch.int64, device=dev)
        b["bg"] = m.BACKGROUND.detach().reshape(1, 3).to(dev, torch.float32).contiguous().clone()
        b["radii"] = self._take("radii", (1, N), torch.int32)
        b["means2d"] = self._take("means2d", (1, N, 2), torch.float32)
        b["depths"] = self._take("depths", (1, N), torch.float32)
        b["conics"] = self._take("conics", (1, N, 3), torch.float32)
        b["applied"] = torch.zeros((1,), dtype=torch.int64, device=dev)
        b["render_colors"] = torch.empty((1, H, W, 3), **f32)
        b["render_alphas"] = torch.empty((1, H, W, 1), **f32)
        b["loss_ws"] = torch.empty((int(L.gs_loss_workspace_floats(H, W)),), **f32)
        b["loss3"] = torch.zeros((3,), **f32)
        b["loss_ring"] = torch.zeros((self.LOSS_RING, 3), **f32)
        b["one"] = torch.ones((), **f32)
        b["v_render"] = torch.empty((H, W, 3), **f32)
        b["v_abs"] = self._take("v_abs", (1, N, 2), torch.float32)
        self.grads = None if self.fuse_adam else {
            "means": torch.empty((N, 3), **f32), "log_scales": torch.empty((N, 3), **f32),
            "quats": torch.empty((N, 4), **f32), "sh_0": torch.empty((N, 1, 3), **f32),
            "sh_rest": torch.empty((N, self.K - 1, 3), **f32) if self.K > 1 else None,
            "logit_opacities": torch.empty((N,), **f32)}
        b["hyper"] = torch.zeros((16,), **f32)
        if self.antialiased:   # gs_project_fwd_aa's rho per Gaussian (nothing in the step reads it back: the backward recomputes the chain)
            b["compensations"] = self._take("compensations", (1, N), torch.float32)
        if self.poses is not None:
            b.update(self._pose_bufs)
            b["w2c_raw"] = b["pose_rec"][:16].view(1, 4, 4)
            b["cam_partials"] = self._take("cam_partials", (int(L.gs_cam_partials_doubles(1, N)),), torch.float64)
            if self.fuse_adam:   # the camera kernel reads the row sums: the fused kernel writes no gradient tensor
                b["pose_row_sums"] = self._take("pose_row_sums", (N, 12), torch.float32)
                b["pose_v_pre"] = self._take("pose_v_pre", (N, 3), torch.float32)
            else:                # gs_project_bwd_cam's three gradient tensors
                b["v_means2d"] = self._take("pose_v_means2d", (1, N, 2), torch.float32)
                b["v_conics"] = self._take("pose_v_conics", (1, N, 3), torch.float32)
                b["v_colors_post"] = self._take("pose_v_colors_post", (1, N, 3), torch.float32)
        if self.exposure is not None:
            eb = self._exposure_bufs
            if "exposed" not in eb or tuple(eb["exposed"].shape) != (H, W, 3):   # (the first build, or another frame size)
                eb["exposed"] = torch.empty((H, W, 3), **f32)
                eb["exposure_partials"] = torch.empty((int(L.gs_exposure_partials_doubles(H, W)),), dtype=torch.float64, device=dev)
            b.update(eb)
        if self.bilagrid is not None:
            gb = self._bilagrid_bufs
            if "exposed" not in gb or tuple(gb["exposed"].shape) != (H, W, 3):   # (the first build, or another frame size)
                gl, gy, gx = (int(x) for x in self.bilagrid.grids.shape[2:])
                gb["exposed"] = torch.empty((H, W, 3), **f32)
                gb["bilagrid_partials"] = torch.empty((int(L.gs_bilagrid_partials_doubles(H, W, gx, gy, gl)),), dtype=torch.float64, device=dev)
            b.update(gb)
        if self.depth is not None:
            db = self._depth_bufs
            if "render_colors4" not in db or tuple(db["render_colors4"].shape) != (1, H, W, 4):   # (the first build, or another frame size)
                db["render_colors4"] = torch.empty((1, H, W, 4), **f32)   # the blend's output; render_colors: its split image
                db["render_depth"] = torch.empty((H, W), **f32)
                db["v_colors4"] = torch.empty((H, W, 4), **f32)
                db["v_alphas"] = torch.empty((H, W), **f32)
                db["depth_partials"] = torch.empty((int(L.gs_depth_loss_partials_doubles(H, W)),), dtype=torch.float64, device=dev)
            b.update(db)
            b["bg4"] = torch.cat([b["bg"], torch.zeros((1, 1), **f32)], dim=1).contiguous()   # background [bg, 0]
            if self.fuse_adam:   # v_z per Gaussian: gs_depth_grads_z -> gs_project_bwd_adam_depth
                b["v_depths"] = self._take("v_depths", (N,), torch.float32)
        # {reg, -, fp64 block partials}: the regulariser's value and its reduction scratch (gs_scale_reg)
        b["scale_reg"] = self._take("scale_reg", (int(L.gs_scale_reg_workspace_floats(N)),), torch.float32) if self.scale_reg else None
        if self.mcmc is not None:
            # {reg, -, fp64 block partials} of the budget regulariser (gs_mcmc_reg); {strength, step, seed} of the step's noise
            b["mcmc_reg"] = self._take("mcmc_reg", (int(L.gs_mcmc_reg_workspace_floats(N)),), torch.float32)
            b["mcmc_rec"] = torch.zeros((nat.GS_MCMC_REC_WORDS,), dtype=torch.int64, device=dev)
            self._means_seg = [grp["name"] for grp, _ in self.opt._plist].index("means")
        self._stage_inputs(staged)
        probe_walk = False
        front_before, self.front_only = self.front_only, False   # (the probes below run both rounds)
        if projected is not None:
            n_isects, max_tile, units, rows = projected
            self.cap = int(n_isects * self.margin) + 4096
            need_tile = int(max_tile * self.margin)
            self.cap_tile = _sort_class(need_tile)
            self.cap_units, self.cap_rows = int(units * self.margin) + 512, int(rows * self.margin) + 4096
            self.stats["projected_rebuilds"] = self.stats.get("projected_rebuilds", 0) + 1
        elif self.cap == 0 or min_cap or min_cap_tile or min_walk[0] or min_walk[1]:
            n_isects, max_tile = self._probe()
            self.probed = (n_isects, max_tile)
            self.cap = max(int(max(n_isects, min_cap) * self.margin) + 4096, self.cap, self.cap_floor)
            need_tile = max(int(max(max_tile, min_cap_tile) * self.margin), self.cap_tile)   # (same head-room as the lists)
            self.cap_tile = _sort_class(need_tile)
            probe_walk = True
        self._lay(1 if probe_walk else 0)   # (behind a probe the fixed arena stays as it is)
        self._alloc_rounds()
        if probe_walk:
            # what the forward WALKS on this view: one guarded forward on first-guess capacities, repeated with what it reports
            floor = (max(min_walk[0], self.walk_floor[0]), max(min_walk[1], self.walk_floor[1]))
            self.cap_units = max(self.cap_units, int(floor[0] * self.margin) + 512, self.cap // 64 + 4 * tiles + 512)
            self.cap_rows = max(self.cap_rows, int(floor[1] * self.margin) + 4096, self.cap // 8 + 4096)
            while True:
                self._alloc_walk()
                units, rows, fl = self._probe_walk()
                if not fl:
                    break
                self.cap_units = max(self.cap_units, int(units * self.margin) + 512)
                self.cap_rows = max(self.cap_rows, int(rows * self.margin) + 4096)
            self.probed_walk = (units, rows)
            # The probe saw ONE view.  The list capacity carries the history of all of them (cap_floor); the walk is scaled to
            # it -- and after an opacity reset, when the history of the walk is void (nothing saturates any more, how deep a
            # view walks is anybody's guess: 1.1 to 2.6 M rows over the six views of tests/test_gpu_train_graph.py's soak),
            # with twice the head-room until the next re-build has steps to go by.
            scale = max(1.0, (self.cap / self.margin) / max(n_isects, 1))
            wm = self.margin * (2.0 if self._walk_history_void else 1.0)
            self.cap_units = max(int(max(units * scale, floor[0]) * wm) + 512, 256)
            self.cap_rows = max(int(max(rows * scale, floor[1]) * wm) + 4096, 4096)
            self._walk_history_void = False
            if self.rounds_mode == "auto":
                # listed against walked: a gradient row is one (intersection, quadrant) pair some pixel took, 1.5 per walked entry
                self.rounds_on = n_isects >= self.ROUNDS_MIN_LISTED and n_isects >= self.ROUNDS_MIN_RATIO * max(rows, 1)
        elif self.rounds_mode == "auto" and self.rounds_on and self._live_n > 0 and self._live_sum > self.ROUNDS_MAX_LIVE * tiles * self._live_n:
            self.rounds_on = False   # (a re-build without a probe: the steps since the last build left too many tiles to the back round)
        self.front_only = bool(front_before and not probe_walk and self.rounds_on and self.rounds_mode == "auto" and self._live_sum == 0)
        self._alloc_walk()
        self._alloc_rounds()
        if probe_walk and self.rounds_mode == "auto" and self.rounds_on:
            # ... and only where the front slab finishes (nearly) the whole frame: a back round that has work pays the passes over
            # the footprints and the fixed costs of the list stages a second time -- with 38 % of the tiles still live the two-round
            # step is 4-9 % SLOWER than one round (tools/rounds_time.py heavy2Mwin), with 7 % it breaks even
            self._probe_walk()
            live = int(b["rounds"][nat.GS_ROUND_LIVE])
            self.stats["probed_live_tiles"] = live
            if live > self.ROUNDS_MAX_LIVE * tiles:
                self.rounds_on = False
            # (a probing re-build that follows a voided speculation -- `_recover` -- keeps both rounds until the next refinement)
            self.front_only = self.rounds_on and live == 0 and self.speculate_front and not self._back_needed
            self._back_needed = False
        self._live_sum = self._live_n = 0
        self._key = self._state_key()
        self._opacity_resets = getattr(m, "opacity_resets", 0)
        # eager warm-up of the guarded pipeline (raises every kernel attribute; also a functional check before capture)
        t_cap = time.perf_counter()
        self._capture(warm_up=projected is None)
        self.stats["rebuilds"] += 1
        now = time.perf_counter()
        self.stats["build_ms"] = round(self.stats.get("build_ms", 0.0) + 1e3 * (now - t_build), 2)        # whole (re-)builds, wall clock
        self.stats["capture_ms"] = round(self.stats.get("capture_ms", 0.0) + 1e3 * (now - t_cap), 2)    # ... of which warm-up + capture

    def _take(self, name: str, shape, dtype, shrink: bool = False) -> Tensor:
        """A buffer of the workspace from the runner's pool: re-used across re-builds while it fits, re-allocated with head-room
        when it does not (a model that has been refined once will be refined again: `densify_and_prune` grows N by 20-30 % per
        call, and a re-build that has to `hipMalloc` twenty-five new buffers cost 16 ms per refinement on some boxes of the
        pool against 1.3 ms of capture -- bench.py `real_loop`).  First build: exact sizes."""
        n = 1
        for d in shape:
            n *= int(d)
        t = self._pool.get(name)
        if shrink and t is not None and t.numel() > 2 * n + 4096:
            t = None   # (a first-guess buffer of the walk probe several times what the walk turned out to need: let it go)
        if t is None or t.dtype != dtype or t.numel() < n:
            slack = 1.0 if self.stats["rebuilds"] == 0 else 1.6
            t = torch.empty((int(n * slack) + 16,), dtype=dtype, device=self.dev)
            self._pool[name] = t
            self.stats["pool_allocs"] = self.stats.get("pool_allocs", 0) + 1
        return t[:n].view(*shape)

    def _lay(self, first: int):
        """Moves the lease onto the library's layout (gs_workspace_query) for the capacities as they stand, from arena `first` on -- 0: all, a
        build; 1: lists and walk (the fixed arena, and a projection in it, stay: its offsets depend on no capacity and no binning); 2: walk
        alone -- and refreshes `buf`'s views of those arenas (None: not in this layout).  The arenas come from `_take`, the runner's memory
        policy; the walk arena is let go for a smaller one only where the walk capacities are known: a probe lays placeholders first."""
        bins, st, lease = self.binning == "bins", self.stream.cuda_stream, self.lease
        lay = WS.Layout(1, self.N, self.W, self.H, self.cap, self.cap_coarse if bins else 0, self.bin_shift if bins else 0,
                        WS.F_TRAIN | (WS.F_TWO_LEVEL if bins else 0), max(self.cap_units, 256), self.cap_rows)
        if first == 2 and lay.key == lease.layout.key and self.buf.get("rows") is not None:
            return   # (laid by this build already)
        for which, nbytes in list(zip(("fixed", "lists", "walk"), lay.arena_bytes))[first:]:
            setattr(lease, which, self._take(which, (nbytes,), torch.uint8, shrink=which == "walk" and self.cap_rows > 0))
        if first == 0:
            with torch.cuda.device(self.dev):   # (validates, and zeroes the info block on the runner's stream -- unless it has seen these
                lease.bind(lay, st)             #  arenas and this layout before: the flags are sticky, so zeroed here in any case)
                lease.view(WS.INFO, nat.GS_INFO_WORDS).zero_()
        else:
            lease.grow_lists(lay, st) if first == 1 else lease.grow_walk(lay)
        dims = dict(N=self.N, tiles=self.tiles, quads=4 * self.tiles, cap=self.cap, cap_coarse=lay.key[5], cap_units=self.cap_units, cap_rows=self.cap_rows)
        for name, (slot, shape) in _SLOTS.items():
            if WS._arena(slot) >= first:
                self.buf[name] = None
                if lay.offsets[slot] >= 0 and (_SH_JAC or slot != WS.SH_JAC):   # (GS_SH_JAC=0 keeps the coefficient-staging backward)
                    shape, ext = [dims.get(d, d) for d in shape], lay.extent(slot) // WS._DTYPES[slot].itemsize
                    n = ext if shape == [-1] else math.prod(shape)
                    assert n <= ext, (name, shape)
                    self.buf[name] = lease.view(slot, n) if len(shape) == 1 else lease.view(slot, n).view(shape)

    def _alloc_walk(self):
        """What is sized by what the forward WALKS: a checkpoint, a sublist block and a descriptor per work unit, the gradient rows."""
        self.cap_units, self.cap_rows = max(int(self.cap_units), 256), max(int(self.cap_rows), 1)
        self._lay(2)
        if self.depth is not None:
            self.lease.ckpt_ext()   # (the fourth channel's checkpoint plane follows the walk: allocated here, never inside a capture)
        n_cls = int(nat.lib().gs_unit_classes_ints(self.cap_units, 1, self.W, self.H))   # (gs_blend_bwd's fill classes; GS_BWD_CLASSES=0: off)
        self.buf["unit_cls"] = self._take("unit_cls", (n_cls,), torch.int32, shrink=True) if rendering._BWD_CLASSES else None

    ROUNDS_MIN_LISTED = 4_000_000   # "auto": below this the list stages are too short for a second round to pay
    ROUNDS_MIN_RATIO = 4.0          # ... and so they are when the frame lists less than this many entries per gradient row
    ROUNDS_MAX_LIVE = 0.05          # ... and rounds stay off where the front slab leaves more than this share of the tiles live
    speculate_front = os.environ.get('GS_TG_FRONT_ONLY', '1') != '0'   # 0: "auto" never captures the front round alone
    _back_needed = False

    def _alloc_rounds(self):
        """Depth rounds: the round block, the tiles' liveness / pixel states / sublist records between the rounds, the footprints
        and per-Gaussian counts of the round at hand."""
        b, tiles = self.buf, self.tw * self.th
        if not self.rounds_on:
            return
        b["rounds"] = torch.zeros((nat.GS_ROUND_WORDS,), dtype=torch.int64, device=self.dev)
        b["depth_hist"] = torch.zeros((4096,), dtype=torch.int32, device=self.dev)
        b["tile_live"] = torch.zeros((tiles,), dtype=torch.uint8, device=self.dev)
        b["tile_state"] = self._take("tile_state", (tiles, 4, 64, 4), torch.float32)
        b["tile_rec"] = self._take("tile_rec", (tiles, 8), torch.int32)
        b["bbox_round"] = self._take("bbox_round", (self.N, 4), torch.int32)
        b["tpg_round"] = self._take("tpg_round", (1, self.N), torch.int32)

    def _rounds_phase(self, phase: int):
        L, b = nat.lib(), self.buf
        if phase == 0:
            nat.check(L.gs_rounds_set(None, None, None, None, 0), "gs_rounds_set")
        else:
            nat.check(L.gs_rounds_set(_p(b["rounds"]), _p(b["tile_live"]), _p(b["tile_state"]), _p(b["tile_rec"]), phase), "gs_rounds_set")

    def _tpg(self):
        """The per-Gaussian intersection counts the backward reads: the projection's, or (depth rounds) each Gaussian's in its round."""
        return _p(self.buf["tpg_round"] if self.rounds_on else self.buf["tiles_per_gauss"])

    def _probe_walk(self):
        """One guarded forward (projection .. blend) on the current capacities; returns (storage units, gradient rows, flags) of
        its walk -- the counters keep counting past the capacities.  Build time only (blocking)."""
        b = self.buf
        with torch.cuda.device(self.dev), self._on_stream():
            self._guarded(self._enqueue_forward)
        self.stream.synchronize()
        info = b["info"].tolist()
        w = b["walk_state"][:8].tolist()
        b["info"].zero_()
        walk_flags = nat.GS_FLAG_UNITS | nat.GS_FLAG_ROWS
        if int(info[nat.GS_INFO_FLAGS]) & ~walk_flags:
            raise RuntimeError(f"TrainStepGraph: the probed list capacities do not hold their own view {info}")
        return int(w[nat.GS_WALK_STORAGE]), int(w[nat.GS_WALK_ROWS]), int(info[nat.GS_INFO_FLAGS]) & walk_flags

    def _protect_pending(self, static: Tensor):
        """`static` (one of the runner's input buffers) is about to be overwritten: steps still pending that were issued
        with "same as the buffer holds" get a snapshot of it first (enqueued ahead of the overwrite on the same stream)."""
        snap = None
        for e in self.pending:
            for name in ("w2c", "K", "gt", "mask"):   # (the fields that can alias a static buffer)
                x = getattr(e, name)
                if isinstance(x, Tensor) and x.data_ptr() == static.data_ptr():
                    if snap is None:
                        snap = static.clone()
                    setattr(e, name, snap[0] if (x.dim() < static.dim()) else snap)

    def _image(self, t: Tensor, shape) -> Tensor:
        """The caller's image as the loss kernels read it: float32, contiguous, on the runner's device (a tensor that already is
        comes back as it is -- the usual case; anything else is converted once)."""
        if t.device != self.dev or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"TrainStepGraph: image of shape {tuple(t.shape)}, expected {tuple(shape)}")
            t = t.to(device=self.dev, dtype=torch.float32).contiguous()
        return t

    def _depth_image(self, t: Tensor, shape) -> Tensor:
        """The caller's depth target as the depth kernels read it: `_image`'s conversions, and a 16-byte aligned address (a view
        into the middle of a buffer is copied once)."""
        t = self._image(t, shape)
        return t if t.data_ptr() % 16 == 0 else t.clone()

    def _static_w2c(self) -> Tensor:
        """The step's static camera INPUT [1,4,4]: the view matrix the projection reads, or (poses) the raw matrix in the pose record."""
        return self.buf["w2c_raw"] if self.poses is not None else self.buf["viewmats"]

    def _stage_inputs(self, e: _Pending):
        """Everything that differs from the previous step, in ONE launch on the current stream (gs_step_inputs): Adam's bias
        corrections / learning rates, the camera into the static buffers, and the POINTERS to the target image and mask.
        Leaves in the record the (gt, mask) tensors whose pointers went in -- it keeps them alive until the step is applied --
        and the record in `self._staged`."""
        L, b, opt = nat.lib(), self.buf, self.opt
        t, lrs, w2c, K = e.t, e.lrs, e.w2c, e.K
        ok = lambda x, n: x.device == self.dev and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == n   # noqa: E731
        vm_src = k_src = None
        static_vm = self._static_w2c()
        if w2c.data_ptr() != static_vm.data_ptr():   # (the static buffer itself = "same as last step")
            self._protect_pending(static_vm)
            if ok(w2c, 16):
                vm_src = w2c
            else:
                static_vm[0].copy_(w2c, non_blocking=True)
        if K.data_ptr() != b["Ks"].data_ptr():
            self._protect_pending(b["Ks"])
            if ok(K, 9):
                k_src = K
            else:
                b["Ks"][0].copy_(K, non_blocking=True)
        gt = e.gt = self._image(e.gt, (self.H, self.W, 3))
        if self.has_mask and e.mask is None:
            raise ValueError("this runner was built with a mask; pass one every step")
        mask = e.mask = self._image(e.mask, (self.H, self.W)) if self.has_mask else None
        ns = len(opt._plist)
        b1, b2 = opt.defaults["betas"]
        nat.check(L.gs_step_inputs(self._st(), ns, (ct.c_float * ns)(*lrs), float(b1), float(b2), int(t), _p(b["hyper"]),
                                   None if self.poses is not None else _p(vm_src), _p(b["viewmats"]), _p(k_src), _p(b["Ks"]), _p(gt), _p(mask),
                                   _p(b["img_slots"])), "gs_step_inputs")
        if self.poses is not None:   # the view, its raw matrix into the record, the pose Adam's bias corrections at ITS step count
            view, pose_t = e.pose
            nat.check(L.gs_pose_step_inputs(self._st(), int(view), int(self.poses.deltas.shape[0]), _p(vm_src), None, self.pose_lr,
                                            self.pose_betas[0], self.pose_betas[1], int(pose_t), _p(b["pose_rec"])), "gs_pose_step_inputs")
        if self.exposure is not None:   # the view and the exposure Adam's bias corrections at ITS step count and the step's own rate
            view, exp_t, exp_lr = e.exposure
            nat.check(L.gs_exposure_step_inputs(self._st(), int(view), int(self.exposure.affine.shape[0]), float(exp_lr), self.exposure_betas[0],
                                                self.exposure_betas[1], int(exp_t), _p(b["exposure_rec"])), "gs_exposure_step_inputs")
        if self.bilagrid is not None:   # the view and the grids' Adam's bias corrections at ITS step count and the step's own rate
            view, bg_t, bg_lr = e.bilagrid
            nat.check(L.gs_bilagrid_step_inputs(self._st(), int(view), int(self.bilagrid.grids.shape[0]), float(bg_lr), self.bilagrid_betas[0],
                                                self.bilagrid_betas[1], int(bg_t), _p(b["bilagrid_rec"])), "gs_bilagrid_step_inputs")
        if self.depth is not None:   # the step's depth target (its address: read in place) and the weight as it stood at the call
            gd, lam = e.depth
            nat.check(L.gs_depth_step_inputs(self._st(), float(lam), self._depth_mode, _p(gd), _p(b["depth_rec"])), "gs_depth_step_inputs")
        if self.mcmc is not None:   # the step's noise: its strength at the means learning rate this step's Adam uses, its counter, the seed
            nat.check(L.gs_mcmc_step_inputs(self._st(), self.mcmc.noise_lr * float(lrs[self._means_seg]), int(t), self.mcmc.seed,
                                            _p(b["mcmc_rec"])), "gs_mcmc_step_inputs")
        self._staged = e

    def _st(self) -> int:
        return torch.cuda.current_stream(self.dev).cuda_stream

    class _OnStepStream:
        """`with runner._on_stream():` -- everything inside is enqueued on the runner's stream, ordered after the
        caller's current stream on entry and (`hand_back`) before it on exit."""

        def __init__(self, runner, wait_outer: bool = True, hand_back: bool = True):
            self.r = runner
            self.wait_outer = wait_outer
            self.hand_back = hand_back

        def __enter__(self):
            r = self.r
            self.outer = torch.cuda.current_stream(r.dev)
            if self.wait_outer:
                r.stream.wait_stream(self.outer)
            self.ctx = torch.cuda.stream(r.stream)
            self.ctx.__enter__()

        def __exit__(self, *exc):
            self.ctx.__exit__(*exc)
            if self.hand_back:
                self.outer.wait_stream(self.r.stream)
            return False

    def _on_stream(self, wait_outer: bool = True, hand_back: bool = True):
        return TrainStepGraph._OnStepStream(self, wait_outer, hand_back)

    def fence(self):
        """Orders the caller's current stream behind every step issued so far (what `handback="eager"` does on return from
        each `step()`): call it before reading parameters / statistics / outputs on the caller's stream in "lazy" mode."""
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)

    class _StepOutputs(Mapping):
        """The runner's static output tensors; in `handback="lazy"` mode the first access orders the caller's current
        stream behind the step that produced them.  A read-only Mapping, not a dict subclass: `dict(out)`, `{**out}`, `.get`,
        `.values()`, `.items()` all reach the tensors through `__getitem__` -- a dict subclass is read by the C-level fast
        paths behind the fence's back."""

        def __init__(self, runner, items, lazy: bool):
            self._items, self._runner, self._pending = dict(items), runner, lazy

        def _touch(self):
            if self._pending:
                self._pending = False
                self._runner.fence()

        def __getitem__(self, k):
            self._touch()
            return self._items[k]

        def __iter__(self):
            return iter(self._items)

        def __len__(self):
            return len(self._items)

    stop_after = int(os.environ.get('GS_TG_STOP_AFTER', '0'))
    project_rebuilds = os.environ.get('GS_TG_PROJECT_REBUILDS', '1') != '0'   # 0: every re-build probes and warms up
    debug_sync = False   # set True to synchronise after every stage (locates a faulting kernel; never under capture)

    class _Stop(Exception):
        pass

    def _ck(self, rc: int, what: str) -> None:
        nat.check(rc, what)
        self._stage_no = getattr(self, "_stage_no", 0) + 1
        if self.stop_after and self._stage_no >= self.stop_after:   # debugging aid: truncate the pipeline
            raise TrainStepGraph._Stop()
        if self.debug_sync and not torch.cuda.is_current_stream_capturing():
            self.stream.synchronize()

    def _project(self):
        L, b, m = nat.lib(), self.buf, self.model
        # (the runner hands out no list arrays: "gsplat" -- exact arrays, built when read -- renders from the short lists
        #  like "tight"; "gsplat_eager" walks gsplat's own lists)
        culling = {"gsplat": 1, "tight": 1, "gsplat_eager": 0}[getattr(m, "tile_culling", "tight")]
        if self.poses is not None:   # the corrected view matrix of the record's view, from the deltas as they stand
            self._ck(L.gs_pose_compose(self._st(), int(self.poses.deltas.shape[0]), _p(b["pose_rec"]), _p(self.poses.deltas.data),
                                       _p(b["viewmats"])), "gs_pose_compose")
        args = (self._st(), 1, self.N, self.K, int(m.active_sh_degree), _p(m.means), _p(m.quats), _p(m.log_scales),
                _p(m.logit_opacities), _p(m.sh_0), _p(m.sh_rest) if self.K > 1 else None, 0,
                _p(b["viewmats"]), _p(b["Ks"]), self.W, self.H, EPS2D, NEAR_PLANE, FAR_PLANE, RADIUS_CLIP, culling, 0, 1,
                _p(b["radii"]), _p(b["means2d"]), _p(b["depths"]), _p(b["conics"]), _p(b["colors_post"]),
                _p(b["rec"]), _p(b["bbox"]), _p(b["tiles_per_gauss"]), None, _p(b["sh_jac"]))
        if self.antialiased:
            self._ck(L.gs_project_fwd_aa(*args, _p(b["compensations"])), "gs_project_fwd_aa")
        elif self.camera_model == nat.GS_CAMERA_PINHOLE:
            self._ck(L.gs_project_fwd(*args), "gs_project_fwd")
        else:
            self._ck(L.gs_project_fwd_cm(*args, self.camera_model), "gs_project_fwd_cm")

    def _count(self, bbox: str = "bbox"):
        b = self.buf
        rendering.stage_count(nat.lib(), self._st(), self.lease, (1, self.N, self.tw, self.th), _p(b[bbox]), _p(b["depths"]), self.cap_coarse_list,
                              self._ck)

    def _probe(self):
        """Blocking reads of the list sizes for the current inputs (build time only): {I, longest tile list} from the
        per-tile count, then -- if the footprints call for the two-level binning -- {coarse entries, longest bin list}."""
        from .rendering import MAX_TILES_PER_TILE_PIPELINE, bin_shift_for, binning_choice
        b, dev, tiles = self.buf, self.dev, self.tiles
        n_isects, max_tile, footprint, per_tile = 0, 0, None, tiles <= MAX_TILES_PER_TILE_PIPELINE
        self.binning, self.bin_shift, self.cap_coarse, self.cap_coarse_list = "tiles" if per_tile else "bins", 2, 0, 0   # (else never counted per tile: the two-level scratch)
        cap, self.cap = self.cap, 0   # (the counts need nothing that the list capacity sizes: those slots are absent from `buf` here)
        self._lay(0)
        with torch.cuda.device(dev), self._on_stream():
            self._project()
            if per_tile:
                self._count()
        if per_tile:
            info = b["info"].tolist()
            n_isects, max_tile = int(info[nat.GS_INFO_ISECTS]), int(info[nat.GS_INFO_MAX_TILE])
            footprint = n_isects / max(1, self.N)
        self.binning = binning_choice(footprint, tiles)
        if self.binning == "bins":
            self.bin_shift = bin_shift_for(footprint) or 2
            self.cap_coarse, self.cap_coarse_list = 2 * self.N + 1024, 0
            while True:
                self._lay(1)
                with torch.cuda.device(dev), self._on_stream():
                    self._count()
                info = b["info"].tolist()
                self.cap_coarse = int(int(info[nat.GS_INFO_COARSE]) * self.margin) + 4096
                if not int(info[nat.GS_INFO_FLAGS]) & (nat.GS_FLAG_COARSE | nat.GS_FLAG_COARSE_LIST):
                    break
            self.cap_coarse_list = int(int(info[nat.GS_INFO_MAX_BIN]) * 1.5) + 64
            self.probed_coarse = (int(info[nat.GS_INFO_COARSE]), int(info[nat.GS_INFO_MAX_BIN]))   # coarse-bin entries I', longest bin list
            n_isects, max_tile = int(info[nat.GS_INFO_ISECTS]), int(info[nat.GS_INFO_MAX_TILE])
        b["info"].zero_()
        self.cap = cap
        return n_isects, max_tile

    def _enqueue_forward(self):
        """Projection, tile lists and the training blend on the current stream (the caller holds the step guard).  With depth
        rounds: the list stages and the blend twice, on the footprints of the front and of the back round; the rounds context is
        left at "behind both" for the backward (the caller clears it)."""
        L, b = nat.lib(), self.buf
        self._project()
        if self.depth is not None:   # the depth into lane 3 of the records' colour quad: the blend's fourth channel
            self._ck(L.gs_rec_depth(self._st(), 1, self.N, 3, _p(b["depths"]), _p(b["radii"]), _p(b["rec"])), "gs_rec_depth")
        if not self.rounds_on:
            self._lists_and_blend("bbox")
            return
        self._ck(L.gs_round_split(self._st(), self.N, _p(b["depths"]), _p(b["tiles_per_gauss"]), self.round_fraction, _p(b["depth_hist"]),
                                   _p(b["rounds"])), "gs_round_split")
        for phase in ((4,) if self.front_only else (1, 2)):
            self._rounds_phase(phase)
            self._ck(L.gs_round_footprints(self._st(), self.N, self.tw, self.th, _p(b["bbox"]), _p(b["depths"]), _p(b["bbox_round"]),
                                            _p(b["tpg_round"])), "gs_round_footprints")
            self._lists_and_blend("bbox_round")
        self._rounds_phase(3)

    def _lists_and_blend(self, bbox: str):
        L, b, st, lease = nat.lib(), self.buf, self._st(), self.lease
        self._count(bbox)
        rendering.stage_lists(L, st, lease, (1, self.N, self.tw, self.th), _p(b[bbox]), _p(b["depths"]), self.cap, self.cap_tile, self._ck)
        # (the blend, forward and backward, walks at the LAYOUT's capacities: `_alloc_walk` laid it for the runner's as they stand)
        assert (lease.layout.cap_units, lease.layout.cap_rows) == (self.cap_units, self.cap_rows)
        if self.depth is not None:
            rendering.stage_blend_fwd(L, st, lease, 1, self.W, self.H, 4, _p(b["bg4"]), self.cap, _p(b["render_colors4"]), _p(b["render_alphas"]), self._ck)
            return
        rendering.stage_blend_fwd(L, st, lease, 1, self.W, self.H, 3, _p(b["bg"]), self.cap, _p(b["render_colors"]), _p(b["render_alphas"]), self._ck)

    def _guarded(self, enqueue):
        """`enqueue()` on the current stream under the step guard, its stages counted from one (GS_TG_STOP_AFTER cuts it short); the
        guard and the rounds context are cleared whatever happens."""
        L = nat.lib()
        nat.check(L.gs_guard_set(_p(self.buf["info"]), self.cap, self.cap_tile), "gs_guard_set")
        self._stage_no = 0
        try:
            enqueue()
        except TrainStepGraph._Stop:
            pass
        finally:
            L.gs_guard_set(None, 0, 0)
            L.gs_rounds_set(None, None, None, None, 0)

    def _enqueue_step(self):
        """The captured step on the current stream, guarded: forward, loss and blend backward, then `_enqueue_rest` -- what the step
        does with the gradient rows; nothing here allocates or synchronises."""
        L, b, st, W, H = nat.lib(), self.buf, self._st(), self.W, self.H

        def enqueue():
            self._enqueue_forward()
            lam = float(self.lc.lambda_ssim)
            slots = _p(b["img_slots"]) if self.has_mask else None
            if self.depth is not None:
                # ONE pass over the 4-channel blend: the image the kernels below read (render_colors), the expected-depth map and the
                # depth term's partials; target, mode and weight come from the record (gs_depth_step_inputs), the mask from its slot
                self._ck(L.gs_depth_loss_split(st, H, W, _p(b["depth_rec"]), 0.0, 0, None, None, slots, _p(b["render_colors4"]),
                                               _p(b["render_alphas"]), _p(b["render_colors"]), _p(b["render_depth"]), _p(b["depth_partials"])),
                         "gs_depth_loss_split")
            img = b["render_colors"]
            if self.exposure is not None:   # the loss reads the view's affine of the render; the blend backward keeps the raw render
                n_exp, tab, img = int(self.exposure.affine.shape[0]), _p(self.exposure.affine.data), b["exposed"]
                self._ck(L.gs_exposure_apply(st, H, W, n_exp, _p(b["exposure_rec"]), 0, tab, _p(b["render_colors"]), _p(img)), "gs_exposure_apply")
            if self.bilagrid is not None:   # the loss reads the slice of the view's grid applied to the render
                img = b["exposed"]
                n_bg, gx, gy, gl = self._bilagrid_shape()
                self._ck(L.gs_bilagrid_apply(st, H, W, n_bg, gx, gy, gl, _p(b["bilagrid_rec"]), 0, _p(self.bilagrid.grids.data),
                                             _p(b["render_colors"]), _p(img)), "gs_bilagrid_apply")
            self._ck(L.gs_l1_ssim_fwd_slots(st, H, W, lam, _p(img), _p(b["img_slots"]), int(self.has_mask), 1, _p(b["loss_ws"]),
                                             _p(b["loss3"])), "gs_l1_ssim_fwd_slots")
            if self.depth is not None:   # value and 1 / sum(w) into the record; lambda_depth * value behind the image loss in the total
                self._ck(L.gs_depth_loss_finish(st, H, W, _p(b["depth_rec"]), 0.0, 1, _p(b["depth_partials"]), _p(b["loss3"])),
                         "gs_depth_loss_finish")
            self._ck(L.gs_l1_ssim_bwd_slots(st, H, W, lam, _p(img), _p(b["img_slots"]), 1, _p(b["loss_ws"]),
                                             _p(b["one"]), _p(b["v_render"])), "gs_l1_ssim_bwd_slots")
            if self.exposure is not None:   # v_render: dL/d exposed -> dL/d render in place; the 12 sums of the view's row
                self._ck(L.gs_exposure_bwd(st, H, W, n_exp, _p(b["exposure_rec"]), 0, tab, _p(b["render_colors"]), _p(b["v_render"]),
                                           _p(b["exposure_partials"]), _p(b["v_affine"])), "gs_exposure_bwd")
            if self.bilagrid is not None:   # v_render: dL/d exposed -> dL/d render in place; the slice's adjoint into the view's slab
                self._ck(L.gs_bilagrid_bwd(st, H, W, n_bg, gx, gy, gl, _p(b["bilagrid_rec"]), 0, _p(self.bilagrid.grids.data),
                                           _p(b["render_colors"]), _p(b["v_render"]), _p(b["bilagrid_partials"]), _p(b["v_slab"])),
                         "gs_bilagrid_bwd")
            if self.scale_reg and self.fuse_adam:   # the value, from the parameters before the in-place update; the gradient: `_enqueue_rest`
                self._scale_reg(None)
            if self.mcmc is not None and self.fuse_adam:   # likewise the budget regulariser's, behind it in the total
                self._mcmc_reg(None, None)
            if self.bilagrid is not None and self.fuse_adam:   # the total variation behind both: the total sums scale, budget, TV
                self._bilagrid_tv()
            if self.depth is not None:
                # ONE pass: v_render and the depth term's gradient (through the expected depth's quotient) into the 4-channel blend
                # backward's v_colors and v_alphas
                self._ck(L.gs_depth_loss_join(st, H, W, _p(b["depth_rec"]), 0.0, 0, None, None, slots, _p(b["render_colors4"]),
                                              _p(b["render_alphas"]), _p(b["render_depth"]), _p(b["v_render"]), _p(b["v_colors4"]),
                                              _p(b["v_alphas"])), "gs_depth_loss_join")
                rendering.stage_blend_bwd(L, st, self.lease, 1, W, H, 4, _p(b["render_colors4"]), _p(b["render_alphas"]), _p(b["v_colors4"]),
                                          _p(b["v_alphas"]), _p(b["unit_cls"]), self._ck)
            else:
                rendering.stage_blend_bwd(L, st, self.lease, 1, W, H, 3, _p(b["render_colors"]), _p(b["render_alphas"]), _p(b["v_render"]), None,
                                          _p(b["unit_cls"]), self._ck)
            self._enqueue_rest(st)
        self._guarded(enqueue)

    def _enqueue_rest(self, st: int):
        """Projection / SH backward, statistics and Adam from the gradient rows, and the step's status words."""
        L, b, m, opt = nat.lib(), self.buf, self.model, self.opt
        N, W, H = self.N, self.W, self.H
        b1, b2 = opt.defaults["betas"]
        poses = self.poses is not None
        if self.fuse_adam:
            if poses:
                # The gradient rows are walked ONCE, by gs_row_sums; the camera gradient is formed from the per-Gaussian sums BEFORE the
                # fused kernel moves the parameters (gs_project_bwd_cam's kernels on the sums), and the fused kernel consumes the same
                # sums (gs_project_bwd_adam_sums: the same update bit for bit).  DESIGN.md "Poses in the captured step".
                self._ck(L.gs_row_sums(st, 1, N, _p(b["radii"]), _p(b["colors_post"]), self._tpg(), _p(b["cum_tiles"]), _p(b["rows"]),
                                        _p(b["row_base"]), _p(b["qmask"]), _p(b["pose_row_sums"]), _p(b["pose_v_pre"]), None, float(max(H, W)),
                                        None, None), "gs_row_sums")
                self._ck(L.gs_cam_grad_sums(st, N, self.K, int(m.active_sh_degree), _p(m.means), _p(m.quats), _p(m.log_scales),
                                             _p(m.sh_rest) if self.K > 1 else None, _p(b["viewmats"]), _p(b["Ks"]), W, H, EPS2D, NEAR_PLANE,
                                             FAR_PLANE, _p(b["radii"]), _p(b["colors_post"]), 1, _p(b["sh_jac"]), _p(b["pose_row_sums"]),
                                             _p(b["cam_partials"]), _p(b["v_viewmats"]), _p(b["v_campos"])), "gs_cam_grad_sums")
            offs = (ct.c_int64 * 6)(*opt._offs)
            # what every row-walking entry takes, once -- a plain tuple literal: tests/test_native_header.py counts the calls below against
            # the header with it; [19:22]: the gradient rows, in whose place gs_project_bwd_adam_sums takes the sums
            row_args = (st, N, self.K, int(m.active_sh_degree), _p(opt.flat_param), _p(opt.exp_avg), _p(opt.exp_avg_sq), offs,
                        _p(b["viewmats"]), _p(b["Ks"]), W, H, EPS2D, NEAR_PLANE, FAR_PLANE, _p(b["radii"]), _p(b["colors_post"]),
                        self._tpg(), _p(b["cum_tiles"]), _p(b["rows"]), _p(b["row_base"]), _p(b["qmask"]), _p(b["v_abs"]), float(b1),
                        float(b2), float(opt.defaults["eps"]), _p(b["hyper"]), _p(b["applied"]), _p(m.max_radii),
                        _p(m.grad_norm_accum), _p(m.collecting_counts), _p(b["sh_jac"]))
            reg_on, ratio, lam = (1, self.max_scale_ratio, self.lambda_scale) if self.scale_reg else (0, 0.0, 0.0)
            mcmc_on, (bud_a, bud_b) = int(self.mcmc is not None), self.mcmc_reg if self.mcmc is not None else (0.0, 0.0)
            if self.visible_adam:   # (no depth, poses, mcmc, other camera model or mode here: refused at construction)
                self._ck(L.gs_project_bwd_selective(*row_args, reg_on, ratio, lam), "gs_project_bwd_selective")
            elif self.depth is not None:
                # v_z per Gaussian from lane 3 of its gradient rows (gs_depth_grads' gather), then the fused kernel adds v_z times row 2
                # of the view matrix to the means gradient where gs_depth_grads would: the same update bit for bit
                self._ck(L.gs_depth_grads_z(st, 1, N, 3, _p(b["radii"]), self._tpg(), _p(b["cum_tiles"]), _p(b["rows"]), _p(b["row_base"]),
                                             _p(b["qmask"]), _p(b["v_depths"])), "gs_depth_grads_z")
                self._ck(L.gs_project_bwd_adam_depth(*row_args, reg_on, ratio, lam, mcmc_on, bud_a, bud_b, _p(b["v_depths"])), "gs_project_bwd_adam_depth")
            elif poses:   # (the sums in place of rows, row_base, qmask; one entry for the three variants)
                self._ck(L.gs_project_bwd_adam_sums(*row_args[:19], _p(b["pose_row_sums"]), *row_args[22:], reg_on, ratio, lam, mcmc_on, bud_a, bud_b),
                         "gs_project_bwd_adam_sums")
            elif self.mcmc is not None:
                self._ck(L.gs_project_bwd_adam_mcmc(*row_args, reg_on, ratio, lam, bud_a, bud_b), "gs_project_bwd_adam_mcmc")
            elif self.camera_model != nat.GS_CAMERA_PINHOLE and self.scale_reg:   # (no depth, poses or mcmc here: refused at construction)
                self._ck(L.gs_project_bwd_adam_reg_cm(*row_args, ratio, lam, self.camera_model), "gs_project_bwd_adam_reg_cm")
            elif self.camera_model != nat.GS_CAMERA_PINHOLE:
                self._ck(L.gs_project_bwd_adam_cm(*row_args, self.camera_model), "gs_project_bwd_adam_cm")
            elif self.antialiased and self.scale_reg:   # (no depth, poses, mcmc or other camera model here: refused at construction)
                self._ck(L.gs_project_bwd_adam_reg_aa(*row_args, ratio, lam), "gs_project_bwd_adam_reg_aa")
            elif self.antialiased:
                self._ck(L.gs_project_bwd_adam_aa(*row_args), "gs_project_bwd_adam_aa")
            elif self.scale_reg:
                self._ck(L.gs_project_bwd_adam_reg(*row_args, ratio, lam), "gs_project_bwd_adam_reg")
            else:
                self._ck(L.gs_project_bwd_adam(*row_args), "gs_project_bwd_adam")
        else:
            g = self.grads
            bwd_args = (st, 1, N, self.K, int(m.active_sh_degree), _p(m.means), _p(m.quats), _p(m.log_scales),
                        _p(m.sh_0), _p(m.sh_rest) if self.K > 1 else None, 0, _p(b["viewmats"]), _p(b["Ks"]), W, H,
                        EPS2D, NEAR_PLANE, FAR_PLANE, _p(b["radii"]), _p(b["colors_post"]), self._tpg(),
                        _p(b["cum_tiles"]), _p(b["rows"]), _p(b["row_base"]), _p(b["qmask"]), _p(g["means"]), _p(g["quats"]),
                        _p(g["log_scales"]), _p(g["logit_opacities"]), _p(g["sh_0"]), _p(g["sh_rest"]), _p(b["v_abs"]))
            if poses:   # the same gradients, and the camera's from the three tensors it hands out
                self._ck(L.gs_project_bwd_cam(*bwd_args, _p(b["v_means2d"]), _p(b["v_conics"]), _p(b["v_colors_post"]), None,
                                               _p(m.logit_opacities), 1, _p(b["sh_jac"]), None, None, None, _p(b["cam_partials"]),
                                               _p(b["v_viewmats"]), _p(b["v_campos"])), "gs_project_bwd_cam")
            elif self.antialiased:
                self._ck(L.gs_project_bwd_aa(*bwd_args, None, None, None, None, _p(m.logit_opacities), 1, _p(b["sh_jac"]), None, None, None),
                         "gs_project_bwd_aa")
            elif self.camera_model != nat.GS_CAMERA_PINHOLE:
                self._ck(L.gs_project_bwd_cm(*bwd_args, None, None, None, None, _p(m.logit_opacities), 1, _p(b["sh_jac"]), None, None, None,
                                              self.camera_model), "gs_project_bwd_cm")
            else:
                self._ck(L.gs_project_bwd(*bwd_args, None, None, None, None, _p(m.logit_opacities), 1, _p(b["sh_jac"]), None, None, None),
                         "gs_project_bwd")
            if self.depth is not None:   # the depth lane's gradient onto the means', in front of the regularisers
                self._ck(L.gs_depth_grads(st, 1, N, 3, _p(m.means), _p(b["viewmats"]), _p(b["radii"]), self._tpg(), _p(b["cum_tiles"]),
                                           _p(b["rows"]), _p(b["row_base"]), _p(b["qmask"]), _p(g["means"]), None, None, None), "gs_depth_grads")
            if self.scale_reg:   # value into the loss total, gradient onto the render's
                self._scale_reg(g["log_scales"])
            if self.mcmc is not None:
                self._mcmc_reg(g["logit_opacities"], g["log_scales"])
            if self.bilagrid is not None:
                self._bilagrid_tv()
            self._ck(L.gs_update_statistics(st, N, float(max(H, W)), _p(b["radii"]), _p(b["v_abs"]), _p(m.max_radii),
                                            _p(m.grad_norm_accum), _p(m.collecting_counts)), "gs_update_statistics")
            ns = len(opt._plist)
            ends = (ct.c_int64 * ns)(*opt._ends)
            lens = (ct.c_int64 * ns)(*opt._lens)
            gptr = (ct.c_void_p * ns)(*[_p(g[grp["name"]]) for grp, _ in opt._plist])
            if self.visible_adam:   # the same launch over the Gaussians with radii > 0
                widths = (ct.c_int64 * ns)(*[p.numel() // N for _, p in opt._plist])
                self._ck(L.gs_adam_step_visible_dev(st, opt.flat_param.numel(), _p(opt.flat_param), _p(opt.exp_avg), _p(opt.exp_avg_sq), ns,
                                                    ends, lens, gptr, float(b1), float(b2), float(opt.defaults["eps"]), 1.0, _p(b["hyper"]),
                                                    _p(b["applied"]), N, widths, _p(b["radii"])), "gs_adam_step_visible_dev")
            else:
                self._ck(L.gs_adam_step_dev(st, opt.flat_param.numel(), _p(opt.flat_param), _p(opt.exp_avg), _p(opt.exp_avg_sq), ns,
                                            ends, lens, gptr, float(b1), float(b2), float(opt.defaults["eps"]), 1.0, _p(b["hyper"]),
                                            _p(b["applied"])), "gs_adam_step_dev")
        if self.mcmc is not None:   # the noise, on the updated parameters; a skipped step adds none
            self._ck(L.gs_mcmc_noise_step(st, N, _p(b["mcmc_rec"]), _p(m.log_scales), _p(m.quats), _p(m.logit_opacities), _p(m.means)),
                     "gs_mcmc_noise_step")
        if poses:   # the chain to the view's 6-vector and Adam over all corrections; a skipped step moves none
            ps = self.pose_state
            self._ck(L.gs_pose_adam(st, int(self.poses.deltas.shape[0]), _p(b["pose_rec"]), _p(self.poses.deltas.data), _p(ps.exp_avg),
                                    _p(ps.exp_avg_sq), _p(b["v_viewmats"]), _p(b["v_campos"]), _p(b["v_delta"]), self.pose_betas[0],
                                    self.pose_betas[1], self.pose_eps), "gs_pose_adam")
        if self.exposure is not None:   # Adam over the whole table, the step's sums on the view's row; a skipped step moves none
            es = self.exposure_state
            self._ck(L.gs_exposure_adam(st, int(self.exposure.affine.shape[0]), _p(b["exposure_rec"]), _p(self.exposure.affine.data),
                                        _p(es.exp_avg), _p(es.exp_avg_sq), _p(b["v_affine"]), self.exposure_betas[0], self.exposure_betas[1],
                                        self.exposure_eps), "gs_exposure_adam")
        if self.bilagrid is not None:   # Adam over every grid with the step's dense gradient; a skipped step moves none
            gs_ = self.bilagrid_state
            self._ck(L.gs_bilagrid_adam(st, int(self.bilagrid.grids.numel()), _p(b["bilagrid_rec"]), _p(self.bilagrid.grids.data),
                                        _p(gs_.exp_avg), _p(gs_.exp_avg_sq), _p(b["v_grids"]), self.bilagrid_betas[0], self.bilagrid_betas[1],
                                        self.bilagrid_eps), "gs_bilagrid_adam")
        self._ck(L.gs_step_status(st, _p(b["info"]), _p(b["applied"]), self.status.data_ptr(), _p(b["loss3"]), _p(b["loss_ring"]),
                                  self.LOSS_RING, _p(b["walk_state"])), "gs_step_status")

    def _scale_reg(self, v_log_scales: Optional[Any], check=None):
        """The scale-ratio regulariser on the current stream: lambda * reg into loss3[2], reg into buf["scale_reg"][0], and (a gradient
        tensor or a device address given) its gradient added to that log-scale gradient."""
        b, m = self.buf, self.model
        v = v_log_scales if (v_log_scales is None or isinstance(v_log_scales, int)) else v_log_scales.data_ptr()
        (check or self._ck)(nat.lib().gs_scale_reg(self._st(), self.N, _p(m.log_scales), self.max_scale_ratio, self.lambda_scale, _p(b["loss3"]),
                                        _p(b["scale_reg"]), v), "gs_scale_reg")

    def _bilagrid_shape(self):
        """(n_views, grid_x, grid_y, grid_l) as the gs_bilagrid_* entries take them."""
        n, _, gl, gy, gx = (int(x) for x in self.bilagrid.grids.shape)
        return n, gx, gy, gl

    def _bilagrid_tv(self):
        """The grids' total variation on the current stream: bilagrid_tv * tv into loss3[2], tv into buf["bilagrid_tv"], and the
        step's dense gradient buf["v_grids"] = bilagrid_tv * d tv / d grids + the view's slab -- from the grids before the update."""
        b = self.buf
        n_bg, gx, gy, gl = self._bilagrid_shape()
        self._ck(nat.lib().gs_bilagrid_tv(self._st(), n_bg, gx, gy, gl, _p(self.bilagrid.grids.data), self.bilagrid_tv,
                                          _p(b["bilagrid_rec"]), 0, _p(b["v_slab"]), _p(b["loss3"]), _p(b["bilagrid_tv"]), _p(b["v_grids"]),
                                          _p(b["bilagrid_tv_ws"])), "gs_bilagrid_tv")

    def _mcmc_reg(self, v_logit: Optional[Tensor], v_log_scales: Optional[Tensor]):
        """The budget regulariser on the current stream: reg into loss3[2] and buf["mcmc_reg"][0], and (gradient tensors given) its
        gradients added to them."""
        b, m = self.buf, self.model
        self._ck(nat.lib().gs_mcmc_reg(self._st(), self.N, _p(m.logit_opacities), _p(m.log_scales), self.mcmc_reg[0], self.mcmc_reg[1],
                                       _p(b["loss3"]), _p(b["mcmc_reg"]), _p(v_logit), _p(v_log_scales)), "gs_mcmc_reg")

    def _tail(self, t: int, lrs):
        """What a step enqueues behind its graph (nothing: the single-GPU step is the graph)."""

    def _hyper(self, t: int, lrs):
        L, opt = nat.lib(), self.opt
        ns = len(opt._plist)
        b1, b2 = opt.defaults["betas"]
        nat.check(L.gs_adam_hyper(self._st(), ns, (ct.c_float * ns)(*lrs), float(b1), float(b2), int(t), _p(self.buf["hyper"])),
                  "gs_adam_hyper")

    def _capture(self, warm_up: bool = True):
        """Warm-up outside capture is NOT possible without applying a step, so the first launch of every kernel
        happens on a throw-away copy of the optimizer state: parameters, moments and statistics are saved, one eager
        guarded step runs (raising kernel attributes, validating capacities), and the state is restored.
        `warm_up=False` (a re-build on projected capacities: every kernel has run before in this process): capture only."""
        opt, m = self.opt, self.model
        names = ("max_radii", "grad_norm_accum", "collecting_counts")
        with torch.cuda.device(self.dev), self._on_stream():
            if warm_up:
                self._warm.add((self.binning, self.cap_tile))
                saved = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [getattr(m, n).clone() for n in names]
                # (the per-view tables and their moments are throw-away state of the warm-up step like the model's)
                pose_live = [x for _, _, table, state in self._tables for x in (table.data, state.exp_avg, state.exp_avg_sq)]
                pose_saved = [x.clone() for x in pose_live]
                self._hyper(max(opt._step, 0) + 1, self._lrs())
                self._enqueue_step()
                self.stream.synchronize()
                info = self.buf["info"].tolist()
                with torch.no_grad():
                    opt.flat_param.copy_(saved[0]); opt.exp_avg.copy_(saved[1]); opt.exp_avg_sq.copy_(saved[2])
                    for n, s in zip(names, saved[3:]):
                        getattr(m, n).copy_(s)
                    for x, s in zip(pose_live, pose_saved):
                        x.copy_(s)
                self.buf["applied"].zero_()
                if info[nat.GS_INFO_FLAGS] != 0:   # the capacities learnt from the probe do not hold (cannot happen unless inputs changed in between)
                    self.buf["info"].zero_()
                    raise RuntimeError(f"TrainStepGraph: warm-up step overflowed its own capacities {info}")
            self.graph = None
            if self.use_graph:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.stream):
                    self._enqueue_step()
                self.graph = g
                self.stats["captures"] += 1
            if warm_up:
                self.stream.synchronize()
        self.status.zero_()   # (nothing is in flight: the warm-up step's status words are stale)
        self.confirmed_at_build = self.confirmed

    # ------------------------------------------------------------------------------------------ stepping
    def _issue(self, entry: _Pending):
        # The step waits for the caller's stream on entry: that orders it behind pending WRITERS of the inputs handed in and
        # behind pending READERS of what the replay overwrites -- the static outputs the previous `step()` returned, the
        # parameters and moments (fused Adam), the statistics.  (Round 3 skipped the wait for steps that take no input from
        # the caller; a loss accumulation, a PSNR kernel or an eval render queued on the caller's stream after step i could
        # then run concurrently with replay i+1: ADVICE r3.)  Only `inputs_ready=True` -- the caller's promise that its
        # stream holds neither -- skips it.  The wait is free when the caller's stream is idle, i.e. with handback="lazy" in a
        # loop that reads nothing between steps; behind an eager hand-back it costs two cross-queue signal hops.
        with torch.cuda.device(self.dev), self._on_stream(wait_outer=not entry.inputs_ready, hand_back=self.handback == "eager"):
            if entry.conv is not None:
                # the runner's OWN conversion / copy of a target was enqueued on the caller's stream (`step`): the promise
                # `inputs_ready=True` covers the caller's writers, not this one
                self.stream.wait_event(entry.conv)
                entry.conv = None
            after = entry.ready_event
            if after is not None:   # (`step(ready_event=...)`: the upload of this step's inputs on the caller's copy stream(s))
                for ev in (after if isinstance(after, (list, tuple)) else (after,)):
                    self.stream.wait_event(ev)
                entry.ready_event = None
            self._stage_inputs(entry)   # (the tensors the step reads: kept by the entry)
            if self.graph is not None:
                self.graph.replay()
            else:
                self._enqueue_step()
            self._tail(entry.t, entry.lrs)   # (ViewParallelGraphStep: the collectives and what applies the step; nothing here)
        self.pending.append(entry)
        self.issued += 1

    def step(self, data: Optional[Dict[str, Any]] = None, gt_img: Optional[Tensor] = None, mask: Optional[Tensor] = None,
             inputs_ready: bool = False, ready_event: Optional["torch.cuda.Event"] = None, host_src=None,
             view_index: Optional[int] = None, gt_depth: Optional[Tensor] = None):
        """One training iteration.  `data` / `gt_img` / `mask` default to the previous step's (the camera's static buffers are
        re-used as they are; the target image and the mask are the previous step's own tensors, read in place).  Returns the
        runner's static output tensors (valid until the next `step()` is CALLED: reads
        enqueued on the caller's stream before that call are ordered in front of the replay that overwrites them).
        `inputs_ready=True` is the caller's promise that no work still pending on its stream (a) writes the tensors handed
        in, (b) reads the outputs of an earlier step, the model's parameters or its statistics: the step then does not wait
        for the caller's stream (see `_issue`).  Without the promise every step does.
        LIFETIME of the inputs: the target image and the mask are read IN PLACE, by the loss kernels of the replay and -- after a
        capacity overflow -- again by the replay of the skipped step, up to `check_every` steps later: a tensor handed in must
        not be written (nor its storage recycled by the loader) until the step is retired, i.e. until `finish()` or
        `check_every` further steps.  A loader that refills one staging buffer builds the runner with `copy_targets=True`.
        `ready_event`: an event the step's stream waits for before it reads anything (the upload of the inputs on a copy stream:
        `HostFeed`).  `host_src = {"w2c", "K", "image"[, "mask"]}` host tensors the device inputs were uploaded from: a feeder that
        recycles its device slots hands them in, and an overflow recovery replays the step from a FRESH upload of those instead
        of from slots that have been refilled since.  A `data["w2c"]` that requires grad raises `ValueError` (see `__init__`).
        `view_index`: with `poses`, required -- the row of `poses.deltas` that corrects this step's `data["w2c"]` (data=None: the
        previous step's raw matrix); with `exposure`, required -- the row of `exposure.affine` of this step's target image.
        `gt_depth`: with `depth`, this step's depth target [H, W] (default: the previous step's; `gt_img`'s lifetime rules)."""
        _refuse_camera_grads(data)
        depth_on = self.depth is not None
        if gt_depth is not None and not depth_on:
            raise ValueError("TrainStepGraph.step: gt_depth given, but the runner was built without `depth`")
        view = _pose_view(self.poses, view_index, self.exposure, self.bilagrid)
        W, H = (self.W, self.H) if data is None else (int(data["width"]), int(data["height"]))
        if self._state_key(W, H) != self._key:
            self.finish()
            prev, dep = self._staged, self._staged.depth
            size_changed = (W, H) != (self.W, self.H)
            if size_changed:
                # another frame size: the static image buffers are re-allocated, so the frame must bring its own target
                if gt_img is None or (self.has_mask and mask is None) or (depth_on and gt_depth is None):
                    raise ValueError("TrainStepGraph.step: a change of image size needs gt_img (and mask, and gt_depth) of the new size")
                cur = (data["w2c"], data["K"], gt_img, mask)
                if depth_on:   # (validated against the new size before anything is re-built)
                    dep = (self._depth_image(gt_depth, (H, W)), float(self.lambda_depth))
                self.W, self.H = W, H
            else:
                cur = (prev.w2c, prev.K, prev.gt, prev.mask) if data is None else (data["w2c"], data["K"], gt_img if gt_img is not None else prev.gt,
                                                                                   mask if mask is not None else prev.mask)
                # (old static buffers named here stay alive through `cur` until the new ones have been filled from them)
            # the largest list the status words showed since the last build, scaled to the new model size: a refinement
            # re-captures on whichever view comes next, and a capacity learnt from that one view alone overflows on the first
            # wider one (tools/train_soak.py: 153 of 700 steps were replayed before this).  Not the old CAPACITY scaled: that
            # compounds margin on margin, and every kernel whose grid is sized by the capacity pays for the empty workgroups
            n_new = self.model.means.shape[0]
            growth = max(1.0, n_new / max(self.N, 1))
            self.cap_floor = 0 if size_changed else min(int(self.seen_isects * growth * self.margin), (1 << 31) - (1 << 20))
            self.walk_floor = (0, 0) if size_changed else (int(self.seen_units * growth), int(self.seen_rows * growth))
            # ... and when that history exists (same frame size, per-tile binning, a model that grew by less than 2 x) the
            # re-build needs no probe at all: the host never reads the device between the refinement and the next replay
            # (bench.py `real_loop`: a probing re-build cost 5.5 ms + a throw-away warm-up step per refinement, more than the
            # 100 captured steps in between had saved against the eager loop)
            # (an opacity reset changes how deep the blend walks -- nothing saturates any more -- though not the lists: the walk
            #  capacities then come from a fresh probe, the list capacities keep their floor)
            reset = getattr(self.model, "opacity_resets", 0) != self._opacity_resets
            if reset:
                self.walk_floor = (0, 0)
                self._walk_history_void = True
            projected = carried = None
            if (not size_changed and not reset and self.binning == "tiles" and self.seen_isects > 0 and growth <= 2.0 and self.project_rebuilds
                    and self._key is not None and self._state_key(W, H)[5:] == self._key[5:]):
                projected = (min(int(self.seen_isects * growth), 1 << 30), max(int(self.seen_tile * min(growth, 1.25)), 64),
                             int(self.seen_units * growth), int(self.seen_rows * growth))
                # ... but only into a tile-sort class this runner has already run EAGERLY: a class used for the first time is
                # another kernel / another LDS size, whose attributes `ensure_lds` would raise -- and which would launch for the
                # first time -- inside the stream capture (gs_binning.hip: the warm-up exists to avoid exactly that)
                cls = _sort_class(int(projected[1] * self.margin))
                if (self.binning, cls) not in self._warm:
                    # (the probing re-build still takes the projection as a floor: its probe sees ONE view, the history all)
                    carried, projected = projected, None
            self.seen_isects = self.seen_tile = self.seen_units = self.seen_rows = 0
            self.cap = self.cap_units = self.cap_rows = 0
            # (the tables' views, step counts and rates: the previous step's, as a re-build has always staged them)
            staged = self._next_step(*cur, pose=prev.pose, exposure=prev.exposure, bilagrid=prev.bilagrid, depth=dep)
            if projected is None and carried is not None:
                self._build(staged, min_cap=carried[0], min_cap_tile=carried[1], min_walk=carried[2:4])
            else:
                self._build(staged, projected=projected)
        b = self.buf
        w2c = self._static_w2c()[0] if data is None else data["w2c"]
        K = b["Ks"][0] if data is None else data["K"]
        gt = self._staged.gt if gt_img is None else gt_img   # (the previous step's own tensors, by reference)
        mk = (self._staged.mask if mask is None else mask) if self.has_mask else None
        gt_in, mk_in = gt, mk
        gt = self._image(gt, (self.H, self.W, 3))   # (validated / converted BEFORE the step is counted)
        if self.has_mask:
            if mk is None:
                raise ValueError("this runner was built with a mask; pass one every step")
            mk = self._image(mk, (self.H, self.W))
        if self.copy_targets and gt_img is not None:   # (a step that re-uses the previous step's tensors re-uses its private copies)
            gt = gt.clone() if gt is gt_in else gt
            mk = (mk.clone() if mk is mk_in else mk) if mk is not None else None
        gd = gd_in = None
        if depth_on:
            gd_in = self._staged.depth[0] if gt_depth is None else gt_depth   # (the previous step's own tensor, by reference)
            gd = self._depth_image(gd_in, (self.H, self.W))
            if self.copy_targets and gt_depth is not None and gd is gd_in:
                gd = gd.clone()
        conv = None
        if gt is not gt_in or mk is not mk_in or gd is not gd_in:
            # a conversion (dtype / device / layout) or a private copy ran on the CALLER's stream just now: the runner's stream
            # waits for exactly that, whatever `inputs_ready` promises about the caller's own work
            conv = torch.cuda.Event()
            conv.record(torch.cuda.current_stream(self.dev))
        opt = self.opt
        opt._step += 1
        # The queued entry is what an overflow recovery replays.  Inputs are kept by reference: a caller must not write
        # into a camera / target / mask tensor it has handed in before `finish()` (or `check_every` further steps) -- the
        # target and the mask are not even copied: the step reads them where they lie (`_stage_inputs`).  Entries that alias the
        # runner's OWN static camera buffers (data=None steps) are snapshotted right before a later step overwrites those
        # buffers (`_protect_pending`), so a skipped step is always replayed with its own inputs.
        entry = _Pending(opt._step, self._lrs(), w2c, K, gt, mk, bool(inputs_ready), conv, ready_event, host_src)
        # the view and each table's step count travel with the step, like t and the learning rates: a replay re-stages them -- and so do
        # the rates of the exposure and the grids, and the depth target with its weight, as they stand at this call
        if self.poses is not None:
            self.pose_state.step += 1
            entry.pose = (view, self.pose_state.step)
        if self.exposure is not None:
            self.exposure_state.step += 1
            entry.exposure = (view, self.exposure_state.step, float(self.exposure_lr))
        if self.bilagrid is not None:
            self.bilagrid_state.step += 1
            entry.bilagrid = (view, self.bilagrid_state.step, float(self.bilagrid_lr))
        if depth_on:
            entry.depth = (gd, float(self.lambda_depth))
        self._issue(entry)
        if self.issued % self.check_every == 0:
            self._poll(block=False)
        outs = {"render_img": b["render_colors"][0], "loss3": b["loss3"], "batch_radii": b["radii"], "absgrad": b["v_abs"]}
        if self.scale_reg:
            outs["scale_reg"] = b["scale_reg"][0]   # (0-d, the eager loss dict's "scale_reg")
        if self.mcmc is not None:
            outs["mcmc_reg"] = b["mcmc_reg"][0]   # (0-d, `strategy.regularization(*mcmc_reg)`)
        if self.poses is not None:
            outs["viewmat"] = b["viewmats"][0]    # the corrected matrix the step rendered with
            outs["v_delta"] = b["v_delta"]        # dL / d poses.deltas[view_index] of the step (unchanged by a step the guard skipped)
        if self.exposure is not None:
            outs["exposed"] = b["exposed"]        # the image the loss read: the view's affine of render_img
            outs["v_affine"] = b["v_affine"]      # dL / d exposure.affine[view_index], 12 floats row-major [3][4]
        if self.bilagrid is not None:
            outs["exposed"] = b["exposed"]          # the image the loss read: the slice of the view's grid applied to render_img
            outs["v_grids"] = b["v_grids"]          # dL / d bilagrid.grids of the step, dense: the view's slab + the TV gradient
            outs["bilagrid_tv"] = b["bilagrid_tv"]  # the total variation of all grids (the loss total holds bilagrid_tv times it)
        if depth_on:
            outs["render_depth"] = b["render_depth"]                       # [H, W]: the expected depth of the step's render
            outs["depth_loss"] = b["depth_rec"][nat.GS_DEPTH_REC_VALUE]    # 0-d, unweighted (the loss total holds lambda_depth times it)
        return TrainStepGraph._StepOutputs(self, outs, lazy=self.handback == "lazy")

    def _poll(self, block: bool):
        """Reads the device-written status words (plain host memory) and retires the steps known to be applied."""
        if block:
            self.stream.synchronize()
        n_isects, _, max_tile, flags, applied, units, rows, live = (int(v) for v in self.status[:8].tolist())
        if live >= 0 and applied > 0:
            self._live_sum, self._live_n = self._live_sum + live, self._live_n + 1
        self.seen_isects = max(self.seen_isects, n_isects)
        self.seen_tile = max(self.seen_tile, max_tile)
        self.seen_units, self.seen_rows = max(self.seen_units, units), max(self.seen_rows, rows)
        done = min(self.confirmed_at_build + applied - self.confirmed, len(self.pending))
        for _ in range(max(done, 0)):
            self.pending.popleft()
        self.confirmed += max(done, 0)
        if flags != 0:
            self._recover(n_isects, max_tile, (units, rows) if flags & (nat.GS_FLAG_UNITS | nat.GS_FLAG_ROWS) else (0, 0))

    def _recover(self, n_isects: int, max_tile: int, walk=(0, 0)):
        """A step did not fit: everything issued after the last applied step was skipped on the device.  Grow, re-capture,
        replay the skipped steps in order."""
        self.stream.synchronize()
        applied = int(self.buf["applied"].item())
        done = self.confirmed_at_build + applied - self.confirmed
        for _ in range(done):
            self.pending.popleft()
        self.confirmed += done
        redo = list(self.pending)
        self.pending.clear()
        self.issued -= len(redo)
        self.stats["overflows"] += 1
        self.stats["replayed_steps"] += len(redo)
        # (what did not fit, and into what: flags 1 = listed intersections, 2 = longest tile list, 4 / 8 = coarse bins, 16 = work units, 32 = rows)
        if int(self.status[nat.GS_INFO_FLAGS]) & nat.GS_FLAG_BACK:   # a frame needed the back round the captured step does not hold
            self._back_needed = True
            self.stats["back_round_needed"] = self.stats.get("back_round_needed", 0) + 1
        self.stats.setdefault("overflow_log", []).append({
            "step": self.confirmed + 1, "flags": int(self.status[nat.GS_INFO_FLAGS]), "isects": n_isects, "longest_list": max_tile, "work_units": walk[0], "rows": walk[1],
            "capacities": [self.cap, self.cap_tile, self.cap_units, self.cap_rows]})
        for e in redo:   # steps fed from recycled device slots (HostFeed): upload their own inputs again
            src = e.host_src
            if src is not None:
                e.w2c, e.K = src["w2c"].to(self.dev, torch.float32), src["K"].to(self.dev, torch.float32)
                e.gt = HostFeed.to_target(src["image"], self.dev)
                e.mask = src["mask"].to(self.dev, torch.float32) if (self.has_mask and src.get("mask") is not None) else e.mask
        # the probe and the warm-up of the re-build run on the first skipped step's own record: its camera and view, its targets
        # (min_cap >= 1 forces a fresh probe even when only a coarse-bin capacity was exceeded and the list sizes read 0)
        self._build(redo[0], min_cap=max(n_isects, 1), min_cap_tile=max_tile, min_walk=walk)
        for e in redo:
            self._issue(e)

    def finish(self):
        """Blocks until every issued step is known to be applied (replaying overflowed ones)."""
        while self.pending:
            self._poll(block=True)

    LOSS_RING = 4096   # steps of loss history kept on the device

    def loss_history(self, last_n: int) -> Tensor:
        """[last_n, 3] = {l1, 1-ssim, total} of the last `last_n` APPLIED steps since the latest (re-)build, oldest first
        (one device read; call after `finish()`).  The `loss3` tensor `step()` returns is only the latest launch's value and
        is meaningless for a step the guard skipped -- this log is written by applied steps only."""
        applied = int(self.buf["applied"].item())
        n = max(0, min(int(last_n), applied, self.LOSS_RING))
        idx = (torch.arange(applied - n, applied, device=self.dev)) % self.LOSS_RING
        return self.buf["loss_ring"][idx]

    def report(self) -> Dict[str, Any]:
        extra = dict(scale_reg=True, max_scale_ratio=self.max_scale_ratio, lambda_scale=self.lambda_scale) if self.scale_reg else {}
        if self.mcmc is not None:
            extra.update(mcmc=True, mcmc_reg=self.mcmc_reg, mcmc_seed=self.mcmc.seed, mcmc_noise_lr=self.mcmc.noise_lr)
        for option, prefix, _, state in self._tables:   # (like the two above: a runner without the feature reports what it always reported)
            extra.update({option: True, prefix + "_lr": getattr(self, prefix + "_lr"), prefix + "_steps": state.step})
        if self.bilagrid is not None:
            extra.update(bilagrid_tv=self.bilagrid_tv)
        if self.depth is not None:
            extra.update(depth=True, lambda_depth=self.lambda_depth, depth_mode=self.depth.mode)
        return dict(self.stats, **extra, binning=self.binning, probed_isects=self.probed[0], probed_longest_list=self.probed[1],
                    probed_coarse_entries=getattr(self, "probed_coarse", (0, 0))[0] if self.binning == "bins" else 0,
                    capacity_isects=self.cap, capacity_tile_list=self.cap_tile, capacity_work_units=self.cap_units,
                    capacity_rows=self.cap_rows, probed_work_units=self.probed_walk[0], probed_rows=self.probed_walk[1],
                    seen_work_units=self.seen_units, seen_rows=self.seen_rows, steps=self.confirmed,
                    graph=self.graph is not None, rounds=bool(self.rounds_on), round_fraction=self.round_fraction if self.rounds_on else None,
                    front_round_alone=bool(self.rounds_on and self.front_only))


class ViewParallelGraphStep(TrainStepGraph):
    """The view-parallel step (one view per rank, `distributed.ViewParallelStep`'s two collectives) with everything in front of
    the first collective as ONE replayable hipGraph:

        [graph: projection .. blend forward .. loss .. blend backward .. row sums + this rank's all-gather record + guard words]
        -> all-gather (async) || projection backward from the sums, gradients + statistics into the bucket
        -> all-reduce (async) || SH half of Adam from the gathered records  ->  geometry half of Adam + statistics  ->  status

    The four launches behind the graph and the two collectives are enqueued per step (they take the step's learning rates and
    step count as launch arguments).  Capacities, step guard and overflow recovery are `TrainStepGraph`'s -- with one addition:
    a rank that skips a step on the device must take every replica with it, and every replica must notice at the same step.
    So each rank's guard flag travels inside both collectives (`gs_guard_flag_out` -> one word of the record, one of the
    bucket) and is ORed into every rank's guard in front of the kernels that apply the step (`gs_guard_merge`); and the status
    words are polled BLOCKING every `check_every` steps, so that all ranks re-size, re-capture and replay the same steps in
    the same order (a rank that found the flag sixteen steps before its peers would issue other collectives than they).
    `vp`: a `ViewParallelStep(model, optimizer, force_exchange=..., guard_words=True)`; the model must hand raw parameters to the
    rasterizer (`fuse_activations`, the default)."""

    def __init__(self, model, optimizer, loss_computer, data, gt_img, mask=None, vp=None, **kw):
        if kw.get("camera_model", "pinhole") != "pinhole":
            raise ValueError("ViewParallelGraphStep: camera_model='pinhole' only -- the view-parallel step's projection backward takes the "
                             "row sums (project_bwd_kernel<DEG, ADAM, SUMS = true>), a variant that does not exist for "
                             f"camera_model={kw['camera_model']!r} yet")
        if (kw.get("rasterize_mode") or getattr(model, "rasterize_mode", "classic")) != "classic":
            raise ValueError("ViewParallelGraphStep: rasterize_mode='classic' only -- the view-parallel step's projection backward takes the "
                             "row sums (project_bwd_kernel<DEG, ADAM, SUMS = true>), a variant that does not exist in the antialiased mode yet")
        if kw.get("poses") is not None:
            raise ValueError("ViewParallelGraphStep: no `poses` -- pose refinement inside the captured step is single-GPU "
                             "(TrainStepGraph(poses=...)): the view-parallel step has no camera gradient")
        if kw.get("exposure") is not None:
            raise ValueError("ViewParallelGraphStep: no `exposure` -- exposure compensation inside the captured step is single-GPU "
                             "(TrainStepGraph(exposure=...)): the view-parallel step's loss reads each rank's raw render")
        if kw.get("bilagrid") is not None:
            raise ValueError("ViewParallelGraphStep: no `bilagrid` -- bilateral grids inside the captured step are single-GPU "
                             "(TrainStepGraph(bilagrid=...)): the view-parallel step's loss reads each rank's raw render")
        if kw.get("depth") is not None:
            raise ValueError("ViewParallelGraphStep: no `depth` -- depth supervision inside the captured step is single-GPU "
                             "(TrainStepGraph(depth=...)): the view-parallel exchange carries three colour channels")
        if kw.get("visible_adam"):
            raise ValueError("ViewParallelGraphStep: no `visible_adam` -- the view-parallel step's two Adam halves (gs_sh_adam_views, "
                             "gs_adam_step_stats) have no form over the visible Gaussians (adam_step_visible_kernel carries no statistics)")
        if kw.get("mcmc") is not None:
            raise ValueError("ViewParallelGraphStep: no `mcmc` -- MCMCStrategy refuses torch.distributed (the replicas would need "
                             "broadcast draws)")
        if vp is None or not vp.exchange or not vp.native or not vp.guard_words:
            raise ValueError("ViewParallelGraphStep needs a native ViewParallelStep(..., guard_words=True) with the exchange on")
        if not vp._raw_parameters():
            raise ValueError("ViewParallelGraphStep: the model must pass its raw parameters (fuse_activations)")
        self.vp = vp
        kw["fuse_adam"] = False
        super().__init__(model, optimizer, loss_computer, data, gt_img, mask, **kw)

    def _lay(self, first: int):
        """... and, once per build, what the view-parallel step needs beside the layout: the row sums, the record and the bucket."""
        super()._lay(first)
        if first == 0:
            self.buf["row_sums"] = self._take("row_sums", (self.N, 12), torch.float32)
            self.vp._records(); self.vp._bucket()   # (the record and the bucket the graph writes into: made before the capture)

    def _enqueue_rest(self, st: int):
        """The captured part ends with this rank's all-gather record: the row sums, and the guard flag into the record and the bucket."""
        L, b, N, vp = nat.lib(), self.buf, self.N, self.vp
        sp, flat = vp._records()[0].data_ptr(), vp._bucket()[2]
        self._ck(L.gs_row_sums(st, 1, N, _p(b["radii"]), _p(b["colors_post"]), self._tpg(), _p(b["cum_tiles"]), _p(b["rows"]),
                                _p(b["row_base"]), _p(b["qmask"]), _p(b["row_sums"]), sp, sp + 4 * 3 * N, float(max(self.H, self.W)), _p(b["viewmats"]),
                                sp + 4 * 4 * N), "gs_row_sums")
        # this rank's guard flag: into its record and into the bucket (both collectives carry it)
        self._ck(L.gs_guard_flag_out(st, _p(b["info"]), sp + 4 * (4 * N + 16), flat.data_ptr() + 4 * vp._flag_off), "gs_guard_flag_out")

    def _tail(self, t: int, lrs):
        """Behind the graph: the two collectives and the four launches that apply the step (on the runner's stream)."""
        import torch.distributed as dist
        L, b, m, vp, opt = nat.lib(), self.buf, self.model, self.vp, self.opt
        st = self._st()
        N, W, H, world = self.N, self.W, self.H, vp.world
        P = vp.record_len()
        send, recv = vp._records()
        _, offs, flat = vp._bucket()
        seg = lambda i, n: flat.data_ptr() + 4 * offs[i]   # noqa: E731
        w_gather = dist.all_gather_into_tensor(recv, send, group=vp.group, async_op=True)
        vp.collectives += 1

        def apply():
            nat.check(L.gs_project_bwd(st, 1, N, self.K, int(m.active_sh_degree), _p(m.means), _p(m.quats), _p(m.log_scales), _p(m.sh_0),
                                       _p(m.sh_rest) if self.K > 1 else None, 0, _p(b["viewmats"]), _p(b["Ks"]), W, H, EPS2D, NEAR_PLANE, FAR_PLANE, _p(b["radii"]),
                                       _p(b["colors_post"]), self._tpg(), _p(b["cum_tiles"]), _p(b["rows"]), _p(b["row_base"]), _p(b["qmask"]),
                                       seg(0, 3 * N), seg(2, 4 * N), seg(1, 3 * N), seg(3, N), None, None, _p(b["v_abs"]), None, None, None, None,
                                       _p(m.logit_opacities), 1, _p(b["sh_jac"]), _p(b["row_sums"]), seg(4, N), seg(5, N)), "gs_project_bwd")
            if self.scale_reg:   # each replica adds it (the eager exchange: flat[o:o+n].add_(p.grad)); Adam's 1 / world makes it count once
                self._scale_reg(seg(1, 3 * N), nat.check)
            w_sum = dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=vp.group, async_op=True)
            vp.collectives += 1
            w_gather.wait()
            nat.check(L.gs_guard_merge(st, _p(b["info"]), recv.data_ptr() + 4 * (4 * N + 16), world, P), "gs_guard_merge")
            lr = dict(zip([g["name"] for g, _ in opt._plist], lrs))
            m0, v0 = opt.moments_of(m.sh_0)
            mr, vr = opt.moments_of(m.sh_rest) if self.K > 1 else (None, None)
            b1, b2 = opt.defaults["betas"]
            nat.check(L.gs_sh_adam_views(st, world, N, self.K, int(m.active_sh_degree), _p(m.means), recv.data_ptr(), P, _p(m.sh_0), _p(m0), _p(v0),
                                         _p(m.sh_rest) if self.K > 1 else None, _p(mr), _p(vr), float(lr["sh_0"]), float(lr["sh_rest"]), float(b1),
                                         float(b2), float(opt.defaults["eps"]), int(t), 1.0 / world, _p(m.max_radii)), "gs_sh_adam_views")
            w_sum.wait()
            nat.check(L.gs_guard_merge(st, _p(b["info"]), flat.data_ptr() + 4 * vp._flag_off, 1, 0), "gs_guard_merge")
            ns = len(opt._plist)
            grads = {"means": seg(0, 3 * N), "log_scales": seg(1, 3 * N), "quats": seg(2, 4 * N), "logit_opacities": seg(3, N)}
            gptr = (ct.c_void_p * ns)(*[grads.get(g["name"]) for g, _ in opt._plist])
            nat.check(L.gs_adam_step_stats(st, opt.flat_param.numel(), _p(opt.flat_param), _p(opt.exp_avg), _p(opt.exp_avg_sq), ns,
                                           (ct.c_int64 * ns)(*opt._ends), (ct.c_int64 * ns)(*opt._lens), gptr, (ct.c_float * ns)(*lrs), float(b1),
                                           float(b2), float(opt.defaults["eps"]), int(t), 1.0 / world, N, seg(4, N), seg(5, N),
                                           _p(m.grad_norm_accum), _p(m.collecting_counts)), "gs_adam_step_stats")
            nat.check(L.gs_step_applied(st, _p(b["info"]), _p(b["applied"])), "gs_step_applied")
            nat.check(L.gs_step_status(st, _p(b["info"]), _p(b["applied"]), self.status.data_ptr(), _p(b["loss3"]), _p(b["loss_ring"]),
                                       self.LOSS_RING, _p(b["walk_state"])), "gs_step_status")
        self._guarded(apply)

    def _poll(self, block: bool):
        # every rank must find an overflow at the SAME step: the status words are read behind a synchronisation, never early
        super()._poll(block=True)


class HostFeed:
    """The loop the way the reference feeds it (/root/reference/train.py:36-43 `DataLoader(pin_memory=True)`, :97
    `data_to_device`, scene/data_class.py:158-162): every step's camera, target image and mask come from PAGE-LOCKED HOST
    memory -- 33 MB per step at 1080p, 23 GB/s at 700 it/s.  The reference uploads them on the compute stream in front of the
    forward; here they cross PCIe on a copy stream into one of `n_slots` device slots while the previous step computes, and the
    step waits for exactly that upload (an event), not for the caller's stream:

        feed = HostFeed(runner)                      # runner: TrainStepGraph
        for batch in loader:                         # batch: {"w2c", "K", "width", "height", "image"[, "mask"][, "view_index"]} pinned host tensors
            feed.step(batch)

    A slot is refilled once the step that read it last has run -- the copy stream waits for that (an event on the runner's
    stream), and so does the HOST: a feeder is never more than `n_slots` steps ahead of the device, a DataLoader's prefetch depth.
    (Unthrottled, the enqueueing thread ran hundreds of uploads ahead and stalled for 8-15 ms at a time inside the runtime's copy
    path: 645 it/s instead of 695 at the bench workload.)  A step the device SKIPPED behind a capacity overflow is replayed from
    a fresh upload of its own host tensors (`step(host_src=...)`), so recycling the slots never feeds a replay another step's
    image; the host tensors themselves must stay untouched until the step is retired (a DataLoader's pinned batches are: each is
    a new allocation).
    `image` may be uint8 [H, W, 3] (8 MB instead of 25 MB across the link): it is widened on the copy stream with the
    reference's own arithmetic, `float32(x) / 255` (a true division: bit-identical to `Frame.to_data`'s numpy expression).
    Measured and not kept (round 6, tools/host_feed_probe.py; 33 MB per step, the link 55 GB/s on an idle GPU): the batch pulled
    across by a KERNEL of 8 / 32 / 128 workgroups instead of the DMA engine -- 17-19 GB/s whatever its size, 1.70 / 1.94 / 2.00 ms
    per step; the image split over 2 / 4 / 8 copy streams -- 656 / 637 / 602 it/s against 680 on one.  A concurrent GEMM slows the
    same DMA batch from 0.64 to 7.1 ms: how fast the link is under load is the platform's business."""

    def __init__(self, runner: "TrainStepGraph", n_slots: int = 2, inputs_ready: bool = False):
        """`inputs_ready`: the caller's promise of `TrainStepGraph.step` (its stream holds no pending reader of the outputs, the
        parameters or the statistics) -- the uploads themselves are ordered by events either way."""
        if runner.depth is not None:
            raise NotImplementedError("HostFeed: a runner built with `depth` -- the feed uploads image, mask and camera, not a depth "
                                      "target; hand device depth maps to runner.step(..., gt_depth=...)")
        self.r, self.n = runner, max(2, int(n_slots))
        self.inputs_ready = bool(inputs_ready)
        dev = runner.dev
        self.copy_stream = torch.cuda.Stream(dev)
        H, W = runner.H, runner.W
        f32 = dict(dtype=torch.float32, device=dev)
        self.gt = [torch.empty((H, W, 3), **f32) for _ in range(self.n)]
        self.u8 = [None] * self.n
        self.mask = [torch.empty((H, W), **f32) if runner.has_mask else None for _ in range(self.n)]
        self.w2c = [torch.empty((4, 4), **f32) for _ in range(self.n)]
        self.K = [torch.empty((3, 3), **f32) for _ in range(self.n)]
        self.done = [None] * self.n
        self._t255 = torch.full((), 255.0, **f32)
        self.i = 0

    @staticmethod
    def to_target(image: Tensor, dev) -> Tensor:
        """A host image as the loss kernels read it: float32 [H, W, 3] on the device (uint8: / 255 as the reference's loader)."""
        x = image.to(dev, non_blocking=False)
        if x.dtype == torch.uint8:
            return torch.div(x.to(torch.float32), torch.full((), 255.0, dtype=torch.float32, device=dev))
        return x.to(torch.float32)

    def step(self, batch: Dict[str, Any]):
        r, j = self.r, self.i % self.n
        self.i += 1
        if (int(batch["width"]), int(batch["height"])) != (r.W, r.H):
            raise ValueError("HostFeed: one frame size per feed (build another for another size)")
        cs = self.copy_stream
        if self.done[j] is not None:
            self.done[j].synchronize()    # (the host: never more than n_slots steps ahead)
            cs.wait_event(self.done[j])   # the step that read this slot last has run
        img = batch["image"]
        with torch.cuda.device(r.dev), torch.cuda.stream(cs):
            self.w2c[j].copy_(batch["w2c"], non_blocking=True)
            self.K[j].copy_(batch["K"], non_blocking=True)
            if img.dtype == torch.uint8:
                if self.u8[j] is None:
                    self.u8[j] = torch.empty(tuple(img.shape), dtype=torch.uint8, device=r.dev)
                self.u8[j].copy_(img, non_blocking=True)
                torch.div(self.u8[j].to(torch.float32), self._t255, out=self.gt[j])
            else:
                self.gt[j].copy_(img, non_blocking=True)
            if r.has_mask:
                self.mask[j].copy_(batch["mask"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        per_view = r.poses is not None or r.exposure is not None or r.bilagrid is not None
        view = batch.get("view_index") if per_view else None   # (poses / exposure / bilagrid: the batch names its row of the tables)
        out = r.step({"w2c": self.w2c[j], "K": self.K[j], "width": r.W, "height": r.H}, self.gt[j], self.mask[j] if r.has_mask else None,
                     inputs_ready=self.inputs_ready, ready_event=ev, host_src=batch, view_index=view)
        self.done[j] = torch.cuda.Event()
        self.done[j].record(r.stream)
        return out
