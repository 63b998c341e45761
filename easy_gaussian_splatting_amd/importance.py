"""Scoring Gaussians by their blend weights and pruning by the scores (INTEGRATION.md "Pruning by contribution").

    stats = importance.collect(model, views)              # one blend_weights() per view, totals on the device
    drop = importance.prune_mask(stats, min_views_hit=1)  # bool [N], True = drop
    model.prune(drop)

`rendering.blend_weights` gives the per-view scores -- per (camera, Gaussian) the sum and the maximum of the blend weight w = alpha * T
over the pixels the blend took, and their number --; `BlendWeightStats` folds views into per-Gaussian totals (`gs_score_accumulate`, one
launch per view, no host read); `prune_mask` turns totals into a drop mask the way RadSplat (maximum weight), LightGaussian /
Mini-Splatting (summed weight, hit count) and Taming-3DGS rank Gaussians; `GaussianModel.prune` removes them.  Single process only:
view-parallel scoring is not implemented and every entry point here refuses `is_distributed()`."""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, Optional

import torch
from torch import Tensor

from .distributed import is_distributed

RANK_BY = ("weight_sum", "weight_max", "hits")


def _refuse_distributed(what: str) -> None:
    if is_distributed():
        raise RuntimeError(f"{what}: blend-weight scoring is single-process only (every rank would have to see every view's scores; "
                           "view-parallel scoring is not implemented)")


class BlendWeightStats:
    """Per-Gaussian totals over the views added so far:
      weight_sum  f64 [N]  sum of the per-view weight sums, views (and the cameras of a view) added in order
      weight_max  f32 [N]  maximum of the per-view maxima
      hits        i64 [N]  taken pixels (int32 overflows at 4K over a few hundred views)
      views_seen  i32 [N]  views with radii > 0
      views_hit   i32 [N]  views with hits > 0
    and `n_views`, the number of cameras added (a Python int).  `fused=True` (default): HIP tensors go through one `gs_score_accumulate`
    launch; CPU tensors, or `fused=False`, through plain torch with the same semantics -- the same bits.  Nothing here reads the device."""

    def __init__(self, n: int, device=None, fused: bool = True):
        self.n, self.device, self.fused = int(n), torch.device("cpu" if device is None else device), bool(fused)
        self.reset()

    def reset(self) -> None:
        z = lambda dt: torch.zeros((self.n,), dtype=dt, device=self.device)
        self.weight_sum, self.weight_max, self.hits = z(torch.float64), z(torch.float32), z(torch.int64)
        self.views_seen, self.views_hit = z(torch.int32), z(torch.int32)
        self.n_views = 0

    def add(self, per_view: Dict[str, Tensor]) -> "BlendWeightStats":
        """Folds the dict `rendering.blend_weights` returns ([C,N] each; a [N] entry counts as one camera) into the totals."""
        ws, wm, hits, radii = (per_view[k] for k in ("weight_sum", "weight_max", "hits", "radii"))
        ws, wm, hits, radii = (t.reshape(-1, t.shape[-1]) for t in (ws, wm, hits, radii))
        C = ws.shape[0]
        for t, dt in ((ws, torch.float32), (wm, torch.float32), (hits, torch.int32), (radii, torch.int32)):
            if t.shape != (C, self.n) or t.dtype != dt or t.device != self.weight_sum.device:
                raise ValueError(f"BlendWeightStats.add: expected [C,{self.n}] float32 / float32 / int32 / int32 tensors on "
                                 f"{self.weight_sum.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        if C == 0:
            return self
        if self.fused and ws.is_cuda:
            if self.n > 0:
                from . import _native as nat
                ws, wm, hits, radii = (t.contiguous() for t in (ws, wm, hits, radii))
                with torch.cuda.device(ws.device):
                    nat.check(nat.lib().gs_score_accumulate(
                        torch.cuda.current_stream(ws.device).cuda_stream, C, self.n, ws.data_ptr(), wm.data_ptr(), hits.data_ptr(),
                        radii.data_ptr(), self.weight_sum.data_ptr(), self.weight_max.data_ptr(), self.hits.data_ptr(),
                        self.views_seen.data_ptr(), self.views_hit.data_ptr()), "gs_score_accumulate")
        else:
            for c in range(C):   # cameras in order: the float64 sum is a sequence of additions, not a reduction
                self.weight_sum += ws[c].to(torch.float64)
                self.weight_max = torch.maximum(self.weight_max, wm[c])
                self.hits += hits[c].to(torch.int64)
                self.views_seen += (radii[c] > 0).to(torch.int32)
                self.views_hit += (hits[c] > 0).to(torch.int32)
        self.n_views += C
        return self

    def add_view(self, model, data: Dict[str, Any]) -> "BlendWeightStats":
        """Scores one view of `model` (a `GaussianModel`) and adds it; the call is built from the model and the data dict the way
        `GaussianModel.forward` builds its render: raw parameters + in-kernel activations on the GPU, the model's `tile_culling` and
        `rasterize_mode`, `data.get("camera_model", "pinhole")`."""
        from .rendering import blend_weights
        _refuse_distributed("BlendWeightStats.add_view")
        raw = model.means.is_cuda and getattr(model, "fuse_activations", True)
        with torch.no_grad():
            return self.add(blend_weights(
                model.means, model.quats, model.log_scales if raw else model.scales, model.logit_opacities if raw else model.opacities,
                data["w2c"][None], data["K"][None], data["width"], data["height"],
                rasterize_mode=getattr(model, "rasterize_mode", "classic"), camera_model=data.get("camera_model", "pinhole"),
                _activations="exp_sigmoid" if raw else "none", _tile_culling=getattr(model, "tile_culling", "tight")))


def collect(model, views: Iterable[Dict[str, Any]], fused: bool = True) -> BlendWeightStats:
    """The totals of `model` over the data dicts `views` (what `GaussianModel.forward` takes)."""
    _refuse_distributed("importance.collect")
    stats = BlendWeightStats(model.nbr_gaussians, model.means.device, fused=fused)
    for data in views:
        stats.add_view(model, data)
    return stats


def prune_mask(stats: BlendWeightStats, *, min_weight_max: Optional[float] = None, min_views_hit: Optional[int] = None,
               keep_fraction: Optional[float] = None, rank_by: str = "weight_sum") -> Tensor:
    """bool [N], True = drop.  The criteria OR together:
      min_weight_max  drop where the largest blend weight over all views stayed below it (RadSplat's rule)
      min_views_hit   drop where fewer views than this took the Gaussian at any pixel
      keep_fraction   keep the ceil(keep_fraction * N) Gaussians that rank highest by `rank_by` ("weight_sum" | "weight_max" | "hits"),
                      drop the rest; equal scores rank by index, the lower one first -- the result is deterministic.
    No criterion: nothing is dropped.  Pure torch on whatever device the totals live on."""
    _refuse_distributed("importance.prune_mask")
    if rank_by not in RANK_BY:
        raise ValueError(f"rank_by: one of {RANK_BY} (got {rank_by!r})")
    if keep_fraction is not None and not (0.0 <= float(keep_fraction) <= 1.0):
        raise ValueError(f"keep_fraction: a share in [0, 1] (got {keep_fraction!r})")
    n = stats.n
    drop = torch.zeros((n,), dtype=torch.bool, device=stats.weight_sum.device)
    if min_weight_max is not None:
        drop |= stats.weight_max < float(min_weight_max)
    if min_views_hit is not None:
        drop |= stats.views_hit < int(min_views_hit)
    if keep_fraction is not None and n > 0:
        k = min(n, int(math.ceil(float(keep_fraction) * n)))
        order = torch.sort(getattr(stats, rank_by), descending=True, stable=True).indices   # (stable: ties keep index order)
        drop[order[k:]] = True
    return drop
