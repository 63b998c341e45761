"""Depth supervision: gsplat's trainer's depth term on the expected depth of the render (`model(data, depth="ED")["render_depth"]`)
against a target depth map from a sensor, from SfM points or from a monocular prior.  For a frame of H*W pixels

    valid = (t > 0) & isfinite(t)          a NaN, an inf, zero and negatives all mean "no measurement"
    w     = valid * (1 - mask)             LossComputer's mask convention: mask = 1 excludes a pixel; no mask: 0
    e     = d - t                          mode="depth"
          = disp(d) - 1 / t                mode="disparity" (gsplat's trainer), disp(d) = 1 / d where d > 0, else 0
    depth_loss = sum(w |e|) / sum(w)       exactly 0 when sum(w) == 0

In the eager loop: `total = loss["total"] + lambda_depth * depth_loss(out["render_depth"], gt_depth, mask, mode)`, through the HIP
kernels of csrc/gs_depth_loss.hip (`fused=True`, the default: fp64 sums in a fixed order, reproducible bits) or as the plain torch
expression (`fused=False`, the semantic reference, any device and dtype).  In the captured step:
`TrainStepGraph(..., depth=DepthSupervision(lambda_depth, mode), gt_depth=t)` and `step(..., gt_depth=t)`.  See INTEGRATION.md
"Supervising depth"."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

MODES = ("depth", "disparity")   # their index is the library's GS_DEPTH_MODE_*


def _mode_index(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"depth_loss: mode {mode!r}, expected 'depth' or 'disparity'")
    return MODES.index(mode)


class DepthSupervision:
    """The settings of the depth term for `TrainStepGraph(depth=...)`: `lambda_depth` weighs `depth_loss` in the total, `mode` is
    "depth" or "disparity".  The runner copies `lambda_depth` into `runner.lambda_depth`, a plain attribute staged every step."""

    def __init__(self, lambda_depth: float = 1e-2, mode: str = "disparity"):
        _mode_index(mode)
        lam = float(lambda_depth)
        if lam != lam or lam < 0.0:
            raise ValueError(f"DepthSupervision: lambda_depth {lambda_depth!r} must be a number >= 0")
        self.lambda_depth, self.mode = lam, mode

    def __repr__(self):
        return f"DepthSupervision(lambda_depth={self.lambda_depth}, mode={self.mode!r})"


def _check_shapes(render_depth: Tensor, gt_depth: Tensor, mask: Optional[Tensor]):
    """(H, W) of the frame; ValueError for anything that does not fit -- before any device work."""
    if not (render_depth.dim() == 2 or (render_depth.dim() == 3 and render_depth.shape[2] == 1)):
        raise ValueError(f"depth_loss: render_depth of shape {tuple(render_depth.shape)}, expected [H, W, 1] or [H, W]")
    H, W = int(render_depth.shape[0]), int(render_depth.shape[1])
    if H == 0 or W == 0:
        raise ValueError("depth_loss: an empty frame")
    if tuple(gt_depth.shape) != (H, W):
        raise ValueError(f"depth_loss: gt_depth of shape {tuple(gt_depth.shape)}, expected {(H, W)}")
    if mask is not None and tuple(mask.shape) != (H, W):
        raise ValueError(f"depth_loss: mask of shape {tuple(mask.shape)}, expected {(H, W)}")
    for name, t in (("gt_depth", gt_depth), ("mask", mask)):
        if t is not None and t.device != render_depth.device:
            raise ValueError(f"depth_loss: {name} on {t.device}, render_depth on {render_depth.device}")
    return H, W


def depth_loss_torch(render_depth: Tensor, gt_depth: Tensor, mask: Optional[Tensor] = None, mode: str = "depth") -> Tensor:
    """The plain-torch statement of the formula, in `render_depth`'s dtype, differentiable by autograd."""
    _mode_index(mode)
    H, W = _check_shapes(render_depth, gt_depth, mask)
    d = render_depth.reshape(H, W)
    t = gt_depth.to(d.dtype)
    valid = torch.isfinite(t) & (t > 0)
    w = valid.to(d.dtype) if mask is None else valid.to(d.dtype) * (1 - mask.to(d.dtype))
    t_safe = torch.where(valid, t, torch.ones_like(t))
    if mode == "depth":
        e = d - t_safe
    else:   # (the reciprocal of a d <= 0 never enters the graph: its gradient would be 0 * inf)
        pos = d > 0
        e = torch.where(pos, 1 / torch.where(pos, d, torch.ones_like(d)), torch.zeros_like(d)) - 1 / t_safe
    num = (w * torch.where(valid, e.abs(), torch.zeros_like(e))).sum()
    den = w.sum()
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))


class _DepthLoss(torch.autograd.Function):
    """HIP path (csrc/gs_depth_loss.hip): one image-sized pass and a one-block finish forward, one pass backward."""

    @staticmethod
    def forward(ctx, depth: Tensor, target: Tensor, mask: Optional[Tensor], mode: int):
        from . import _native as nat
        L = nat.lib()
        H, W = depth.shape
        dev = depth.device
        rec = torch.zeros((nat.GS_DEPTH_REC_FLOATS,), dtype=torch.float32, device=dev)
        partials = torch.empty((int(L.gs_depth_loss_partials_doubles(H, W)),), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_depth_loss_fwd(st, H, W, rec.data_ptr(), mode, target.data_ptr(), None if mask is None else mask.data_ptr(),
                                          depth.data_ptr(), partials.data_ptr()), "gs_depth_loss_fwd")
        ctx.save_for_backward(depth, target, mask, rec)
        ctx.mode = mode
        return rec[nat.GS_DEPTH_REC_VALUE].clone()

    @staticmethod
    def backward(ctx, v_loss: Tensor):
        from . import _native as nat
        L = nat.lib()
        depth, target, mask, rec = ctx.saved_tensors
        H, W = depth.shape
        dev = depth.device
        v = v_loss.to(torch.float32).reshape(1).contiguous()
        v_depth = torch.empty_like(depth)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_depth_loss_bwd(st, H, W, rec.data_ptr(), ctx.mode, target.data_ptr(), None if mask is None else mask.data_ptr(),
                                          depth.data_ptr(), v.data_ptr(), v_depth.data_ptr()), "gs_depth_loss_bwd")
        return v_depth, None, None, None


def _aligned(t: Tensor) -> Tensor:
    """Contiguous float32 at a 16-byte aligned address (a view into the middle of a buffer is copied)."""
    t = t.to(torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def depth_loss(render_depth: Tensor, gt_depth: Tensor, mask: Optional[Tensor] = None, mode: str = "depth", fused: bool = True) -> Tensor:
    """The unweighted 0-d depth loss of one frame (module docstring).  `render_depth`: [H, W, 1] or [H, W], what
    `GaussianModel.forward(data, depth="ED")["render_depth"]` returns; `gt_depth` [H, W]; `mask` [H, W] or None.
    `fused=True`: an `autograd.Function` over the HIP kernels -- tensors on a HIP device only, float32, the gradient reaches
    `render_depth`; `ValueError` for a shape or a device that does not fit, before any device work.  `fused=False`: plain torch."""
    if not fused:
        return depth_loss_torch(render_depth, gt_depth, mask, mode)
    m = _mode_index(mode)
    H, W = _check_shapes(render_depth, gt_depth, mask)
    if render_depth.dtype != torch.float32:
        raise ValueError(f"depth_loss(fused=True): render_depth of dtype {render_depth.dtype}, expected float32")
    if render_depth.device.type != "cuda":
        raise ValueError(f"depth_loss(fused=True): tensors on {render_depth.device}; the HIP kernels need a HIP device (fused=False is plain torch)")
    d = render_depth.reshape(H, W).contiguous()   # (the model's [H, W, 1] is a strided view of the 4-channel render: one copy)
    d = d if d.data_ptr() % 16 == 0 else d.clone()
    return _DepthLoss.apply(d, _aligned(gt_depth.detach()), None if mask is None else mask.detach().to(torch.float32).contiguous(), m)
