"""Held-out evaluation as the reference does it (the reference's eval.py): `Evaluator` (PSNR / SSIM / LPIPS / fps over a
loader, :22-73) and `evaluate_output` (its `eval(training_output_path, iterations)`, :76-133).

On the GPU the two torchmetrics figures of a view come from ONE fused HIP pass, `gs_image_metrics` (csrc/gs_metrics.hip):
`{mse, ssim}` of the mask-composited render against the ground truth, written into row i of a device buffer that is read back
once, after the last view -- the reference's loop reads three scalars back per view (`.item()`).  PSNR is formed on the host:
torchmetrics' `PeakSignalNoiseRatio(data_range=1.0)` is `10 log10(1 / mse)` (a float data_range does not clamp), `inf` where
`mse == 0`.  `image_metrics` on CPU tensors (and for images that are not `[H, W, 3]` float32) states the same metric in plain
torch: `loss.ssim` plus a mean of squares.

LPIPS.  The reference's third figure is torchmetrics' `LearnedPerceptualImagePatchSimilarity("vgg", normalize=True)`, whose VGG
weights this package neither ships nor fetches.  `Evaluator(lpips=...)` takes any callable `(gt[1,3,H,W], img[1,3,H,W]) -> scalar
tensor`; where torchmetrics and its weights are installed that is the reference's own object:

    from torchmetrics.image import LearnedPerceptualImagePatchSimilarity
    evaluator = Evaluator(cfg.eval_render_num, lpips=LearnedPerceptualImagePatchSimilarity("vgg", normalize=True).cuda())

Without one the key is there and NaN.
"""
from __future__ import annotations

import math
import random
import time
from pathlib import Path
from typing import Any, Callable, Dict, Optional

import numpy as np
import torch
from torch import Tensor

from .loss import ssim

_WORKSPACES: Dict[Any, Tensor] = {}   # (device, stream) -> the kernel's partial sums; grows to the largest image seen


def _workspace(dev: torch.device, stream: int, floats: int) -> Tensor:
    key = (dev, stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < floats:
        ws = _WORKSPACES[key] = torch.empty((floats,), dtype=torch.float32, device=dev)
    return ws


def _check_inputs(render_img: Tensor, gt_img: Tensor, mask: Optional[Tensor]) -> None:
    """The refusals of `loss._fused_inputs`, for every path: the kernel reads `gt_img` as `render_img`'s shape and `mask` as
    `[H, W]` on `render_img`'s device through bare pointers."""
    if tuple(gt_img.shape) != tuple(render_img.shape):
        raise ValueError(f"gt_img has shape {tuple(gt_img.shape)}, render_img {tuple(render_img.shape)}")
    if gt_img.device != render_img.device:
        raise ValueError(f"gt_img is on {gt_img.device}, render_img on {render_img.device}")
    if mask is not None:
        if tuple(mask.shape) != tuple(render_img.shape[:2]):
            raise ValueError(f"mask has shape {tuple(mask.shape)}, expected {tuple(render_img.shape[:2])}")
        if mask.device != render_img.device:
            raise ValueError(f"mask is on {mask.device}, render_img on {render_img.device}")


@torch.no_grad()
def image_metrics(render_img: Tensor, gt_img: Tensor, mask: Optional[Tensor] = None, clamp_input: bool = False,
                  out: Optional[Tensor] = None) -> Tensor:
    """-> `[2]` = {mse, ssim} of `c = mask * gt + (1 - mask) * render` against `gt_img` (`render_img` clamped to [0, 1] first with
    `clamp_input`): the mean of `(c - gt)^2` over all elements and the mean SSIM (11 x 11 window, sigma 1.5, data range 1) over
    the interior.  `render_img`, `gt_img`: `[H, W, C]`; `mask`: `[H, W]` or None.  `out`: where to write them (a row of a
    caller's `[n, 2]` float32 buffer on `render_img`'s device); without it a new tensor.
    `[H, W, 3]` float32 tensors on the GPU go through `gs_image_metrics` -- no allocation beyond a cached workspace, nothing
    read back; anything else through plain torch.  `gt_img` / `mask` of another float dtype are cast."""
    if render_img.dim() != 3:
        raise ValueError(f"render_img must be [H, W, C], got {tuple(render_img.shape)}")
    _check_inputs(render_img, gt_img, mask)
    if out is not None and (tuple(out.shape) != (2,) or out.device != render_img.device):
        raise ValueError(f"out must be a [2] tensor on {render_img.device}, got {tuple(out.shape)} on {out.device}")
    fused = render_img.device.type == "cuda" and render_img.dtype == torch.float32 and render_img.shape[2] == 3
    if gt_img.dtype != render_img.dtype:
        gt_img = gt_img.to(render_img.dtype)
    if mask is not None and mask.dtype != render_img.dtype:
        mask = mask.to(render_img.dtype)
    if fused:
        from . import _native as nat
        L = nat.lib()
        dev = render_img.device
        H, W = int(render_img.shape[0]), int(render_img.shape[1])
        if out is None:
            out = torch.empty((2,), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor")
        r, g = render_img.contiguous(), gt_img.contiguous()
        m = None if mask is None else mask.contiguous()
        st = torch.cuda.current_stream(dev).cuda_stream
        ws = _workspace(dev, st, int(L.gs_metrics_workspace_floats(H, W)))
        with torch.cuda.device(dev):
            nat.check(L.gs_image_metrics(st, H, W, r.data_ptr(), g.data_ptr(), None if m is None else m.data_ptr(), int(clamp_input),
                                         ws.data_ptr(), out.data_ptr()), "gs_image_metrics")
        return out
    vals = _torch_metrics(render_img, gt_img, mask, clamp_input)
    if out is None:
        return vals
    out.copy_(vals)
    return out


def _torch_metrics(render_img: Tensor, gt_img: Tensor, mask: Optional[Tensor], clamp_input: bool = False) -> Tensor:
    """The two metrics in plain torch on any device: the composite, a mean of squares and `loss.ssim`."""
    c = torch.clamp(render_img, min=0.0, max=1.0) if clamp_input else render_img
    if mask is not None:
        m = mask.unsqueeze(2)
        c = m * gt_img + (1.0 - m) * c
    return torch.stack([torch.mean((c - gt_img) ** 2), ssim(gt_img.permute(2, 0, 1)[None], c.permute(2, 0, 1)[None])])


def psnr_from_mse(mse: np.ndarray) -> np.ndarray:
    """10 log10(1 / mse) in float64, `inf` where mse == 0 (torchmetrics' PeakSignalNoiseRatio(data_range=1.0) of one image)."""
    mse = np.asarray(mse, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(mse > 0, -10.0 * np.log10(np.where(mse > 0, mse, 1.0)), np.inf)


def _model_device(model) -> Optional[torch.device]:
    """Where `data_to_device` sends a view: the device of the model's parameters.  A model without parameters (any callable)
    gets the views where the loader left them."""
    params = getattr(model, "parameters", None)
    if callable(params):
        for p in params():
            return p.device
    return None


class Evaluator:
    """The reference's `Evaluator` (the reference's eval.py:22-73).  `evaluator(dataloader, model)` -> dict with `psnr`, `ssim`,
    `lpips` (means over the views), `fps`, `fps_host` and `render_1 .. render_k`: `eval_render_num` views picked with
    `random.sample` as the reference picks them, each `torch.cat((gt, render), dim=1)` as a numpy array `[H, 2 W, 3]`.

    Nothing is read back inside the loop: every view's {mse, ssim} goes into row i of one device buffer (`image_metrics`), the
    picked renders and the `lpips` callable's scalars stay on the device, and all of it is read once after the last view.
    `fps` is views per second of DEVICE time of `model(data)` (one event pair per view, read after the final synchronise);
    `fps_host` is the reference's own figure, `time.time()` around `model(data)` without a synchronise -- here `model(data)` returns
    with the list stages and the blend still enqueued, so `fps_host` leaves most of a frame out.  On CPU tensors
    both are the host figure.
    Everything runs on the caller's current stream.  `fused=False` takes the plain-torch metrics on every device.
    (The reference ends with `torch.cuda.empty_cache()`; this one leaves the allocator alone: it runs between training steps.)"""

    def __init__(self, eval_render_num: int, lpips: Optional[Callable[[Tensor, Tensor], Tensor]] = None, fused: bool = True) -> None:
        self.eval_render_num = eval_render_num
        self.lpips = lpips
        self.fused = fused

    def _metrics(self, render_img: Tensor, gt_img: Tensor, mask: Optional[Tensor], out: Tensor) -> None:
        if self.fused:
            image_metrics(render_img, gt_img, mask, out=out)
            return
        _check_inputs(render_img, gt_img, mask)
        out.copy_(_torch_metrics(render_img, gt_img.to(render_img.dtype), None if mask is None else mask.to(render_img.dtype)))

    @torch.no_grad()
    def __call__(self, dataloader, model) -> Dict[str, Any]:
        from .scene import data_to_device
        n = len(dataloader)
        if n == 0:
            raise ValueError("Evaluator: the dataloader is empty")
        render_indexes = list(range(n))
        if len(render_indexes) > self.eval_render_num:
            render_indexes = random.sample(render_indexes, k=self.eval_render_num)
        target = _model_device(model)
        buf, events, renders, lpips_vals = None, [], [], []
        cost = 0.0
        for i, data in enumerate(dataloader):
            if target is not None and data.get("mask") is not None:
                data_to_device(data, non_blocking=False, device=target)
            elif target is not None:   # (a view without a mask: the same move of what is there)
                for k in ("K", "w2c", "image"):
                    data[k] = data[k].to(target, non_blocking=False)
            timed = data["image"].device.type == "cuda"
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            t0 = time.time()
            model_output = model(data)
            t1 = time.time()
            if timed:
                e1.record()
                events.append((e0, e1))
            cost += t1 - t0
            gt_img: Tensor = data["image"]
            mask: Optional[Tensor] = data.get("mask")
            render_img: Tensor = model_output["render_img"]
            if buf is None:
                buf = torch.empty((n, 2), dtype=torch.float32, device=render_img.device)
            self._metrics(render_img, gt_img, mask, buf[i])
            if self.lpips is not None:
                c = render_img if mask is None else mask.unsqueeze(2) * gt_img + (1.0 - mask.unsqueeze(2)) * render_img
                lpips_vals.append(torch.as_tensor(self.lpips(gt_img.permute(2, 0, 1)[None, ...], c.permute(2, 0, 1)[None, ...])).detach().reshape(()))
            if i in render_indexes:
                renders.append(torch.cat((gt_img, render_img), dim=1))
        # ---- the one synchronise and read-back
        if events:
            torch.cuda.current_stream(buf.device).synchronize()
        vals = buf.cpu().double().numpy()
        metrics: Dict[str, Any] = {"psnr": float(np.mean(psnr_from_mse(vals[:, 0]))), "ssim": float(np.mean(vals[:, 1])),
                                   "lpips": float(torch.stack(lpips_vals).double().mean().cpu()) if lpips_vals else math.nan}
        for k, r in enumerate(renders):
            metrics[f"render_{k + 1}"] = r.cpu().numpy()
        metrics["fps_host"] = n / cost if cost > 0 else math.inf
        metrics["fps"] = n / (sum(a.elapsed_time(b) for a, b in events) * 1e-3) if events else metrics["fps_host"]
        return metrics


def _cfg_get(cfg, key: str):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def evaluate_output(training_output_path, iterations: Optional[int] = None, cfg=None) -> Dict[str, Dict[str, Any]]:
    """The reference's `eval(training_output_path, iterations)` (the reference's eval.py:76-133): the configuration from
    `<output>/config.yaml` (or `cfg`: a dict or an object with the same names), the model from `<output>/checkpoints/`
    (`iterations=None`: the latest), the `Scene` the run trained on with its repeated `train_indexes` de-duplicated, and the
    `Evaluator` (`eval_render_num = 0`) over the train and the eval set; an empty set is skipped.
    -> `{"train": {...}, "eval": {...}}`, each the evaluator's dict."""
    from torch.utils.data import DataLoader
    from .checkpoint import load_gaussian_model
    from .scene import Scene
    out_path = Path(training_output_path)
    if cfg is None:
        import yaml
        with open(out_path / "config.yaml", "r") as f:
            cfg = yaml.safe_load(f)
    seed = _cfg_get(cfg, "random_seed")   # (the reference's set_global_state: the seeds and the device of the run)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.set_device(_cfg_get(cfg, "device"))
    model = load_gaussian_model(out_path, iterations).eval()
    scene = Scene(_cfg_get(cfg, "data"), _cfg_get(cfg, "data_format"), None, _cfg_get(cfg, "total_iterations"), _cfg_get(cfg, "eval"),
                  _cfg_get(cfg, "eval_split_ratio"), _cfg_get(cfg, "eval_in_val"), _cfg_get(cfg, "eval_in_test"), _cfg_get(cfg, "use_masks"),
                  _cfg_get(cfg, "mask_expand_pixels"), _cfg_get(cfg, "white_background"))
    scene.train_indexes = list(set(scene.train_indexes))
    workers = int(_cfg_get(cfg, "dataloader_workers"))
    first = lambda x: x[0]   # noqa: E731
    evaluator = Evaluator(0)
    results: Dict[str, Dict[str, Any]] = {}
    for name, dataset in (("train", scene.train_dataset), ("eval", scene.eval_dataset)):
        loader = DataLoader(dataset, batch_size=1, pin_memory=torch.cuda.is_available(), num_workers=workers, collate_fn=first)
        if len(loader) == 0:
            continue
        results[name] = evaluator(loader, model)
    return results
