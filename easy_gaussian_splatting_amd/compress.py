"""A compact file of a trained model: a k-means codebook over the higher SH bands, 8/16-bit affine quantisation of everything else,
the Gaussians in Morton order of their means, deflated (DESIGN.md "Exporting a trained model").

The container is `numpy.savez_compressed`; the layout is this project's own, versioned by the `format` entry:

    format            the string FORMAT
    meta              a JSON string: n, sh_degree, active_sh_degree, background, bits, sh_clusters and the constructor's settings
    means             uint16 [N, 3]   of sign(v) log1p(|v|)
    log_scales        uint8  [N, 3]
    quats             uint8  [N, 4]   of the unit quaternion with w >= 0
    logit_opacities   uint8  [N, 1]
    sh_0              uint8  [N, 3]
    sh_labels         uint16 [N] (uint32 beyond 65 536 clusters)   } absent at SH degree 0
    sh_codebook       uint8  [K, 3 ((deg + 1)^2 - 1)]              }
    ranges            float32 [R, 2]  {lo, hi} of every channel, in the order above (the codebook: ONE range)

Quantisation is per channel and affine in the quantised domain T(v) (the identity but for the means):
q = clamp(rint((T(v) - T(lo)) / (T(hi) - T(lo)) (2^b - 1)), 0, 2^b - 1), lo / hi the channel's minimum / maximum, stored as the
float32 values they are; hi == lo gives q = 0 and the value back exactly.  The arithmetic is float64: T(v) comes back within half
a step, (T(hi) - T(lo)) / (2^b - 1) / 2.  The permutation is not stored: a load yields the same set of Gaussians in another order,
so renders differ from the uncompressed model's only by the quantisation and where two Gaussians tie in depth.
"""
from __future__ import annotations

import json
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native as nat
from .kmeans import kmeans
from .model import GaussianModel

FORMAT = "easy-gaussian-splatting-amd/compact/1"
DEFAULT_BITS = {"means": 16, "log_scales": 8, "quats": 8, "logit_opacities": 8, "sh_0": 8, "sh_rest": 8}
_SETTINGS = ("densify_grad_thresh", "densify_scale_thresh", "num_splits", "prune_radii_ratio_thresh", "prune_scale_thresh", "min_opacity",
             "means_lr_init", "means_lr_final", "means_lr_schedule_max_steps", "use_scale_regularization", "max_scale_ratio",
             "white_background", "fuse_sh_cat")


def log_domain(v: Tensor) -> Tensor:
    """sign(v) log1p(|v|): the domain the means are quantised in (steps grow with the distance from the origin)"""
    return torch.sign(v) * torch.log1p(torch.abs(v))


def log_domain_inverse(t: Tensor) -> Tensor:
    return torch.sign(t) * torch.expm1(torch.abs(t))


def _levels(bits: int) -> int:
    if isinstance(bits, bool) or not isinstance(bits, int) or not 1 <= bits <= 16:
        raise ValueError(f"a width must be an integer in [1, 16] bits, got {bits!r}")
    return (1 << bits) - 1


def quantize(v: Tensor, bits: int, transform: Optional[Callable[[Tensor], Tensor]] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """v [N, C] float32 -> (q [N, C] uint8 (bits <= 8) or int32 holding a uint16, lo [C], hi [C] float32): the formula of the module's
    header, per channel, `transform` = T.  A NaN or an infinity raises ValueError."""
    levels = _levels(bits)
    if v.dim() != 2 or v.dtype != torch.float32:
        raise ValueError(f"a [N, C] float32 tensor, got {tuple(v.shape)} {v.dtype}")
    if not bool(torch.isfinite(v).all()):
        raise ValueError("a non-finite value cannot be quantised")
    if v.shape[0] == 0:
        z = torch.zeros((v.shape[1],), dtype=torch.float32, device=v.device)
        return torch.zeros(v.shape, dtype=torch.uint8 if bits <= 8 else torch.int32, device=v.device), z, z.clone()
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    T = transform if transform is not None else (lambda t: t)
    t, tlo, thi = T(v.double()), T(lo.double()), T(hi.double())
    span = thi - tlo
    q = torch.where(span > 0, (t - tlo) / torch.where(span > 0, span, torch.ones_like(span)) * levels, torch.zeros_like(t))
    q = torch.clamp(torch.round(q), 0, levels)   # (torch.round: half to even, rint)
    return q.to(torch.uint8 if bits <= 8 else torch.int32), lo, hi


def dequantize(q: Tensor, lo: Tensor, hi: Tensor, bits: int, transform: Optional[Callable[[Tensor], Tensor]] = None,
               inverse: Optional[Callable[[Tensor], Tensor]] = None) -> Tensor:
    """-> float64 [N, C] in the value domain: T^-1(T(lo) + q (T(hi) - T(lo)) / (2^b - 1)); a channel with hi == lo gives lo exactly."""
    levels = _levels(bits)
    T = transform if transform is not None else (lambda t: t)
    Ti = inverse if inverse is not None else (lambda t: t)
    lo64, hi64 = lo.double(), hi.double()
    tlo, thi = T(lo64), T(hi64)
    out = Ti(tlo + q.double() * ((thi - tlo) / levels))
    return torch.where((hi64 > lo64).expand_as(out), out, lo64.expand_as(out))


def _spread3(v: np.ndarray) -> np.ndarray:
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x001f00000000ffff), (16, 0x001f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton_order(means: Tensor) -> Tensor:
    """int64 [N]: the indices of `means` [N, 3] sorted (stably) by the 63-bit Morton code of the points inside their bounding box --
    `gs_knn_codes` (csrc/gs_knn.hip) on a HIP device, the same code in numpy for a CPU tensor."""
    n = int(means.shape[0])
    if n < 2:
        return torch.arange(n, dtype=torch.int64, device=means.device)
    pts = means.detach().float().contiguous()
    if pts.device.type == "cuda":
        L, dev = nat.lib(), pts.device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            ws = torch.empty((int(L.gs_knn_workspace_bytes(n)),), dtype=torch.uint8, device=dev)
            codes = torch.empty((n,), dtype=torch.int64, device=dev)
            nat.check(L.gs_knn_codes(st, n, pts.data_ptr(), ws.data_ptr(), codes.data_ptr()), "gs_knn_codes")
            return torch.sort(codes, stable=True).indices
    p = pts.numpy()
    lo, ext = p.min(0), p.max(0) - p.min(0)
    code = np.zeros((n,), dtype=np.uint64)
    for a in range(3):
        inv = np.float32(1.0) / ext[a] if 0 < ext[a] < np.inf else np.float32(0.0)
        t = np.clip((p[:, a] - lo[a]) * inv, np.float32(0.0), np.float32(1.0))
        code |= _spread3(np.minimum((t * np.float32(2097151.0)).astype(np.uint32), 2097151)) << np.uint64(a)
    return torch.from_numpy(np.argsort(code.astype(np.int64), kind="stable"))


def _settings(model: GaussianModel) -> Dict[str, object]:
    s = model.means_lr_scheduler
    bg = [float(b) for b in model.BACKGROUND.detach().cpu()]
    return {"densify_grad_thresh": model.DENSIFY_GRAD_THRESH, "densify_scale_thresh": model.DENSIFY_SCALE_THRESH, "num_splits": model.NUM_SPLITS,
            "prune_radii_ratio_thresh": model.PRUNE_RADII_RATIO_THRESH, "prune_scale_thresh": model.PRUNE_SCALE_THRESH,
            "min_opacity": model.MIN_OPACITY, "means_lr_init": s.lr_init, "means_lr_final": s.lr_final,
            "means_lr_schedule_max_steps": s.max_steps, "use_scale_regularization": bool(model.USE_SCALE_REGULARIZATION),
            "max_scale_ratio": float(model.MAX_SCALE_RATIO), "white_background": all(b == 1.0 for b in bg),
            "fuse_sh_cat": bool(getattr(model, "fuse_sh_cat", True))}


def _np_codes(q: Tensor, bits: int) -> np.ndarray:
    return q.cpu().numpy().astype(np.uint8 if bits <= 8 else np.uint16)


@torch.no_grad()
def save_compact(model: GaussianModel, path, sh_clusters: int = 65536, sh_iters: int = 5, bits: Optional[Dict[str, int]] = None,
                 generator: Optional[torch.Generator] = None) -> Dict[str, object]:
    """Writes `model` to `path` in the layout of the module's header and returns the `meta` record.  `sh_clusters` / `sh_iters` /
    `generator` go to `kmeans.kmeans` over `sh_rest.reshape(N, -1)` in the model's own order (the labels are permuted afterwards);
    a model of no more Gaussians than clusters keeps its rows as the codebook and needs no device.  `bits` overrides DEFAULT_BITS by
    array name (1..16; `sh_rest`: the codebook's width).  A non-finite parameter raises ValueError before anything is written."""
    widths = dict(DEFAULT_BITS)
    for name, b in (bits or {}).items():
        if name not in widths:
            raise ValueError(f"bits: no array named {name!r} (one of {sorted(widths)})")
        _levels(b)
        widths[name] = b
    arrays = {name: getattr(model, name).detach() for name in ("means", "log_scales", "quats", "logit_opacities", "sh_0", "sh_rest")}
    for name, t in arrays.items():
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} holds a NaN or an infinity: refusing to export the model")
    n, degree = int(arrays["means"].shape[0]), int(model.MAX_SH_DEGREE)
    order = morton_order(arrays["means"])
    quats = arrays["quats"].double()   # normalised in float64 and rounded once: the float32 nearest the unit quaternion
    quats = (quats / quats.norm(dim=1, keepdim=True).clamp_min(1e-300)).float()
    quats = torch.where(quats[:, :1] < 0, -quats, quats)
    planes = {"means": arrays["means"].float().reshape(n, 3), "log_scales": arrays["log_scales"].float().reshape(n, 3), "quats": quats,
              "logit_opacities": arrays["logit_opacities"].float().reshape(n, 1), "sh_0": arrays["sh_0"].float().reshape(n, 3)}
    out: Dict[str, np.ndarray] = {}
    ranges = []
    for name, v in planes.items():
        q, lo, hi = quantize(v[order].contiguous(), widths[name], log_domain if name == "means" else None)
        out[name] = _np_codes(q, widths[name])
        ranges.append(torch.stack([lo, hi], dim=1).cpu())
    k = 0
    if degree > 0:
        flat = arrays["sh_rest"].float().reshape(n, -1).contiguous()
        codebook, labels, _ = kmeans(flat, sh_clusters, iters=sh_iters, generator=generator)
        k = int(codebook.shape[0])
        q, lo, hi = quantize(codebook.reshape(-1, 1), widths["sh_rest"])
        out["sh_codebook"] = _np_codes(q, widths["sh_rest"]).reshape(k, -1)
        out["sh_labels"] = labels.long()[order].cpu().numpy().astype(np.uint16 if k <= 65536 else np.uint32)
        ranges.append(torch.stack([lo, hi], dim=1).cpu())
    meta = {"n": n, "sh_degree": degree, "active_sh_degree": int(model.active_sh_degree), "sh_clusters": k, "bits": widths,
            "background": [float(b) for b in model.BACKGROUND.detach().cpu()], "rasterize_mode": getattr(model, "rasterize_mode", "classic"),
            "settings": _settings(model)}
    out["ranges"] = torch.cat(ranges, dim=0).numpy().astype(np.float32)
    with open(path, "wb") as f:   # (a file object: savez would append ".npz" to a name)
        np.savez_compressed(f, format=np.array(FORMAT), meta=np.array(json.dumps(meta)), **out)
    return meta


def read_compact(path) -> Tuple[Dict[str, object], Dict[str, Tensor]]:
    """-> (meta, arrays): the dequantised float32 CPU tensors of a compact file -- means [N, 3], log_scales [N, 3], quats [N, 4],
    logit_opacities [N], sh_0 [N, 1, 3], sh_rest [N, K - 1, 3] -- in the file's (Morton) order."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or str(z["format"]) != FORMAT:
            raise ValueError(f"{path}: not a compact model file of format {FORMAT!r}")
        meta = json.loads(str(z["meta"]))
        data = {name: z[name] for name in z.files if name not in ("format", "meta")}
    n, degree, widths = int(meta["n"]), int(meta["sh_degree"]), meta["bits"]
    ranges = torch.from_numpy(data["ranges"].astype(np.float32))
    arrays: Dict[str, Tensor] = {}
    row = 0
    for name, c in (("means", 3), ("log_scales", 3), ("quats", 4), ("logit_opacities", 1), ("sh_0", 3)):
        q = torch.from_numpy(data[name].astype(np.int32))
        if tuple(q.shape) != (n, c):
            raise ValueError(f"{path}: {name} is {tuple(q.shape)}, the header says {(n, c)}")
        lo, hi = ranges[row:row + c, 0], ranges[row:row + c, 1]
        row += c
        logd = name == "means"
        arrays[name] = dequantize(q, lo, hi, int(widths[name]), log_domain if logd else None, log_domain_inverse if logd else None).float()
    arrays["logit_opacities"] = arrays["logit_opacities"].reshape(n)
    arrays["sh_0"] = arrays["sh_0"].reshape(n, 1, 3)
    coeffs = (degree + 1) ** 2 - 1
    if degree > 0:
        k = int(meta["sh_clusters"])
        q = torch.from_numpy(data["sh_codebook"].astype(np.int32))
        labels = torch.from_numpy(data["sh_labels"].astype(np.int64))
        if tuple(q.shape) != (k, 3 * coeffs) or tuple(labels.shape) != (n,) or (n and int(labels.max()) >= k):
            raise ValueError(f"{path}: the codebook is {tuple(q.shape)} with labels up to {int(labels.max()) if n else 0}, the header says {k} clusters")
        codebook = dequantize(q.reshape(-1, 1), ranges[row:row + 1, 0], ranges[row:row + 1, 1], int(widths["sh_rest"])).float().reshape(k, coeffs, 3)
        arrays["sh_rest"] = codebook[labels]
    else:
        arrays["sh_rest"] = torch.zeros((n, 0, 3), dtype=torch.float32)
    return meta, arrays


def load_compact(path, device=None) -> GaussianModel:
    """The model of a compact file: a `GaussianModel` with the file's settings, its parameters on `device` (default: the HIP device
    when there is one, as `checkpoint.load_gaussian_model`), which `Evaluator`, `FrameRenderer` and `forward` take as they take a
    checkpoint's.  No optimizer: a compact file is for rendering, not for resuming."""
    meta, arrays = read_compact(path)
    settings = {k: v for k, v in meta["settings"].items() if k in _SETTINGS}
    model = GaussianModel(sh_degree=int(meta["sh_degree"]), **arrays, **settings)
    model.active_sh_degree = int(meta["active_sh_degree"])
    model.BACKGROUND.data = torch.tensor(meta["background"], dtype=torch.float32)
    if meta.get("rasterize_mode", "classic") != "classic":
        model.rasterize_mode = meta["rasterize_mode"]
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    return model.to(device)
