"""Regularising normals for meshing: the term 2DGS, GOF, PGSR, RaDe-GS and gsplat's 2DGS trainer (`normal_loss`) add so that the
rendered depth describes a surface.  Every Gaussian gets a normal -- its rotation's column along its smallest scale, in camera space,
faced towards the camera --, the normals are blended like colours, and the blend is held against the normal of the rendered depth:

    n_d(x, y) = normalise(A x B), A = P(x, y + 1) - P(x, y - 1), B = P(x + 1, y) - P(x - 1, y),
    P(x, y) = d(x, y) * ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)                       (a fronto-parallel plane: (0, 0, -1))
    valid = interior, alpha >= min_alpha and 0 < d < inf at the pixel and its four neighbours, 1e-30 <= |A x B|^2 < inf
    w = valid * (1 - mask)                                                      LossComputer's convention: mask = 1 excludes a pixel
    loss = sum(w (1 - dot(Nb, n_d))) / sum(w)        Nb: the blended, un-normalised normal; exactly 0 when sum(w) == 0

csrc/gs_normals.h is the definition; csrc/gs_normals.hip holds the kernels.  In the eager loop:

    out = render_normals(model, data)
    total = loss["total"] + lambda_normal * normal_consistency_loss(out["render4"], out["alphas"], data["K"])

See INTEGRATION.md "Regularising normals for meshing".  The captured step (`TrainStepGraph`), a viewer mode and non-pinhole cameras
are out of scope."""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch
from torch import Tensor

MIN_LEN2 = 1e-30   # csrc/gs_normals.h: kNormalMinLen2


def _f32c(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


class _GaussianNormals(torch.autograd.Function):
    """HIP path (csrc/gs_normals.hip): one thread per Gaussian forward and backward; the gradient reaches `quats` only."""

    @staticmethod
    def forward(ctx, means: Tensor, quats: Tensor, scales: Tensor, viewmats: Tensor):
        from . import _native as nat
        L = nat.lib()
        N, C, dev = int(means.shape[0]), int(viewmats.shape[0]), means.device
        m, q, s, vm = _f32c(means), _f32c(quats), _f32c(scales), _f32c(viewmats)
        out = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_gauss_normals_fwd(st, N, C, m.data_ptr(), q.data_ptr(), s.data_ptr(), vm.data_ptr(), out.data_ptr()),
                      "gs_gauss_normals_fwd")
        ctx.save_for_backward(m, q, s, vm)
        return out

    @staticmethod
    def backward(ctx, v_normals: Tensor):
        from . import _native as nat
        L = nat.lib()
        m, q, s, vm = ctx.saved_tensors
        N, C, dev = int(m.shape[0]), int(vm.shape[0]), m.device
        v = _f32c(v_normals)
        v_quats = torch.empty((N, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_gauss_normals_bwd(st, N, C, m.data_ptr(), q.data_ptr(), s.data_ptr(), vm.data_ptr(), v.data_ptr(),
                                             v_quats.data_ptr()), "gs_gauss_normals_bwd")
        return None, v_quats, None, None


def gaussian_normals(means: Tensor, quats: Tensor, scales: Tensor, viewmats: Tensor) -> Tensor:
    """[C, N, 3]: the normal of every Gaussian in the space of every camera.  `means` [N, 3], `quats` [N, 4] (wxyz, need not be
    normalised), `scales` [N, 3] (log-scales or activated ones: only their order counts), `viewmats` [C, 4, 4] world -> camera
    (pinhole).  Differentiable with respect to `quats`; `means` and `scales` receive `None` (the axis and the facing are piecewise
    constant).  A `viewmats` that requires grad is refused.  HIP device only: there is no CPU fallback."""
    if viewmats.requires_grad:
        raise NotImplementedError("gaussian_normals: viewmats.requires_grad -- the cameras are constants of the normal term")
    N = int(means.shape[0])
    if tuple(means.shape) != (N, 3) or tuple(quats.shape) != (N, 4) or tuple(scales.shape) != (N, 3):
        raise ValueError(f"gaussian_normals: means {tuple(means.shape)}, quats {tuple(quats.shape)}, scales {tuple(scales.shape)}; "
                         "expected [N, 3], [N, 4], [N, 3]")
    if viewmats.dim() != 3 or tuple(viewmats.shape[1:]) != (4, 4) or viewmats.shape[0] < 1:
        raise ValueError(f"gaussian_normals: viewmats of shape {tuple(viewmats.shape)}, expected [C, 4, 4]")
    if means.device.type != "cuda":
        raise NotImplementedError("gaussian_normals runs on the GPU only; there is no CPU fallback")
    for name, t in (("quats", quats), ("scales", scales), ("viewmats", viewmats)):
        if t.device != means.device:
            raise ValueError(f"gaussian_normals: {name} on {t.device}, means on {means.device}")
    return _GaussianNormals.apply(means, quats, scales, viewmats)


def render_normals(model, data: Dict[str, Any], min_alpha: float = 0.5) -> Dict[str, Any]:
    """One `rasterization(colors=normals, sh_degree=None, render_mode="RGB+ED")` call of `model` under the view `data` (what
    `GaussianModel.forward` takes): the model's raw parameters with `_activations="exp_sigmoid"`, its `rasterize_mode` and
    `tile_culling`, no background.  -> {"render4": [H, W, 4] the blended normals and the expected depth, "alphas": [H, W],
    "normals": the view render4[..., :3], "depth": the view render4[..., 3], "min_alpha": min_alpha}.  Pinhole only."""
    from .rendering import rasterization
    cm = data.get("camera_model", "pinhole")
    if cm != "pinhole":
        raise NotImplementedError(f"render_normals: camera_model {cm!r} is not supported -- the depth normal un-projects through a "
                                  "pinhole, and a fisheye or orthographic depth is not a z-depth along its columns")
    w2c = data["w2c"]
    viewmats = w2c[None] if w2c.dim() == 2 else w2c
    normals = gaussian_normals(model.means, model.quats, model.log_scales, viewmats)
    rmode = getattr(model, "rasterize_mode", "classic")
    img, alphas, _ = rasterization(
        means=model.means, quats=model.quats, scales=model.log_scales, opacities=model.logit_opacities, colors=normals, sh_degree=None,
        viewmats=viewmats, Ks=data["K"][None] if data["K"].dim() == 2 else data["K"], width=data["width"], height=data["height"],
        backgrounds=None, packed=False, render_mode="RGB+ED", _tile_culling=getattr(model, "tile_culling", "tight"),
        _activations="exp_sigmoid", **({} if rmode == "classic" else {"rasterize_mode": rmode}))
    render4 = img[0]
    return {"render4": render4, "alphas": alphas[0, ..., 0], "normals": render4[..., :3], "depth": render4[..., 3],
            "min_alpha": float(min_alpha)}


def _check_frame(what: str, H: int, W: int, alphas: Tensor, K: Tensor, mask: Optional[Tensor], ref: Tensor) -> None:
    if H == 0 or W == 0:
        raise ValueError(f"{what}: an empty frame")
    if tuple(alphas.shape) not in ((H, W), (H, W, 1)):
        raise ValueError(f"{what}: alphas of shape {tuple(alphas.shape)}, expected {(H, W)}")
    if tuple(K.shape) != (3, 3):
        raise ValueError(f"{what}: K of shape {tuple(K.shape)}, expected (3, 3)")
    if mask is not None and tuple(mask.shape) != (H, W):
        raise ValueError(f"{what}: mask of shape {tuple(mask.shape)}, expected {(H, W)}")
    for name, t in (("alphas", alphas), ("K", K), ("mask", mask)):
        if t is not None and t.device != ref.device:
            raise ValueError(f"{what}: {name} on {t.device}, the render on {ref.device}")


def _min_alpha(what: str, min_alpha: float) -> float:
    a = float(min_alpha)
    if a != a:
        raise ValueError(f"{what}: min_alpha is NaN")
    return a


def _depth_normals_torch(d: Tensor, alphas: Tensor, K: Tensor, min_alpha: float):
    """(n_d [H-2, W-2, 3], valid [H-2, W-2]) of the interior pixels, in d's dtype, differentiable with respect to d"""
    H, W = d.shape
    dt, dev = d.dtype, d.device
    ok = (alphas >= min_alpha) & torch.isfinite(d) & (d > 0)
    ds = torch.where(ok, d, torch.ones_like(d))
    K = K.to(dt)
    u = ((torch.arange(W, device=dev, dtype=dt) + 0.5) - K[0, 2]) / K[0, 0]
    v = ((torch.arange(H, device=dev, dtype=dt) + 0.5) - K[1, 2]) / K[1, 1]
    P = torch.stack([ds * u[None, :], ds * v[:, None], ds], -1)
    A = P[2:, 1:-1] - P[:-2, 1:-1]
    B = P[1:-1, 2:] - P[1:-1, :-2]
    c = torch.cross(A, B, dim=-1)
    len2 = (c * c).sum(-1)
    valid = ok[1:-1, 1:-1] & ok[2:, 1:-1] & ok[:-2, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & torch.isfinite(len2) & (len2 >= MIN_LEN2)
    length = torch.where(valid, len2, torch.ones_like(len2)).sqrt()
    return c / length[..., None], valid


def normal_consistency_loss_torch(render4: Tensor, alphas: Tensor, K: Tensor, mask: Optional[Tensor] = None, min_alpha: float = 0.5,
                                  detach_depth: bool = False) -> Tensor:
    """The plain-torch statement of the formula, in `render4`'s dtype, on any device, differentiable by autograd."""
    if render4.dim() != 3 or render4.shape[2] != 4:
        raise ValueError(f"normal_consistency_loss: render4 of shape {tuple(render4.shape)}, expected [H, W, 4]")
    H, W = int(render4.shape[0]), int(render4.shape[1])
    _check_frame("normal_consistency_loss", H, W, alphas, K, mask, render4)
    min_alpha = _min_alpha("normal_consistency_loss", min_alpha)
    if H < 3 or W < 3:   # no interior pixel: the empty sum, exactly 0 with zero gradients
        return render4[:0].sum()
    dt = render4.dtype
    d = render4[..., 3].detach() if detach_depth else render4[..., 3]
    n, valid = _depth_normals_torch(d, alphas.reshape(H, W).to(dt), K, min_alpha)
    e = 1 - (render4[1:-1, 1:-1, :3] * n).sum(-1)
    w = valid.to(dt) if mask is None else valid.to(dt) * (1 - mask[1:-1, 1:-1].to(dt))
    num = (w * torch.where(valid, e, torch.zeros_like(e))).sum()
    den = w.sum()
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))


class _NormalLoss(torch.autograd.Function):
    """HIP path (csrc/gs_normals.hip): one image pass and a one-block finish forward, one image pass backward."""

    @staticmethod
    def forward(ctx, render4: Tensor, alphas: Tensor, K: Tensor, mask: Optional[Tensor], min_alpha: float, detach_depth: bool):
        from . import _native as nat
        L = nat.lib()
        H, W, _ = render4.shape
        dev = render4.device
        rec = torch.zeros((nat.GS_NORMAL_REC_FLOATS,), dtype=torch.float32, device=dev)
        partials = torch.empty((int(L.gs_normal_loss_partials_doubles(H, W)),), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_normal_loss_fwd(st, H, W, K.data_ptr(), min_alpha, render4.data_ptr(), alphas.data_ptr(),
                                           None if mask is None else mask.data_ptr(), rec.data_ptr(), partials.data_ptr(), None),
                      "gs_normal_loss_fwd")
        ctx.save_for_backward(render4, alphas, K, mask, rec)
        ctx.min_alpha, ctx.detach_depth = min_alpha, detach_depth
        return rec[nat.GS_NORMAL_REC_VALUE].clone()

    @staticmethod
    def backward(ctx, v_loss: Tensor):
        from . import _native as nat
        L = nat.lib()
        render4, alphas, K, mask, rec = ctx.saved_tensors
        H, W, _ = render4.shape
        dev = render4.device
        v = v_loss.to(torch.float32).reshape(1).contiguous()
        v_render4 = torch.empty_like(render4)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_normal_loss_bwd(st, H, W, K.data_ptr(), ctx.min_alpha, 1 if ctx.detach_depth else 0, render4.data_ptr(),
                                           alphas.data_ptr(), None if mask is None else mask.data_ptr(), rec.data_ptr(), v.data_ptr(),
                                           v_render4.data_ptr()), "gs_normal_loss_bwd")
        return v_render4, None, None, None, None, None


def _fused_frame(what: str, image: Tensor, channels: int, alphas: Tensor, K: Tensor, mask: Optional[Tensor]):
    """The checks of the fused entries, before any device work -> (H, W)."""
    if image.dim() != 3 or image.shape[2] != channels:
        raise ValueError(f"{what}: an image of shape {tuple(image.shape)}, expected [H, W, {channels}]")
    H, W = int(image.shape[0]), int(image.shape[1])
    _check_frame(what, H, W, alphas, K, mask, image)
    if image.dtype != torch.float32:
        raise ValueError(f"{what}(fused=True): an image of dtype {image.dtype}, expected float32")
    if image.device.type != "cuda":
        raise ValueError(f"{what}(fused=True): tensors on {image.device}; the HIP kernels need a HIP device (fused=False is plain torch)")
    if H * W * 4 >= 2 ** 31:
        raise ValueError(f"{what}: a frame of {H} x {W} pixels is beyond the kernels' 32-bit offsets")
    return H, W


def _aligned16(t: Tensor) -> Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def normal_consistency_loss(render4: Tensor, alphas: Tensor, K: Tensor, mask: Optional[Tensor] = None, min_alpha: float = 0.5,
                            detach_depth: bool = False, fused: bool = True) -> Tensor:
    """The unweighted 0-d normal-consistency loss of one frame (module docstring).  `render4` [H, W, 4]: the blended normals and the
    expected depth, `render_normals(...)["render4"]`; `alphas` [H, W]; `K` [3, 3]; `mask` [H, W] or None (1 excludes a pixel).
    The gradient reaches `render4`: the normal channels directly, the depth channel through the depth normals of the four
    neighbours -- exact zeros with `detach_depth=True`; `alphas` receive none (validity is a threshold).
    `fused=True`: an `autograd.Function` over the HIP kernels -- float32 tensors on a HIP device; `ValueError` for a shape, a dtype or
    a device that does not fit, before any device work.  `fused=False`: plain torch, any device and dtype: the semantic reference."""
    if not fused:
        return normal_consistency_loss_torch(render4, alphas, K, mask, min_alpha, detach_depth)
    H, W = _fused_frame("normal_consistency_loss", render4, 4, alphas, K, mask)
    min_alpha = _min_alpha("normal_consistency_loss", min_alpha)
    return _NormalLoss.apply(_aligned16(render4), _f32c(alphas).reshape(H, W), _f32c(K), None if mask is None else _f32c(mask),
                             min_alpha, bool(detach_depth))


@torch.no_grad()
def depth_to_normal(depth: Tensor, alphas: Tensor, K: Tensor, min_alpha: float = 0.5, fused: bool = True) -> Tensor:
    """[H, W, 3]: the normal of a z-depth map by central differences (module docstring) where the pixel is valid, zeros elsewhere.
    `depth` [H, W] or [H, W, 1].  Forward only.  `fused=True`: the HIP kernel (float32, HIP device); `fused=False`: plain torch."""
    if depth.dim() == 2:
        depth = depth[..., None]
    if not fused:
        if depth.dim() != 3 or depth.shape[2] != 1:
            raise ValueError(f"depth_to_normal: depth of shape {tuple(depth.shape)}, expected [H, W] or [H, W, 1]")
        H, W = int(depth.shape[0]), int(depth.shape[1])
        _check_frame("depth_to_normal", H, W, alphas, K, None, depth)
        out = torch.zeros((H, W, 3), dtype=depth.dtype, device=depth.device)
        if H >= 3 and W >= 3:
            n, valid = _depth_normals_torch(depth[..., 0], alphas.reshape(H, W).to(depth.dtype), K, _min_alpha("depth_to_normal", min_alpha))
            out[1:-1, 1:-1] = torch.where(valid[..., None], n, torch.zeros_like(n))
        return out
    H, W = _fused_frame("depth_to_normal", depth, 1, alphas, K, None)
    min_alpha = _min_alpha("depth_to_normal", min_alpha)
    from . import _native as nat
    L = nat.lib()
    dev = depth.device
    render4 = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    render4[..., 3] = depth[..., 0]
    a, k = _f32c(alphas).reshape(H, W), _f32c(K)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        nat.check(L.gs_normal_loss_fwd(st, H, W, k.data_ptr(), min_alpha, render4.data_ptr(), a.data_ptr(), None, None, None, out.data_ptr()),
                  "gs_normal_loss_fwd")
    return out
