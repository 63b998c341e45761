"""Reference of the depth render modes ("D", "ED", "RGB+D", "RGB+ED"), composed from the oracle as it is: `TO.project(...)[2]` for
the depths (fp64, differentiable w.r.t. means and view matrices), `TO.spherical_harmonics` for SH colours, the oracle's
`rasterization(sh_degree=None)` over cat(colours, depths) with a zero background on the depth channel, and the ED division in fp64
torch on top.  Shared by tests/test_depth_host.py and tests/test_gpu_depth.py; also the scenes of those tests and the GPU runner."""
import numpy as np
import torch

from oracle import c_oracle as CO
from oracle import torch_oracle as TO
from scenes import make_scene

GEO = ("means", "quats", "scales", "opacities")
MODES = ("D", "ED", "RGB+D", "RGB+ED")
ED_FLOOR = 1e-10


def scene(name):
    """The five scenes of the depth tests (razor share and coverage measured on the CPU oracle when they were chosen)."""
    if name == "A":   # every pixel covered
        return make_scene(1500, 100, 80, sh_degree=0, n_views=2, seed=23, scale_range=(0.02, 0.2), dist=4.0)
    if name == "B":
        return make_scene(1500, 100, 80, sh_degree=3, n_views=2, seed=61, scale_range=(0.02, 0.2), dist=4.0)
    if name == "C":   # footprints of up to all 35 tiles: runs of more than 64 gradient rows per Gaussian
        return make_scene(300, 100, 80, sh_degree=1, n_views=1, seed=62, scale_range=(0.3, 1.5), dist=4.0)
    if name == "D":   # ragged tiles
        return make_scene(777, 67, 45, sh_degree=2, n_views=2, seed=63, scale_range=(0.02, 0.3), dist=4.0)
    if name == "E":   # 78 % of the pixels uncovered
        return make_scene(60, 100, 80, sh_degree=1, n_views=1, seed=64, scale_range=(0.02, 0.1), dist=4.0)
    raise KeyError(name)


def razor(sc, **proj):
    """[C,H,W] pixels within 1e-4 of a blend discontinuity (the contributor sets do not depend on the colours)."""
    fw = CO.render(sc["means"], sc["quats"], sc["scales"], sc["opacities"], np.zeros((sc["means"].shape[0], 3)), sc["viewmats"], sc["Ks"],
                   int(sc["width"]), int(sc["height"]), sh_degree=None, dtype=np.float64, **proj)
    return CO.blend_margin(fw, mu_tol_ulps=1.0, conic_rtol=2.4e-7) < 1e-4


def upstream(rz, D, seed):
    """Random upstream gradients of the image [C,H,W,D] and the alphas, zero on the razor pixels."""
    g = torch.Generator().manual_seed(seed)
    C, H, W = rz.shape
    keep = torch.from_numpy(~rz).double()[..., None]
    return torch.randn((C, H, W, D), generator=g, dtype=torch.float64) * keep, torch.randn((C, H, W, 1), generator=g, dtype=torch.float64) * keep


def expected_depth(acc, alpha):
    """ED on top of an accumulated image: the last channel divided by alpha.clamp(min=1e-10)."""
    return torch.cat([acc[..., :-1], acc[..., -1:] / alpha.clamp(min=ED_FLOOR)], dim=-1)


def reference(sc, mode, colors, sh_degree, bg, vc, va, cam=False, **proj):
    """fp64 composed oracle.  colors: a list of leaves -- [shs] / [sh_0, sh_rest] with sh_degree, [features [N,D] or [C,N,D]]
    without.  Returns dict(img, alpha, acc (the accumulated image), grads (geometry + colour leaves, in order), absgrad,
    v_viewmats (cam=True))."""
    f64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    W, H = int(sc["width"]), int(sc["height"])
    ins = [f64(sc[k]).requires_grad_(True) for k in GEO]
    leaves = [f64(c).requires_grad_(True) for c in colors]
    V, Ks = f64(sc["viewmats"]).requires_grad_(cam), f64(sc["Ks"])
    C, N = V.shape[0], ins[0].shape[0]
    radii, _, depths, _ = TO.project(ins[0], ins[1], ins[2], V, Ks, W, H, **{k: v for k, v in proj.items()})
    if mode in ("D", "ED"):
        cols, bgx = depths[..., None], None
    else:
        if sh_degree is not None:
            base = TO.spherical_harmonics(sh_degree, ins[0], V, torch.cat(leaves, dim=1) if len(leaves) == 2 else leaves[0], radii)
        else:
            base = leaves[0].expand(C, N, -1) if leaves[0].dim() == 2 else leaves[0]
        cols = torch.cat([base, depths[..., None]], dim=-1)
        bgx = None if bg is None else torch.cat([f64(bg), torch.zeros((C, 1), dtype=torch.float64)], dim=1)
    acc, alpha, meta = TO.rasterization(*ins, cols, V, Ks, W, H, sh_degree=None, packed=False, backgrounds=bgx, absgrad=True, **proj)
    img = expected_depth(acc, alpha) if mode.endswith("ED") else acc
    loss = (img * vc).sum() + (alpha * va).sum()
    wrt = ins + leaves + ([V] if cam else [])
    gs = torch.autograd.grad(loss, wrt, allow_unused=True)
    out = dict(img=img.detach(), alpha=alpha.detach(), acc=acc.detach(), grads=list(gs[:len(ins) + len(leaves)]), absgrad=meta["means2d"].absgrad)
    if cam:
        out["v_viewmats"] = gs[-1]
    return out


def gpu(sc, mode, colors, sh_degree, bg, vc=None, va=None, cam=False, grad=True, culling="gsplat", **kw):
    """One forward (+ backward) of rasterization(render_mode=mode) on the GPU; the same arguments as `reference`."""
    from easy_gaussian_splatting_amd.rendering import rasterization
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    d = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(d)
    ins = [to(sc[k]).requires_grad_(grad) for k in GEO]
    leaves = [to(c).requires_grad_(grad) for c in colors]
    V = to(sc["viewmats"]).requires_grad_(cam)
    extra = dict(_camera_grads=True) if cam else {}
    with torch.set_grad_enabled(grad):
        img, alpha, meta = rasterization(*ins, tuple(leaves) if len(leaves) == 2 else leaves[0], V, to(sc["Ks"]), int(sc["width"]),
                                         int(sc["height"]), sh_degree=sh_degree, packed=False, backgrounds=None if bg is None else to(bg),
                                         absgrad=True, render_mode=mode, _tile_culling=culling, **extra, **kw)
    out = dict(img=img.detach(), alpha=alpha.detach(), meta=meta)
    if grad:
        f = lambda x: x.to(d).float() if torch.is_tensor(x) else to(x)
        loss = (img * f(vc)).sum() + (0.0 if va is None else (alpha * f(va)).sum())
        gs = torch.autograd.grad(loss, ins + leaves + ([V] if cam else []), allow_unused=True)
        out.update(grads=list(gs[:len(ins) + len(leaves)]), absgrad=meta["means2d"].absgrad)
        if cam:
            out["v_viewmats"] = gs[-1]
    torch.cuda.synchronize()
    return out
