"""fp64 reference of `rasterization(rasterize_mode="antialiased")`: a torch projection that forms cov2_0, rho and op_eff as DESIGN.md
"Antialiased mode" defines them, laid out like `oracle.torch_oracle.project` and tests/camera_model_ref.py, composed with the oracle's
own `spherical_harmonics`, `isect_tiles`, `isect_offset_encode` and `rasterize_to_pixels` (fed with op_eff); every gradient by
autograd.  Shared by tests/test_antialias_host.py and tests/test_gpu_antialias.py; also their scenes and the GPU runner.

    cov2_0 = J cov_c J^T                 det0 = a0 c0 - b^2        (BEFORE eps2d joins the diagonal)
    cov2   = cov2_0 + eps2d I            det  = a c - b^2          (cull, radius, conic: `TO.project`'s, unchanged)
    rho    = sqrt(max(0, det0 / det))    op_eff = opacity rho, 0 where culled

sqrt(max(., 0)) goes through the double-`where` pattern: at det0 <= 0 (a rank-deficient covariance) the value is 0 and autograd's
gradient of it is 0, not the NaN 0 * inf of sqrt'(0) behind a clamp."""
import math

import numpy as np
import torch

import camera_model_ref as CM
from oracle import torch_oracle as TO

GEO = CM.GEO
_f64 = CM._f64


def rho_of(a0, b, c0, eps2d):
    """rho from the entries of cov2_0: (rho, det0, det)."""
    det0 = a0 * c0 - b * b
    det = (a0 + eps2d) * (c0 + eps2d) - b * b
    q = det0 / det
    pos = q > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q)), det0, det


def project(means, quats, scales, viewmats, Ks, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0):
    """`TO.project` (pinhole) that also returns rho [C,N] (0 where culled): radii, means2d, depths, conics, rho."""
    eps2d, near_plane, far_plane, radius_clip = (float(np.float32(v)) for v in (eps2d, near_plane, far_plane, radius_clip))
    C = viewmats.shape[0]
    Rq = TO.quat_to_rotmat(quats)
    M = Rq * scales[:, None, :]
    covars = M @ M.transpose(-1, -2)
    Rv, tv = viewmats[:, :3, :3], viewmats[:, :3, 3]
    p_c = torch.einsum("cij,nj->cni", Rv, means) + tv[:, None, :]
    cov_c = torch.einsum("cij,njk,clk->cnil", Rv, covars, Rv)
    z = p_c[..., 2]
    depth_ok = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(depth_ok, z, torch.ones_like(z))
    x, y = p_c[..., 0], p_c[..., 1]
    fx, fy = Ks[:, 0, 0][:, None], Ks[:, 1, 1][:, None]
    cx, cy = Ks[:, 0, 2][:, None], Ks[:, 1, 2][:, None]
    lim_x = TO.FOV_CLAMP * (0.5 * width / fx)
    lim_y = TO.FOV_CLAMP * (0.5 * height / fy)
    tx = zs * torch.minimum(lim_x, torch.maximum(-lim_x, x / zs))
    ty = zs * torch.minimum(lim_y, torch.maximum(-lim_y, y / zs))
    O = torch.zeros_like(zs)
    J = torch.stack([fx / zs, O, -fx * tx / (zs * zs), O, fy / zs, -fy * ty / (zs * zs)], dim=-1).reshape(C, -1, 2, 3)
    cov2 = J @ cov_c @ J.transpose(-1, -2)
    means2d = torch.stack([fx * x / zs + cx, fy * y / zs + cy], dim=-1)
    a0, c0 = cov2[..., 0, 0], cov2[..., 1, 1]
    b = 0.5 * (cov2[..., 0, 1] + cov2[..., 1, 0])
    a, c = a0 + eps2d, c0 + eps2d
    det = a * c - b * b
    det_ok = det > 0
    dets = torch.where(det_ok, det, torch.ones_like(det))
    conics = torch.stack([c / dets, -b / dets, a / dets], dim=-1)
    det0 = a0 * c0 - b * b
    q = det0 / dets
    pos = q > 0
    rho = torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))
    with torch.no_grad():
        mid = 0.5 * (a + c)
        lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=TO.RADIUS_DISC_FLOOR))
        radius = torch.ceil(TO.RADIUS_SIGMA * torch.sqrt(lam))
        valid = depth_ok & det_ok & (radius > radius_clip)
        mx, my = means2d[..., 0], means2d[..., 1]
        valid = valid & (mx + radius > 0) & (mx - radius < width) & (my + radius > 0) & (my - radius < height)
        radii = torch.where(valid, radius, torch.zeros_like(radius)).to(torch.int32)
    means2d = torch.where(valid[..., None], means2d, torch.zeros_like(means2d))
    depths = torch.where(valid, z, torch.zeros_like(z))
    conics = torch.where(valid[..., None], conics, torch.zeros_like(conics))
    rho = torch.where(valid, rho, torch.zeros_like(rho))
    return radii, means2d, depths, conics, rho


# ---- scenes ----

def _view(z0, yaw=0.0, pitch=0.0):
    """World -> camera: the cloud's centre at depth z0 on the optical axis, the camera turned about it by (yaw, pitch)."""
    cy_, sy_, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    R = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = (0.0, 0.0, z0)
    return V.astype(np.float32)


def _pinhole(W, H, C, fov_deg=60.0):
    f = (W / 2) / math.tan(math.radians(fov_deg) / 2)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    return np.broadcast_to(K, (C, 3, 3)).copy()


def _cloud(rng, n, W, H, V, Ks, sigma_px, aniso, sh_degree, spread=0.9):
    """n Gaussians over the frame of camera 0, each with the projected sigma (pixels, at camera 0) it is asked for times a per-axis factor."""
    f, z0 = float(Ks[0, 0, 0]), float(V[0, 2, 3])
    half_x, half_y = spread * 0.5 * W / f * z0, spread * 0.5 * H / f * z0
    means = np.stack([rng.uniform(-half_x, half_x, n), rng.uniform(-half_y, half_y, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    p_c = means @ V[0, :3, :3].T.astype(np.float64) + V[0, :3, 3]
    scales = (sigma_px * p_c[:, 2] / f)[:, None] * aniso
    K = (sh_degree + 1) ** 2
    return dict(means=means.astype(np.float32), quats=rng.standard_normal((n, 4)).astype(np.float32), scales=scales.astype(np.float32),
                opacities=rng.uniform(0.1, 0.95, n).astype(np.float32), shs=(0.4 * rng.standard_normal((n, K, 3))).astype(np.float32),
                viewmats=V, Ks=Ks, backgrounds=rng.random((V.shape[0], 3)).astype(np.float32), width=W, height=H, sh_degree=sh_degree)


# the eight degenerate Gaussians of scene Z: scales (s, 0, 0) along the world x axis, turned by quaternions whose rotation matrices are
# exact (the identity and the three half turns), under a camera whose rotation is the identity -- cov2_0 = [[j00^2 s^2, 0], [0, 0]] and
# det0 = 0 hold exactly in any floating-point format.  (A rank-deficient covariance turned by a general rotation has det0 at rounding
# level, either sign: rho is then 0 or ~1e-8, an effective opacity far below the blend's 1/255 either way.)
Z_DEGENERATE = 8
_Z_QUATS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))


def scene(name):
    """A: 64 x 48, 300 Gaussians, projected sigma log-uniform in 0.06 .. 8 px (per-axis factors 1 .. 1.5 on top), one camera, SH3.
    B: 40 x 24 (ragged tiles), two cameras, 120 Gaussians: a third with whole-frame footprints (sigma 15 .. 40 px), the rest sub-pixel
    (0.12 .. 0.6 px), SH2.  Z: 64 x 48, 40 ordinary Gaussians and, first in the arrays, the eight degenerate ones."""
    if name == "A":
        rng = np.random.default_rng(241)
        W, H, n = 64, 48, 300
        V, Ks = _view(3.0, 0.25, -0.15)[None], _pinhole(W, H, 1)
        sigma = np.exp(rng.uniform(math.log(0.06), math.log(8.0), n))
        return _cloud(rng, n, W, H, V, Ks, sigma, rng.uniform(1.0, 1.5, (n, 3)), 3)
    if name == "B":
        rng = np.random.default_rng(242)
        W, H, n = 40, 24, 120
        V, Ks = np.stack([_view(2.5, 0.1, 0.05), _view(2.8, -0.35, 0.2)]), _pinhole(W, H, 2)
        big = np.arange(n) % 3 == 0
        sigma = np.where(big, np.exp(rng.uniform(math.log(15.0), math.log(40.0), n)), np.exp(rng.uniform(math.log(0.12), math.log(0.6), n)))
        sc = _cloud(rng, n, W, H, V, Ks, sigma, rng.uniform(1.0, 1.4, (n, 3)), 2)
        sc["opacities"] = np.where(big, rng.uniform(0.02, 0.2, n), sc["opacities"]).astype(np.float32)   # (whole-frame splats: translucent)
        return sc
    assert name == "Z", name
    rng = np.random.default_rng(243)
    W, H, n = 64, 48, 48
    V, Ks = _view(3.0)[None], _pinhole(W, H, 1)
    sc = _cloud(rng, n, W, H, V, Ks, np.exp(rng.uniform(math.log(0.5), math.log(5.0), n)), rng.uniform(1.0, 1.5, (n, 3)), 1)
    for i in range(Z_DEGENERATE):
        sc["quats"][i] = _Z_QUATS[i % 4]
        sc["scales"][i] = (0.05 + 0.1 * i, 0.0, 0.0)
        sc["opacities"][i] = 0.9
    return sc


# ---- the composed reference ----

def forward(sc, colors=None, sh_degree="scene", backgrounds=None, mode="RGB", leaves=None, V=None, antialiased=True, **proj):
    """The composed fp64 forward (camera_model_ref.forward with this projection and op_eff)."""
    W, H = int(sc["width"]), int(sc["height"])
    ins = leaves if leaves is not None else [_f64(sc[k]) for k in GEO]
    V = _f64(sc["viewmats"]) if V is None else V
    Ks = _f64(sc["Ks"])
    C, N = V.shape[0], ins[0].shape[0]
    if sh_degree == "scene":
        sh_degree = sc["sh_degree"]
    colors = [_f64(sc["shs"])] if colors is None else colors
    radii, means2d, depths, conics, rho = project(ins[0], ins[1], ins[2], V, Ks, W, H, **proj)
    if mode in ("D", "ED"):
        cols, bg = depths[..., None], None
    else:
        if sh_degree is not None:
            cols = TO.spherical_harmonics(sh_degree, ins[0], V, torch.cat(colors, dim=1) if len(colors) == 2 else colors[0], radii)
        else:
            cols = colors[0].expand(C, N, -1) if colors[0].dim() == 2 else colors[0]
        bg = None if backgrounds is None else _f64(backgrounds)
        if mode != "RGB":
            cols = torch.cat([cols, depths[..., None]], dim=-1)
            bg = None if bg is None else torch.cat([bg, torch.zeros((C, 1), dtype=torch.float64)], dim=1)
    opac = ins[3][None, :].expand(C, N)
    if antialiased:
        opac = opac * rho
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    tpg, isect_ids, flatten_ids = TO.isect_tiles(means2d, radii, depths, 16, tw, th)
    offsets = TO.isect_offset_encode(isect_ids, C, tw, th)
    acc, alpha = TO.rasterize_to_pixels(means2d, conics, cols, opac, W, H, 16, offsets, flatten_ids, bg, True)
    img = torch.cat([acc[..., :-1], acc[..., -1:] / alpha.clamp(min=CM.ED_FLOOR)], dim=-1) if mode.endswith("ED") else acc
    return dict(img=img, alpha=alpha, acc=acc, radii=radii, means2d=means2d, depths=depths, conics=conics, opacities=opac, rho=rho,
                tiles_per_gauss=tpg, isect_ids=isect_ids, flatten_ids=flatten_ids, isect_offsets=offsets, colors=cols)


def razor(sc, **kw):
    """[C,H,W] pixels within 1e-4 of a blend discontinuity of the antialiased render (the margin is taken with op_eff)."""
    with torch.no_grad():
        fw = forward(sc, colors=[torch.zeros((sc["means"].shape[0], 3), dtype=torch.float64)], sh_degree=None, **kw)
    return CM.razor(sc, "pinhole", fw=fw)


upstream = CM.upstream


def reference(sc, colors, sh_degree, bg, vc, va, mode="RGB", cam=False, **kw):
    """Forward + autograd, as camera_model_ref.reference."""
    ins = [_f64(sc[k]).requires_grad_(True) for k in GEO]
    leaves = [_f64(c).requires_grad_(True) for c in colors]
    V = _f64(sc["viewmats"]).requires_grad_(cam)
    fw = forward(sc, leaves, sh_degree, bg, mode, leaves=ins, V=V, **kw)
    loss = (fw["img"] * vc).sum() + (fw["alpha"] * va).sum()
    gs = torch.autograd.grad(loss, ins + leaves + ([V] if cam else []), allow_unused=True)
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in fw.items()}
    out.update(grads=list(gs[:len(ins) + len(leaves)]), absgrad=fw["means2d"].absgrad)
    if cam:
        out["v_viewmats"] = gs[-1]
    return out


def gpu(sc, colors, sh_degree, bg, vc=None, va=None, mode="RGB", cam=False, grad=True, culling="gsplat", rasterize_mode="antialiased", **kw):
    """One forward (+ backward) of rasterization(rasterize_mode=...) on the GPU; rasterize_mode=None: the call without the keyword."""
    extra = {} if rasterize_mode is None else dict(rasterize_mode=rasterize_mode)
    return CM.gpu(sc, "pinhole", colors, sh_degree, bg, vc, va, mode=mode, cam=cam, grad=grad, culling=culling, keyword=False, **extra, **kw)
