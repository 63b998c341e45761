"""fp64 reference of `rasterization(camera_model="ortho" | "fisheye")`: a torch projection with the camera model as an argument, laid
out like `oracle.torch_oracle.project`, composed with the oracle's own `spherical_harmonics`, `isect_tiles`, `isect_offset_encode`
and `rasterize_to_pixels`; every gradient by autograd.  Shared by tests/test_camera_model_host.py and tests/test_gpu_camera_models.py;
also the scenes of those tests and the GPU runner.

The definitions are the project's own (DESIGN.md "Camera models"): the mean goes to camera space as for the pinhole, the near/far cull
on z is unchanged, cov2 = J cov_c J^T + eps2d I with the model's J, and everything behind cov2 is `project`'s.
  ortho:   means2d = (fx x + cx, fy y + cy),     J = [[fx, 0, 0], [0, fy, 0]]
  fisheye: means2d = (fx x k + cx, fy y k + cy), J = [[fx (k + x^2 g), fx x y g, -fx x / d^2], [fy x y g, fy (k + y^2 g), -fy y / d^2]]
           with r^2 = x^2 + y^2, d^2 = r^2 + z^2, theta = atan2(r, z), k = theta / r, g = (z / d^2 - k) / r^2
On the optical axis k -> 1 / z and g -> -2 / (3 z^3): theta / r at r = 0 is 0 / 0, a NaN that would make means2d NaN and cull exactly
the Gaussians on the axis without a word.  Both limits are therefore taken through the double-`where` pattern (the dead branch is
evaluated at a safe r, so that neither the value nor autograd's gradient of it is NaN)."""
import math

import numpy as np
import torch

from oracle import c_oracle as CO
from oracle import torch_oracle as TO
from scenes import make_scene

GEO = ("means", "quats", "scales", "opacities")
MODELS = ("pinhole", "ortho", "fisheye")
ED_FLOOR = 1e-10


def fisheye_kg(x, y, z):
    """k = theta / r and g = (z / d^2 - k) / r^2 with their on-axis limits (r = 0: k = 1 / z, g = -2 / (3 z^3))."""
    r2 = x * x + y * y
    on_axis = r2 == 0
    r2s = torch.where(on_axis, torch.ones_like(r2), r2)
    r = torch.sqrt(r2s)
    k = torch.where(on_axis, 1.0 / z, torch.atan2(r, z) / r)
    g = torch.where(on_axis, -2.0 / (3.0 * z * z * z), (z / (r2s + z * z) - k) / r2s)
    return k, g


def mean_map(model, x, y, z, fx, fy, cx, cy):
    """Camera space -> pixel."""
    if model == "ortho":
        return fx * x + cx, fy * y + cy
    if model == "fisheye":
        k, _ = fisheye_kg(x, y, z)
        return fx * x * k + cx, fy * y * k + cy
    return fx * x / z + cx, fy * y / z + cy


def jacobian(model, x, y, z, fx, fy):
    """The closed-form 2x3 Jacobian of `mean_map` [..., 2, 3] (ortho, fisheye)."""
    O = torch.zeros_like(z)
    if model == "ortho":
        rows = [fx + O, O, O, O, fy + O, O]
    else:
        assert model == "fisheye", model
        k, g = fisheye_kg(x, y, z)
        d2 = x * x + y * y + z * z
        rows = [fx * (k + x * x * g), fx * x * y * g, -fx * x / d2, fy * x * y * g, fy * (k + y * y * g), -fy * y / d2]
    return torch.stack(rows, dim=-1).reshape(z.shape + (2, 3))


def project(model, means, quats, scales, viewmats, Ks, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0):
    """`TO.project` under the camera model: radii[C,N] int32, means2d[C,N,2], depths[C,N], conics[C,N,3]; culled entries are exactly
    zero.  "pinhole" is `TO.project` itself."""
    if model == "pinhole":
        return TO.project(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip)
    eps2d, near_plane, far_plane, radius_clip = (float(np.float32(v)) for v in (eps2d, near_plane, far_plane, radius_clip))
    Rq = TO.quat_to_rotmat(quats)
    M = Rq * scales[:, None, :]
    covars = M @ M.transpose(-1, -2)
    Rv, tv = viewmats[:, :3, :3], viewmats[:, :3, 3]
    p_c = torch.einsum("cij,nj->cni", Rv, means) + tv[:, None, :]
    cov_c = torch.einsum("cij,njk,clk->cnil", Rv, covars, Rv)
    z = p_c[..., 2]
    depth_ok = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(depth_ok, z, torch.ones_like(z))            # keeps the dead branch finite
    x, y = p_c[..., 0], p_c[..., 1]
    fx, fy = Ks[:, 0, 0][:, None], Ks[:, 1, 1][:, None]
    cx, cy = Ks[:, 0, 2][:, None], Ks[:, 1, 2][:, None]
    J = jacobian(model, x, y, zs, fx, fy)
    cov2 = J @ cov_c @ J.transpose(-1, -2)
    means2d = torch.stack(mean_map(model, x, y, zs, fx, fy, cx, cy), dim=-1)
    a = cov2[..., 0, 0] + eps2d
    b = 0.5 * (cov2[..., 0, 1] + cov2[..., 1, 0])
    c = cov2[..., 1, 1] + eps2d
    det = a * c - b * b
    det_ok = det > 0
    dets = torch.where(det_ok, det, torch.ones_like(det))
    conics = torch.stack([c / dets, -b / dets, a / dets], dim=-1)
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
    return radii, means2d, depths, conics


# ---- scenes ----

def intrinsics(model, W, H, C, param):
    """Ks [C,3,3]: fisheye f = (W/2) / radians(half_fov), ortho f = (W/2) / half_width; principal point at the centre."""
    f = (W / 2) / (math.radians(param) if model == "fisheye" else param)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    return np.broadcast_to(K, (C, 3, 3)).copy()


_SCENES = {
    "1": (dict(n=1500, W=100, H=80, sh_degree=3, n_views=2, seed=71, scale_range=(0.02, 0.2), dist=2.5), {"fisheye": 75.0, "ortho": 2.2}),
    "2": (dict(n=777, W=67, H=45, sh_degree=2, n_views=2, seed=72, scale_range=(0.02, 0.3), dist=1.0), {"fisheye": 85.0, "ortho": 1.5}),
    "3": (dict(n=300, W=100, H=80, sh_degree=1, n_views=1, seed=73, scale_range=(0.3, 1.5), dist=4.0), {"fisheye": 60.0, "ortho": 3.0}),
}
# visible (camera, Gaussian) pairs measured on the CPU when the scenes were chosen: a test asks for at least half of them
VISIBLE = {"F1": 2990, "O1": 2984, "F2": 1158, "O2": 848, "F3": 300, "O3": 300, "X": 64}
X_RHOS = (0.0, 1e-7, 1e-5, 1e-3, 1e-2, 0.1, 0.5, 1.0)


def scene(name):
    """(scene dict, model).  F1/O1, F2/O2 (ragged tiles, camera inside the cloud), F3/O3 (footprints up to the whole frame), and X:
    64 Gaussians at rho = r / z in X_RHOS, eight per value, the rho = 0 group exactly on the optical axis at eight depths."""
    if name == "X":
        rng = np.random.default_rng(74)
        W, H, z0 = 100, 80, 2.0
        means = np.zeros((64, 3), np.float32)
        for i, rho in enumerate(X_RHOS):
            for j in range(8):
                phi = 2 * math.pi * (j + 0.3) / 8
                if rho == 0.0:
                    means[8 * i + j] = (0.0, 0.0, 0.25 * j)          # camera-space depths 2.0 .. 3.75
                else:
                    means[8 * i + j] = (rho * z0 * math.cos(phi), rho * z0 * math.sin(phi), 0.0)
        V = np.eye(4, dtype=np.float32)[None].copy()
        V[0, 2, 3] = z0
        quats = rng.standard_normal((64, 4)).astype(np.float32)
        sc = dict(means=means, quats=quats, scales=rng.uniform(0.05, 0.4, (64, 3)).astype(np.float32),
                  opacities=rng.uniform(0.05, 0.3, 64).astype(np.float32), shs=(0.5 * rng.standard_normal((64, 4, 3))).astype(np.float32),
                  viewmats=V, Ks=intrinsics("fisheye", W, H, 1, 70.0), backgrounds=rng.random((1, 3)).astype(np.float32), width=W, height=H,
                  sh_degree=1)
        return sc, "fisheye"
    model = {"F": "fisheye", "O": "ortho"}[name[0]]
    kw, params = _SCENES[name[1]]
    kw = dict(kw)
    sc = make_scene(kw.pop("n"), kw.pop("W"), kw.pop("H"), **kw)
    sc = dict(sc, Ks=intrinsics(model, int(sc["width"]), int(sc["height"]), sc["viewmats"].shape[0], params[model]), sh_degree=kw["sh_degree"])
    return sc, model


# ---- the composed reference ----

def _f64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def forward(sc, model, colors=None, sh_degree="scene", backgrounds=None, mode="RGB", leaves=None, V=None, **proj):
    """The composed fp64 forward.  Returns dict(img, alpha, acc, meta...) with graph tensors when `leaves` (geometry leaves) carry grad."""
    W, H = int(sc["width"]), int(sc["height"])
    ins = leaves if leaves is not None else [_f64(sc[k]) for k in GEO]
    V = _f64(sc["viewmats"]) if V is None else V
    Ks = _f64(sc["Ks"])
    C, N = V.shape[0], ins[0].shape[0]
    if sh_degree == "scene":
        sh_degree = sc["sh_degree"]
    colors = [_f64(sc["shs"])] if colors is None else colors
    radii, means2d, depths, conics = project(model, ins[0], ins[1], ins[2], V, Ks, W, H, **proj)
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
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    tpg, isect_ids, flatten_ids = TO.isect_tiles(means2d, radii, depths, 16, tw, th)
    offsets = TO.isect_offset_encode(isect_ids, C, tw, th)
    acc, alpha = TO.rasterize_to_pixels(means2d, conics, cols, opac, W, H, 16, offsets, flatten_ids, bg, True)
    img = torch.cat([acc[..., :-1], acc[..., -1:] / alpha.clamp(min=ED_FLOOR)], dim=-1) if mode.endswith("ED") else acc
    return dict(img=img, alpha=alpha, acc=acc, radii=radii, means2d=means2d, depths=depths, conics=conics, opacities=opac,
                tiles_per_gauss=tpg, isect_ids=isect_ids, flatten_ids=flatten_ids, isect_offsets=offsets, colors=cols)


def razor(sc, model, fw=None, **proj):
    """[C,H,W] pixels within 1e-4 of a blend discontinuity: `c_oracle.blend_margin` on a dict built from this projection."""
    with torch.no_grad():
        fw = forward(sc, model, colors=[torch.zeros((sc["means"].shape[0], 3), dtype=torch.float64)], sh_degree=None, **proj) if fw is None else fw
    c = lambda t, dt=np.float64: np.ascontiguousarray(t.detach().numpy().astype(dt))
    d = dict(radii=c(fw["radii"], np.int32), means2d=c(fw["means2d"]), conics=c(fw["conics"]), opacities=c(fw["opacities"]),
             isect_offsets=c(fw["isect_offsets"], np.int32), flatten_ids=c(fw["flatten_ids"], np.int32), n_isects=int(fw["flatten_ids"].shape[0]),
             _inputs=dict(width=int(sc["width"]), height=int(sc["height"]), tile_size=16))
    return CO.blend_margin(d, mu_tol_ulps=1.0, conic_rtol=2.4e-7) < 1e-4


def upstream(rz, D, seed):
    """Random upstream gradients of the image [C,H,W,D] and the alphas, zero on the razor pixels."""
    g = torch.Generator().manual_seed(seed)
    C, H, W = rz.shape
    keep = torch.from_numpy(~rz).double()[..., None]
    return torch.randn((C, H, W, D), generator=g, dtype=torch.float64) * keep, torch.randn((C, H, W, 1), generator=g, dtype=torch.float64) * keep


def reference(sc, model, colors, sh_degree, bg, vc, va, mode="RGB", cam=False, **proj):
    """Forward + autograd.  colors: a list of arrays -- [shs] / [sh_0, sh_rest] with sh_degree, [features] without.  Returns
    dict(img, alpha, acc, grads (geometry + colour leaves, in order), absgrad, v_viewmats (cam=True), and the forward's arrays)."""
    ins = [_f64(sc[k]).requires_grad_(True) for k in GEO]
    leaves = [_f64(c).requires_grad_(True) for c in colors]
    V = _f64(sc["viewmats"]).requires_grad_(cam)
    fw = forward(sc, model, leaves, sh_degree, bg, mode, leaves=ins, V=V, **proj)
    loss = (fw["img"] * vc).sum() + (fw["alpha"] * va).sum()
    wrt = ins + leaves + ([V] if cam else [])
    gs = torch.autograd.grad(loss, wrt, allow_unused=True)
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in fw.items()}
    out.update(grads=list(gs[:len(ins) + len(leaves)]), absgrad=fw["means2d"].absgrad)
    if cam:
        out["v_viewmats"] = gs[-1]
    return out


def gpu(sc, model, colors, sh_degree, bg, vc=None, va=None, mode="RGB", cam=False, grad=True, culling="gsplat", keyword=True, **kw):
    """One forward (+ backward) of rasterization(camera_model=model) on the GPU; the same arguments as `reference`.  keyword=False:
    the call without the keyword at all."""
    from easy_gaussian_splatting_amd.rendering import rasterization
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    d = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(d)
    ins = [to(sc[k]).requires_grad_(grad) for k in GEO]
    leaves = [to(c).requires_grad_(grad) for c in colors]
    V = to(sc["viewmats"]).requires_grad_(cam)
    extra = dict(_camera_grads=True) if cam else {}
    if keyword:
        extra["camera_model"] = model
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
