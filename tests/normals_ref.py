"""References for the normal-consistency tests (tests/test_normals_host.py, tests/test_gpu_normals.py), none of them the code under
test:

  * `gauss64`: the normal of a Gaussian in float64 numpy, with the set of *razor* Gaussians -- those whose axis or facing a float32
    rounding may turn -- decided by the float64 run alone, and a per-element error bound;
  * `gauss_vjp64`: v_quats by torch float64 autograd of the same restatement, with a per-element error bound;
  * `loss64`: the loss of a frame, its gradients and their per-element error bounds in float64 numpy (the values are cross-checked
    against float64 autograd of `normals.normal_consistency_loss(fused=False)`, the semantic reference);
  * `host_lib`: tests/hostmath/normals.cpp -- csrc/gs_normals.h, the device's own text -- built with the host compiler;
  * the data of the cases both files share.

The error bounds are forward error analyses of csrc/gs_normals.h, written with U = 2^-24, the unit roundoff of float32: every fmaf,
product, sum, division and square root contributes one relative rounding U of its result, and an input error propagates through the
absolute values of the partial derivatives.  Second-order terms are covered by the factor SLACK = 1.05.  Where a count below is
rounded up it says so.  Nothing here was tuned on the output of the code under test."""
import ctypes as ct
import os
import subprocess

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
SLACK = 1.05
MIN_LEN2 = 1e-30


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _f64(a):
    return np.asarray(_f32(a), np.float64)


# ---- the host build ----

def host_lib(directory):
    so = os.path.join(str(directory), "libnormals_host.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "normals.cpp")], check=True)
    L = ct.CDLL(so)
    P, F, I, I64 = ct.c_void_p, ct.c_float, ct.c_int, ct.c_int64
    L.nm_axis.argtypes, L.nm_axis.restype = [F, F, F], I
    L.nm_gauss_fwd.argtypes, L.nm_gauss_fwd.restype = [I64, I, P, P, P, P, P], None
    L.nm_gauss_bwd.argtypes, L.nm_gauss_bwd.restype = [I64, I, P, P, P, P, P, P], None
    L.nm_loss_fwd.argtypes, L.nm_loss_fwd.restype = [I, I, P, F, P, P, P, P, P, P], None
    L.nm_loss_bwd.argtypes, L.nm_loss_bwd.restype = [I, I, P, F, I, P, P, P, F, F, P], None
    return L


def host_gauss_fwd(L, case):
    m, q, s, vm = (_f32(case[k]) for k in ("means", "quats", "scales", "viewmats"))
    N, C = len(m), len(vm)
    out = np.full((C, N, 3), -7.0, np.float32)
    L.nm_gauss_fwd(N, C, m.ctypes.data, q.ctypes.data, s.ctypes.data, vm.ctypes.data, out.ctypes.data)
    return out


def host_gauss_bwd(L, case, v_normals):
    m, q, s, vm, v = (_f32(a) for a in (case["means"], case["quats"], case["scales"], case["viewmats"], v_normals))
    N, C = len(m), len(vm)
    out = np.full((N, 4), -7.0, np.float32)
    L.nm_gauss_bwd(N, C, m.ctypes.data, q.ctypes.data, s.ctypes.data, vm.ctypes.data, v.ctypes.data, out.ctypes.data)
    return out


def host_loss(L, frame, *, detach_depth=False, v_loss=1.0, with_mask=True):
    """-> dict(value f32, inv_w f32, sums f64[2], depth_normals f32 [H,W,3], v_render4 f32 [H,W,4]) of the host build"""
    r, a, K = _f32(frame["render4"]), _f32(frame["alphas"]), _f32(frame["K"])
    mask = _f32(frame["mask"]) if (with_mask and frame.get("mask") is not None) else None
    H, W, _ = r.shape
    rec, sums = np.full(2, -7.0, np.float32), np.zeros(2, np.float64)
    dn, vr = np.full((H, W, 3), -7.0, np.float32), np.full((H, W, 4), -7.0, np.float32)
    mp = None if mask is None else mask.ctypes.data
    L.nm_loss_fwd(H, W, K.ctypes.data, frame["min_alpha"], r.ctypes.data, a.ctypes.data, mp, rec.ctypes.data, sums.ctypes.data, dn.ctypes.data)
    L.nm_loss_bwd(H, W, K.ctypes.data, frame["min_alpha"], int(detach_depth), r.ctypes.data, a.ctypes.data, mp, float(rec[1]), v_loss,
                  vr.ctypes.data)
    return dict(value=rec[0], inv_w=rec[1], sums=sums, depth_normals=dn, v_render4=vr)


# ---- the normal of a Gaussian in float64 ----

def _column(qh, k):
    """column k (an int array) of R(qh) for unit quaternions qh [..., 4] (wxyz): R e_k = e_k (1 - 2 |v|^2) + 2 v v_k + 2 w (v x e_k)"""
    lib = torch if isinstance(qh, torch.Tensor) else np
    w, v = qh[..., :1], qh[..., 1:]
    if lib is torch:
        e = torch.nn.functional.one_hot(torch.as_tensor(k), 3).to(qh.dtype)
        vk = (v * e).sum(-1, keepdim=True)
        return e * (1 - 2 * (v * v).sum(-1, keepdim=True)) + 2 * v * vk + 2 * w * torch.cross(v, e, dim=-1)
    e = np.eye(3)[k]
    vk = (v * e).sum(-1, keepdims=True)
    return e * (1 - 2 * (v * v).sum(-1, keepdims=True)) + 2 * v * vk + 2 * w * np.cross(v, e)


def axis64(scales):
    """(k, razor): the index of the smallest scale (lowest index on a tie) and whether the two smallest lie within a relative 1e-6"""
    s = _f64(scales)
    k = np.argmin(s, axis=1)
    two = np.sort(s, axis=1)[:, :2]
    razor = np.abs(two[:, 1] - two[:, 0]) <= 1e-6 * np.maximum(np.abs(two[:, 0]), np.abs(two[:, 1]))
    return k, razor


def gauss64(case):
    """-> dict(normals [C,N,3], razor [C,N], bound [C,N,3], flipped [C,N], k [N]).
    Bound: q_hat carries <= 4 U per component (four fmaf-roundings under a square root, the root, the division: 2 + 0.5 + 1 rounded
    up); an entry of the column has partials of absolute sum <= 4 sqrt(2) < 5.7 in q_hat and three local roundings of values <= 2,
    so <= (5.7 * 4 + 4) U < 27 U; the camera rotation multiplies that by its row's absolute sum and adds three roundings of its
    terms.  Razor: the axis (axis64), or |dot(n, p)| within 64 U of the sum of its terms' magnitudes plus the bound's share."""
    m, q, vm = _f64(case["means"]), _f64(case["quats"]), _f64(case["viewmats"])
    k, razor_k = axis64(case["scales"])
    qh = q / np.linalg.norm(q, axis=1, keepdims=True)
    nw = _column(qh, k)
    R, t = vm[:, :3, :3], vm[:, :3, 3]
    nc = np.einsum("cij,nj->cni", R, nw)
    pc = np.einsum("cij,nj->cni", R, m) + t[:, None, :]
    dot = (nc * pc).sum(-1)
    Rabs = np.abs(R)
    bound = SLACK * (27 * U * Rabs.sum(-1)[:, None, :] + 3 * U * np.einsum("cij,nj->cni", Rabs, np.abs(nw)))
    mag = (np.abs(nc) * np.abs(pc)).sum(-1)
    pabs = np.einsum("cij,nj->cni", Rabs, np.abs(m)) + np.abs(t)[:, None, :]
    razor = razor_k[None, :] | (np.abs(dot) <= 64 * U * mag + (bound * np.abs(pc)).sum(-1) + 8 * U * (np.abs(nc) * pabs).sum(-1))
    flipped = dot > 0
    return dict(normals=np.where(flipped[..., None], -nc, nc), razor=razor, bound=bound, flipped=flipped, k=k)


def gauss_vjp64(case, v_normals):
    """-> (v_quats [N,4] by torch float64 autograd with the axis and the facing of the float64 forward held constant, bound [N,4]).
    Bound, per Gaussian (J = the 3 x 4 Jacobian of the column, |J| its absolute values, g = sum_c s_c R_c^T v_c):
      e_g  = (C + 3) U * sum_c |R_c|^T |v_c|                       three roundings per term, one per accumulation
      e_vh = |J|^T e_g + 16 U |g|_1 + 4 U |J|^T |g|                 q_hat's 4 U through coefficients <= 4; four local roundings
      e_d  = |q_hat| . e_vh + 4 U |vh|_1 + 4 U |q_hat| . |vh|       d = q_hat . vh
      e_out_j = (e_vh_j + |q_hat_j| e_d + 4 U |d| + 2 U (|vh_j| + |q_hat_j d|)) / |q| + 3 U |out_j|"""
    fw = gauss64(case)
    q = torch.tensor(_f64(case["quats"]), requires_grad=True)
    vm = torch.tensor(_f64(case["viewmats"]))
    sign = torch.tensor(np.where(fw["flipped"], -1.0, 1.0))
    v = torch.tensor(_f64(v_normals))
    qh = q / q.norm(dim=1, keepdim=True)
    nw = _column(qh, fw["k"])
    nc = torch.einsum("cij,nj->cni", vm[:, :3, :3], nw) * sign[..., None]
    (vq,) = torch.autograd.grad((nc * v).sum(), q)
    # the bound
    qh_, nq = qh.detach().numpy(), q.detach().norm(dim=1).numpy()
    J = torch.autograd.functional.jacobian(lambda x: _column(x, fw["k"]).sum(0), torch.tensor(qh_)).numpy()   # [3, N, 4]
    Jabs = np.abs(J).transpose(1, 0, 2)   # [N, 3, 4]
    R = _f64(case["viewmats"])[:, :3, :3]
    sv = sign.numpy()[..., None] * v.numpy()
    g = np.einsum("cji,cnj->ni", R, sv)
    gabs = np.einsum("cji,cnj->ni", np.abs(R), np.abs(sv))
    C = len(R)
    e_g = (C + 3) * U * gabs
    vh = np.einsum("nkj,nk->nj", J.transpose(1, 0, 2), g)
    e_vh = np.einsum("nkj,nk->nj", Jabs, e_g) + 16 * U * np.abs(g).sum(1, keepdims=True) + 4 * U * np.einsum("nkj,nk->nj", Jabs, np.abs(g))
    d = (qh_ * vh).sum(1, keepdims=True)
    e_d = (np.abs(qh_) * e_vh).sum(1, keepdims=True) + 4 * U * np.abs(vh).sum(1, keepdims=True) + 4 * U * (np.abs(qh_) * np.abs(vh)).sum(1, keepdims=True)
    out = (vh - qh_ * d) / nq[:, None]
    bound = SLACK * ((e_vh + np.abs(qh_) * e_d + 4 * U * np.abs(d) + 2 * U * (np.abs(vh) + np.abs(qh_ * d))) / nq[:, None] + 3 * U * np.abs(out))
    assert np.allclose(out, vq.numpy(), rtol=1e-9, atol=1e-12 * np.abs(out).max())   # (the explicit chain is the autograd result)
    return vq.numpy(), bound


def gauss_case(N, C, seed):
    """Means around the origin, cameras 3 units away looking at it: Gaussians face towards and away from every camera.  Quaternion
    magnitudes log-uniform in [0.1, 10]; log-scales normal (continuous: axis razors have measure zero)."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1, 1, (N, 3))
    quats = rng.normal(size=(N, 4))
    quats *= (10.0 ** rng.uniform(-1, 1, (N, 1))) / np.linalg.norm(quats, axis=1, keepdims=True)
    scales = rng.normal(-3.0, 1.0, (N, 3))
    vms = []
    for c in range(C):
        a = rng.normal(size=(3, 3))
        Q, _ = np.linalg.qr(a)
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        vm = np.eye(4)
        vm[:3, :3] = Q
        vm[:3, 3] = (0.1 * c, -0.05, 3.0)
        vms.append(vm)
    return dict(means=_f32(means), quats=_f32(quats), scales=_f32(scales), viewmats=_f32(np.stack(vms)))


# ---- the loss of a frame in float64, with its error bounds ----

def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _cross_err(a, ea, b, eb):
    """the error of the computed cross product: inputs' errors through |.|, and an fmaf of a rounded product (2 U of the terms)"""
    a, b = np.abs(a), np.abs(b)

    def comp(i, j):
        return a[i] * eb[j] + ea[i] * b[j] + a[j] * eb[i] + ea[j] * b[i] + 2 * U * (a[i] * b[j] + a[j] * b[i])
    return np.stack([comp(1, 2), comp(2, 0), comp(0, 1)])


def loss64(frame, *, detach_depth=False, v_loss=1.0, with_mask=True):
    """-> dict(value, value_bound, valid [H,W] (the mask aside), w [H,W], depth_normals [H,W,3], dn_bound [H,W,3], v_render4 [H,W,4],
    v_bound [H,W,4], min_len [the smallest |c| of a valid pixel]).

    Bounds (components k; everything at one centre; U per rounding):
      ray u = ((x + 0.5) - c) / f: 2 U |u|.   P = d u: 3 U |P|.   A = P1 - P2: e_A = 3 U (|P1| + |P2|) + U |A|, B alike.
      c = A x B: _cross_err.   len = |c|: |dlen| <= |e_c|_2 + 2 U len (three fmaf-roundings of a sum of squares halve under the root,
      plus the root: rounded up to 2 U).   n = c / len: e_n = e_c / len + |n| (|e_c|_2 / len + 3 U).
      e = 1 - Nb . n: e_e = |Nb| . e_n + 3 U |Nb| . |n| + U |e|;  value: sum(w e_e) / sum(w) + 2 U |value| (the fp64 sums and the one
      rounding to fp32).
      g = -(upstream * (1 / sum w)) w: relative 4 U (1 / sum(w) to fp32, two products, w = 1 - m).
      v_Nb = g n: |g| (e_n + 5 U |n|).
      v_n = g Nb: 5 U |v_n|.   dd = n . v_n: e_dd = e_n . |v_n| + 8 U |n| . |v_n|.
      v_c = (v_n - n dd) / len: e_vc = (5 U |v_n| + e_n |dd| + |n| e_dd + 2 U (|v_n| + |n dd|)) / len + |v_c| (|e_c|_2 / len + 3 U)
                                -- the conditioning: the projection cancels, and everything is divided by |c|.
      v_A = B x v_c, v_B = v_c x A: _cross_err.   send = v0 u + v1 v + v2: e_v0 |u| + e_v1 |v| + e_v2 + 5 U (|v0 u| + |v1 v| + |v2|)
      (the rays' 2 U, two fmaf-roundings, rounded up).   v_d = the sum of four: sum(e_send) + 3 U sum |send|."""
    r, al, K = _f64(frame["render4"]), _f64(frame["alphas"]), _f64(frame["K"])
    H, W, _ = r.shape
    min_alpha = float(np.float32(frame["min_alpha"]))
    mask = _f64(frame["mask"]) if (with_mask and frame.get("mask") is not None) else np.zeros((H, W))
    out = dict(value=0.0, value_bound=0.0, valid=np.zeros((H, W), bool), w=np.zeros((H, W)), depth_normals=np.zeros((H, W, 3)),
               dn_bound=np.zeros((H, W, 3)), v_render4=np.zeros((H, W, 4)), v_bound=np.zeros((H, W, 4)), min_len=np.inf)
    if H < 3 or W < 3:
        return out
    d = r[..., 3]
    with np.errstate(invalid="ignore"):
        ok = (al >= min_alpha) & np.isfinite(d) & (d > 0)
    ds = np.where(ok, d, 1.0)
    u = ((np.arange(W) + 0.5) - K[0, 2]) / K[0, 0]
    v = ((np.arange(H) + 0.5) - K[1, 2]) / K[1, 1]
    I = (slice(1, H - 1), slice(1, W - 1))

    def sh(a, dy, dx):
        return a[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
    one = np.ones((H - 2, W - 2))
    ux, ul, ur = u[None, 1:-1] * one, u[None, :-2] * one, u[None, 2:] * one
    vy, vu, vd = v[1:-1, None] * one, v[:-2, None] * one, v[2:, None] * one
    dl, dr, du, dd_ = sh(ds, 0, -1), sh(ds, 0, 1), sh(ds, -1, 0), sh(ds, 1, 0)
    Pd, Pu = np.stack([dd_ * ux, dd_ * vd, dd_]), np.stack([du * ux, du * vu, du])
    Pr, Pl = np.stack([dr * ur, dr * vy, dr]), np.stack([dl * ul, dl * vy, dl])
    A, B = Pd - Pu, Pr - Pl
    eA = 3 * U * (np.abs(Pd) + np.abs(Pu)) + U * np.abs(A)
    eB = 3 * U * (np.abs(Pr) + np.abs(Pl)) + U * np.abs(B)
    c = _cross(A, B)
    ec = _cross_err(A, eA, B, eB)
    len2 = (c * c).sum(0)
    valid = sh(ok, 0, 0) & sh(ok, 0, -1) & sh(ok, 0, 1) & sh(ok, -1, 0) & sh(ok, 1, 0) & np.isfinite(len2) & (len2 >= MIN_LEN2)
    ln = np.sqrt(np.where(valid, len2, 1.0))
    n = c / ln
    ec2 = np.sqrt((ec * ec).sum(0))
    e_n = ec / ln + np.abs(n) * (ec2 / ln + 3 * U)
    w = valid * (1 - sh(mask, 0, 0))
    Nb = np.moveaxis(sh(r[..., :3], 0, 0), -1, 0)
    e = 1 - (Nb * n).sum(0)
    e_e = (np.abs(Nb) * e_n).sum(0) + 3 * U * (np.abs(Nb) * np.abs(n)).sum(0) + U * np.abs(e)
    den = w.sum()
    out["valid"][I], out["w"][I] = valid, w
    out["depth_normals"][I] = np.where(valid[..., None], np.moveaxis(n, 0, -1), 0.0)
    out["dn_bound"][I] = SLACK * np.where(valid[..., None], np.moveaxis(e_n, 0, -1), 0.0)
    if valid.any():
        out["min_len"] = float(ln[valid].min())
    if not den > 0:
        return out
    out["value"] = float((w * np.where(valid, e, 0.0)).sum() / den)
    out["value_bound"] = SLACK * (float((np.abs(w) * np.where(valid, e_e, 0.0)).sum() / den) + 2 * U * abs(out["value"]))
    g = np.where(valid, -(v_loss / den) * w, 0.0)
    v_nb = g * n
    out["v_render4"][I + (slice(0, 3),)] = np.moveaxis(v_nb, 0, -1)
    out["v_bound"][I + (slice(0, 3),)] = SLACK * np.moveaxis(np.abs(g) * (e_n + 5 * U * np.abs(n)), 0, -1)
    if detach_depth:
        return out
    vn = g * Nb
    dd = (n * vn).sum(0)
    e_dd = (e_n * np.abs(vn)).sum(0) + 8 * U * (np.abs(n) * np.abs(vn)).sum(0)
    vc = (vn - n * dd) / ln
    e_vc = (5 * U * np.abs(vn) + e_n * np.abs(dd) + np.abs(n) * e_dd + 2 * U * (np.abs(vn) + np.abs(n * dd))) / ln + np.abs(vc) * (ec2 / ln + 3 * U)
    vA, e_vA = _cross(B, vc), _cross_err(B, eB, vc, e_vc)
    vB, e_vB = _cross(vc, A), _cross_err(vc, e_vc, A, eA)

    def send(vv, ev, uu, vv_ray, sign):
        val = sign * (vv[0] * uu + vv[1] * vv_ray + vv[2])
        err = ev[0] * np.abs(uu) + ev[1] * np.abs(vv_ray) + ev[2] + 5 * U * (np.abs(vv[0] * uu) + np.abs(vv[1] * vv_ray) + np.abs(vv[2]))
        return np.where(valid, val, 0.0), np.where(valid, err, 0.0)
    s_up, e_up = send(vA, e_vA, ux, vu, -1.0)
    s_dn, e_dn = send(vA, e_vA, ux, vd, 1.0)
    s_l, e_l = send(vB, e_vB, ul, vy, -1.0)
    s_r, e_r = send(vB, e_vB, ur, vy, 1.0)
    vdep, edep, mag = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for s_, e_, dy, dx in ((s_up, e_up, -1, 0), (s_dn, e_dn, 1, 0), (s_l, e_l, 0, -1), (s_r, e_r, 0, 1)):
        tgt = (slice(1 + dy, H - 1 + dy), slice(1 + dx, W - 1 + dx))
        vdep[tgt] += s_
        edep[tgt] += e_
        mag[tgt] += np.abs(s_)
    out["v_render4"][..., 3] = vdep
    out["v_bound"][..., 3] = SLACK * (edep + 3 * U * mag)
    return out


def loss_autograd64(frame, *, detach_depth=False, v_loss=1.0, with_mask=True):
    """(value, v_render4 [H,W,4]) by float64 autograd of normals.normal_consistency_loss(fused=False)"""
    from easy_gaussian_splatting_amd import normals as NM
    r = torch.tensor(_f64(frame["render4"]), requires_grad=True)
    mask = torch.tensor(_f64(frame["mask"])) if (with_mask and frame.get("mask") is not None) else None
    value = NM.normal_consistency_loss(r, torch.tensor(_f64(frame["alphas"])), torch.tensor(_f64(frame["K"])), mask=mask,
                                       min_alpha=float(np.float32(frame["min_alpha"])), detach_depth=detach_depth, fused=False)
    (g,) = torch.autograd.grad(value * v_loss, r, allow_unused=True)
    return float(value.detach()), (np.zeros(r.shape) if g is None else g.numpy())


# ---- frames ----

TILE_W, TILE_H = 64, 8   # include/gs_raster.h: GS_NORMAL_TILE_W, GS_NORMAL_TILE_H (tests/test_gpu_normals.py asserts they agree)


def camera(H, W):
    f = 0.9 * max(W, 8)
    return _f32([[f, 0, 0.5 * W + 0.3], [0, 1.1 * f, 0.5 * H - 0.2], [0, 0, 1]])


def frame_case(H, W, seed, *, holes=True, mask=True, bad_depths=True, min_alpha=0.5):
    """A smooth, tilted, wavy surface 2 units away with 1 % noise; blended normals of length about alpha around the surface's;
    alpha holes (5 % of the pixels below min_alpha), a few depths 0 / negative / NaN / inf, a binary mask over 10 %."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 2.0 + 0.02 * x - 0.015 * y + 0.2 * np.sin(x / 5.0) * np.cos(y / 7.0) + 0.01 * rng.normal(size=(H, W))
    alphas = rng.uniform(0.7, 1.0, (H, W))
    if holes:
        alphas[rng.uniform(size=(H, W)) < 0.05] = 0.2
    if bad_depths and H * W >= 9:
        for val in (0.0, -1.0, np.nan, np.inf):
            d[rng.integers(0, H), rng.integers(0, W)] = val
    nb = np.stack([0.3 * rng.normal(size=(H, W)), 0.3 * rng.normal(size=(H, W)), -1.0 + 0.2 * rng.normal(size=(H, W))], -1)
    nb *= (alphas / np.linalg.norm(nb, axis=-1))[..., None]
    m = (rng.uniform(size=(H, W)) < 0.1).astype(np.float32) if mask else None
    return dict(render4=_f32(np.concatenate([nb, d[..., None]], -1)), alphas=_f32(alphas), K=camera(H, W), mask=m, min_alpha=min_alpha)


def border_case(H, W, seed):
    """Alpha is 1 only on centres that sit on tile corners and tile borders and on their four neighbours; 0 elsewhere: every valid
    pixel has a neighbour in another tile."""
    f = frame_case(H, W, seed, holes=False, mask=False, bad_depths=False)
    y, x = np.mgrid[0:H, 0:W]
    xb, yb = np.isin(x % TILE_W, (0, TILE_W - 1)), np.isin(y % TILE_H, (0, TILE_H - 1))
    centres = (xb & yb) | (xb & (y % TILE_H == 3)) | (yb & (x % TILE_W == 20))
    keep = centres.copy()
    keep[1:] |= centres[:-1]; keep[:-1] |= centres[1:]; keep[:, 1:] |= centres[:, :-1]; keep[:, :-1] |= centres[:, 1:]
    f["alphas"] = _f32(np.where(keep, 1.0, 0.0))
    f["centres"] = centres
    return f


def plane_frame(H, W, normal, offset, K):
    """The exact depth map of the plane {p: normal . p = offset} (|normal| = 1, facing the camera: normal_z < 0) in float64."""
    K = _f64(K)
    u = ((np.arange(W) + 0.5) - K[0, 2]) / K[0, 0]
    v = ((np.arange(H) + 0.5) - K[1, 2]) / K[1, 1]
    ray = np.stack([u[None, :] * np.ones((H, 1)), v[:, None] * np.ones((1, W)), np.ones((H, W))], -1)
    return offset / (ray @ np.asarray(normal, np.float64))


def sphere_frame(H, W, centre, radius, K):
    """(depth [H,W] float64 with 0 where the ray misses, the outward unit normal at the hit [H,W,3])"""
    K = _f64(K)
    u = ((np.arange(W) + 0.5) - K[0, 2]) / K[0, 0]
    v = ((np.arange(H) + 0.5) - K[1, 2]) / K[1, 1]
    ray = np.stack([u[None, :] * np.ones((H, 1)), v[:, None] * np.ones((1, W)), np.ones((H, W))], -1)
    c = np.asarray(centre, np.float64)
    a, b, cc = (ray * ray).sum(-1), (ray @ c), c @ c - radius * radius
    disc = b * b - a * cc
    hit = disc > 0
    t = np.where(hit, (b - np.sqrt(np.where(hit, disc, 0.0))) / a, 0.0)
    p = ray * t[..., None]
    return t, np.where(hit[..., None], (p - c) / radius, 0.0)
