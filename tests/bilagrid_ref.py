"""fp64 reference of the bilateral-grid kernels (csrc/gs_bilagrid.h) and the bounds a correct fp32 kernel keeps -- shared by
tests/test_bilagrid_host.py (the header built with the host compiler) and tests/test_gpu_bilagrid.py (the device).  The reference
is torch's `grid_sample(mode="bilinear", align_corners=True, padding_mode="border")` in fp64 on the CPU with its autograd
gradients; nothing here imports the package.

A slab is G[12][L][Hg][Wg], channel k = 4 i + j entry (i, j) of [A | b]; G_k = max |G[k]| over the slab.  eps32 = 2^-24.

The bounds (DESIGN.md "Bilateral grids in the captured step" carries the same derivation):

  coordinates  gx = (x + 0.5) / W * (Wg - 1): x + 0.5 exact, two roundings -> |d tx| <= 2 eps32 (Wg - 1); gy likewise;
               gz = fl(luma) (L - 1) with luma three roundings of partial sums <= S_l = 0.299 |r| + 0.587 |g| + 0.114 |b|
               -> |d tz| <= eps32 (L - 1) (3 S_l + 1); counted as (L - 1) (4 S_l + 1).  g - floor(g) is exact.  In eps32 units:
               d_xy = 2 (Wg - 1) + 2 (Hg - 1),   d_z = (L - 1) (4 S_l + 1).
  slice        M_k: three lerp levels fma(t, b - a, a), each rounds b - a (<= 2 eps32 G_k) and the fma (<= eps32 G_k) and passes
               its inputs' errors on as a convex combination: 9 eps32 G_k, counted as 12; a perturbed weight moves the value by
               at most the cell's range 2 G_k per unit  ->  bound_M = eps32 G_k (12 + 2 (d_xy + d_z)).
               D_k = M_z1 - M_z0: two levels each (6, counted 8, + 2 d_xy on 2 G_k), the subtraction 2 eps32 G_k, one of slack
               ->  bound_D = eps32 G_k (19 + 4 d_xy).
  apply        out_i = fma chain of three roundings over S_i = sum_j G_ij |c_j| + G_i3 -> 4 eps32 S_i + sum_j bound_M_ij |c_j| + bound_M_i3.
  vjp          (M^T v)_j: 4 eps32 sum_i G_ij |v_i| + sum_i bound_M_ij |v_i|;  through the guide, with E_i = sum_j 2 G_ij |c_j| + 2 G_i3
               >= |D_i . [c; 1]|:  err(e_i) <= sum_j bound_D_ij |c_j| + bound_D_i3 + 4 eps32 E_i;  s = sum_i v_i e_i: three more
               roundings; (L - 1) s: one; the closing fma: one  ->  w_j (L - 1) (sum_i |v_i| err(e_i) + 8 eps32 sum_i |v_i| E_i).
  adjoint      v_slab[k][z][y][x] = sum_p wz wy wx a_pk, a_pk = {v_i c_j, v_i} exact in fp64, the weights in fp64 from the fp32
               fractions: a weight is off by at most eps32 (d_xy + d_z) (each of the three factors is <= 1), for every pixel whose
               cell touches the node  ->  eps32 sum_{p touching} (d_xy + d_z[p]) |a_pk|, plus the fp64 sum: one fp32 ulp of the
               result and 1e-12 sum_{p touching} |a_pk|.  "Touching" is taken with 1e-3 of slack per axis, so a pixel that fp32
               puts into the neighbouring cell is counted at the node it then reaches.
  tv           the value: fp64 in a fixed order, one rounding -> one fp32 ulp + 1e-12 sum |terms|; the gradient
               fl32(tv_weight * d tv / d G) with the derivative in fp64 -> one fp32 ulp + 1e-12 sum |its terms|.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
LUMA = np.array([0.299, 0.587, 0.114])
KINK_MARGIN = 1e-3                                   # grid units every pixel keeps from a kink of the guide
FRAMES = [(1, 1), (11, 13), (37, 53)]                # (H, W): one pixel, under one block, ragged
GRIDS = [(16, 16, 8), (5, 3, 2), (2, 2, 2)]          # (Wg, Hg, L): the default, Wg != Hg with the least L, a single cell


def random_grids(rng, n_views, Wg, Hg, L):
    """[n_views, 12, L, Hg, Wg] fp32: [I | 0] plus uniform noise of +-0.3 on every node -- nothing is smooth, nothing commutes."""
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12)
    g = eye[None, :, None, None, None] + rng.uniform(-0.3, 0.3, (n_views, 12, L, Hg, Wg))
    return np.ascontiguousarray(g.astype(np.float32))


def kink_distance(img, L):
    """Per pixel the distance of luma * (L - 1) (fp64, un-clamped) to the nearest node 0 .. L - 1: where it is 0 the gradient
    through the guide jumps (a node between two cells, or the clamp at luma = 0 and 1)."""
    g = (np.asarray(img, dtype=np.float64) @ LUMA) * (L - 1)
    return np.min(np.abs(g[..., None] - np.arange(L)), axis=-1)


def random_images(rng, H, W, L):
    """A render-like image in [-0.2, 1.2]^3 with 8 % of its pixels (at least one when there are 10) pushed below luma 0 and 8 %
    above luma 1, every pixel re-drawn until it keeps KINK_MARGIN from the guide's kinks; a gradient-like image (normal, 1e-4
    scale with a few large entries).  fp32 [H, W, 3] each."""
    img = rng.uniform(-0.2, 1.2, (H, W, 3))
    pick = rng.random((H, W))
    lo, hi = pick < 0.08, pick > 0.92
    img[lo] = rng.uniform(-0.2, -0.01, (int(lo.sum()), 3))
    img[hi] = rng.uniform(1.01, 1.2, (int(hi.sum()), 3))
    img = img.astype(np.float32)
    for _ in range(100):
        bad = kink_distance(img, L) < 2.0 * KINK_MARGIN
        if not bad.any():
            break
        img[bad] = (img[bad] + rng.uniform(-0.05, 0.05, (int(bad.sum()), 3))).astype(np.float32)
    v = (1e-4 * rng.standard_normal((H, W, 3))).astype(np.float32)
    v[rng.random((H, W)) < 0.01] *= 1e3
    return img, v


def _coords(H, W, dtype=torch.float64):
    xs = (2.0 * (torch.arange(W, dtype=dtype) + 0.5) / W - 1.0).expand(H, W)
    ys = (2.0 * (torch.arange(H, dtype=dtype) + 0.5) / H - 1.0)[:, None].expand(H, W)
    return xs, ys


def slice_torch(grids, image, view):
    """The issue's expression on torch tensors of one dtype (differentiable)."""
    H, W = image.shape[:2]
    xs, ys = _coords(H, W, image.dtype)
    luma = 0.299 * image[..., 0] + 0.587 * image[..., 1] + 0.114 * image[..., 2]
    xyz = torch.stack([xs, ys, 2.0 * luma - 1.0], dim=-1)[None, None]
    M = F.grid_sample(grids[view:view + 1], xyz, mode="bilinear", align_corners=True, padding_mode="border")
    M = M[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (M[..., :3] @ image[..., None])[..., 0] + M[..., 3]


def tv_torch(grids):
    n = grids.shape[0]
    total = grids.new_zeros(())
    for dim in (2, 3, 4):
        d = grids.narrow(dim, 1, grids.shape[dim] - 1) - grids.narrow(dim, 0, grids.shape[dim] - 1)
        total = total + d.pow(2).sum() / (d.numel() // n)
    return total / n


def slice64(grids, img, v, view):
    """fp64 reference of one frame: {"out", "v_c": [H, W, 3], "v_grids": [n_views, 12, L, Hg, Wg]} (the gradients of sum(out * v))."""
    g = torch.from_numpy(np.asarray(grids, dtype=np.float64)).requires_grad_(True)
    c = torch.from_numpy(np.asarray(img, dtype=np.float64)).requires_grad_(True)
    out = slice_torch(g, c, view)
    (out * torch.from_numpy(np.asarray(v, dtype=np.float64))).sum().backward()
    return {"out": out.detach().numpy(), "v_c": c.grad.numpy(), "v_grids": g.grad.numpy()}


def bounds64(slab, img, v):
    """{"out", "v_c": [H, W, 3], "v_slab": [12, L, Hg, Wg]}: the bounds of the module docstring for one view's slab; `ref_slab`
    (the fp64 v_slab) adds its fp32 ulp in `slab_bound`."""
    slab = np.asarray(slab, dtype=np.float64)
    c, v = np.abs(np.asarray(img, dtype=np.float64)), np.abs(np.asarray(v, dtype=np.float64))
    _, L, Hg, Wg = slab.shape
    H, W = c.shape[:2]
    G = np.abs(slab).reshape(12, -1).max(axis=1).reshape(3, 4)
    c1 = np.concatenate([c, np.ones((H, W, 1))], axis=-1)                       # |[c; 1]|
    d_xy = 2.0 * (Wg - 1) + 2.0 * (Hg - 1)
    d_z = (L - 1) * (4.0 * (c @ LUMA) + 1.0)                                      # [H, W]
    kM = 12.0 + 2.0 * (d_xy + d_z)                                                # bound_M = eps32 G_k kM
    kD = 19.0 + 4.0 * d_xy
    S = c1 @ G.T                                                                  # [H, W, 3]: sum_j G_ij |c_j| + G_i3
    out_b = EPS32 * (4.0 + kM[..., None]) * S
    vG = v @ G[:, :3]                                                             # [H, W, 3]: sum_i G_ij |v_i|
    E = 2.0 * S
    err_e = EPS32 * (kD + 4.0) * E
    guide = (L - 1) * ((v * err_e).sum(-1) + 8.0 * EPS32 * (v * E).sum(-1))       # [H, W]
    vc_b = EPS32 * (4.0 + kM[..., None]) * vG + guide[..., None] * LUMA
    # the adjoint: |a_pk| over the pixels that touch a node, weighted (the weights' perturbation) and plain (the fp64 sum)
    a = (v[..., :, None] * c1[..., None, :]).reshape(H, W, 12)
    gx = (np.arange(W) + 0.5) / W * (Wg - 1)
    gy = (np.arange(H) + 0.5) / H * (Hg - 1)
    gz = np.clip(np.asarray(img, dtype=np.float64) @ LUMA, 0.0, 1.0) * (L - 1)
    tx = (np.abs(gx[:, None] - np.arange(Wg)) < 1.0 + 1e-3).astype(np.float64)    # [W, Wg]
    ty = (np.abs(gy[:, None] - np.arange(Hg)) < 1.0 + 1e-3).astype(np.float64)    # [H, Hg]
    tz = (np.abs(gz[..., None] - np.arange(L)) < 1.0 + 1e-3).astype(np.float64)   # [H, W, L]
    pert = np.einsum("hwk,hwz,hy,wx->kzyx", a * (d_xy + d_z)[..., None], tz, ty, tx)
    mag = np.einsum("hwk,hwz,hy,wx->kzyx", a, tz, ty, tx)
    return {"out": out_b, "v_c": vc_b, "v_slab_pert": EPS32 * pert, "v_slab_mag": mag}


def slab_bound(b, ref_slab):
    ulp = np.spacing(np.abs(ref_slab).astype(np.float32)).astype(np.float64)
    return b["v_slab_pert"] + ulp + 1e-12 * b["v_slab_mag"]


def tv64(grids, tv_weight=1.0):
    """(tv, bound, tv_weight * d tv / d grids, bound) in fp64.  The value's terms are the squared differences over n_views count_a;
    a node's gradient terms are the (at most six) differences it enters, times 2 tv_weight / (n_views count_a)."""
    g = torch.from_numpy(np.asarray(grids, dtype=np.float64)).requires_grad_(True)
    tv = tv_torch(g)
    (float(np.float32(tv_weight)) * tv).backward()
    tv, grad = float(tv.detach()), g.grad.numpy()
    gn = np.asarray(grids, dtype=np.float64)
    n = gn.shape[0]
    mag = np.zeros_like(gn)
    for ax in (2, 3, 4):
        d = np.abs(np.diff(gn, axis=ax))
        w = 2.0 * abs(float(np.float32(tv_weight))) / (d.size // n * n)
        lo, hi = [slice(None)] * 5, [slice(None)] * 5
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        mag[tuple(lo)] += w * d
        mag[tuple(hi)] += w * d
    tv_bound = float(np.spacing(np.float32(abs(tv)))) + 1e-12 * abs(tv)   # (every term is a square: sum |terms| = tv)
    grad_bound = np.spacing(np.abs(grad).astype(np.float32)).astype(np.float64) + 1e-12 * mag
    return tv, tv_bound, grad, grad_bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0; a NaN counts as infinite)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r))
