"""fp64 reference of the exposure kernels (csrc/gs_exposure.h) and the bounds a correct fp32 kernel keeps -- shared by
tests/test_exposure_host.py (the header built with the host compiler) and tests/test_gpu_exposure.py (the device).

A table row is T[3][4] = [A | b].  With eps32 = 2^-24, the unit round-off of fp32:

  apply   out_i = fma(A_i2, c_2, fma(A_i1, c_1, fma(A_i0, c_0, b_i))): three roundings, each of a partial sum no larger than
          S_i = |b_i| + sum_j |A_ij c_j|  ->  |error| <= 3 eps32 S_i; the bound is 4 eps32 S_i (one of slack).
  vjp     (A^T v)_j = fma(A_2j, v_2, fma(A_1j, v_1, A_0j v_0)): three roundings  ->  4 eps32 sum_i |A_ij v_i|.
  sums    dA_ij = sum_p v_i[p] c_j[p], db_i = sum_p v_i[p]: products exact in fp64, fp64 accumulation, ONE rounding to fp32
          ->  one fp32 ulp of the fp64 sum (the rounding, and the sum's own error carried across a rounding boundary) plus
          1e-12 sum_p |term| for the fp64 accumulation (a chain of n additions errs by at most n 2^-53 sum |term|: 2.2e-13 at
          n = 2000 in pixel order, far less through the kernels' trees).
"""
import numpy as np

EPS32 = 2.0 ** -24
FRAMES = [(11, 11), (11, 13), (37, 53), (208, 320)]   # (H, W): under one block (tail 1, tail 3), ragged with a tail of 1, several blocks
BIG_FRAME = (1080, 1920)                               # beyond the block cap: every thread strides


def random_table(rng, n_views):
    """[n_views, 3, 4] fp32 with entries in [-1.5, 1.5]."""
    return rng.uniform(-1.5, 1.5, (n_views, 3, 4)).astype(np.float32)


def random_images(rng, H, W):
    """A render-like image in [-0.2, 1.2] and a gradient-like image (normal, 1e-4 scale with a few large entries), fp32 [H, W, 3]."""
    img = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32)
    v = (1e-4 * rng.standard_normal((H, W, 3))).astype(np.float32)
    v[rng.random((H, W)) < 0.01] *= 1e3
    return img, v


def apply64(T, img):
    """(out, bound) of the forward: fp64 [.., 3] each."""
    T, c = np.asarray(T, dtype=np.float64), np.asarray(img, dtype=np.float64)
    out = c @ T[:, :3].T + T[:, 3]
    S = np.abs(c) @ np.abs(T[:, :3]).T + np.abs(T[:, 3])
    return out, 4.0 * EPS32 * S


def vjp64(T, v):
    """(A^T v, bound): fp64 [.., 3] each."""
    T, v = np.asarray(T, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return v @ T[:, :3], 4.0 * EPS32 * (np.abs(v) @ np.abs(T[:, :3]))


def sums64(v, img):
    """(sums [3, 4], bound [3, 4]) of the affine's gradient.  Each sum is numpy's pairwise sum over a contiguous vector of exact
    products: its own error is a few 2^-53 of sum |term|, far inside the 1e-12 it is compared under."""
    v, c = np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(img, dtype=np.float64).reshape(-1, 3)
    cols = [np.ascontiguousarray(c[:, j]) for j in range(3)] + [np.ones(c.shape[0])]
    ref, mag = np.empty((3, 4)), np.empty((3, 4))
    for i in range(3):
        vi = np.ascontiguousarray(v[:, i])
        for j in range(4):
            terms = vi * cols[j]
            ref[i, j], mag[i, j] = terms.sum(), np.abs(terms).sum()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return ref, ulp + 1e-12 * mag


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r))
