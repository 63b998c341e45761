"""Lloyd's k-means on the device (csrc/gs_kmeans.hip): the codebook `compress.save_compact` builds over the higher SH bands.

An iteration is two native stages with one `torch.sort` between them: `gs_kmeans_assign` (the fused product + argmin on the f32-input
MFMA: no score matrix is stored), the point indices sorted by label with a stable sort and the segment offsets of the labels, then
`gs_kmeans_update` (fp64 sums in ascending point order).  Labels, distances and centroids are the functions csrc/gs_kmeans.h states,
bit for bit: the same input gives the same result whatever the tiling.  GPU only: there is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _native as nat

MAX_D = nat.GS_KMEANS_MAX_D
MAX_K = nat.GS_KMEANS_MAX_K
MAX_N = nat.GS_KMEANS_MAX_N


def _check_points(x, name: str = "x") -> None:
    if not isinstance(x, Tensor) or x.dim() != 2:
        raise ValueError(f"{name} must be a [N, D] tensor, got {tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_sizes(n: int, k: int, d: int) -> None:
    if not 1 <= d <= MAX_D:
        raise ValueError(f"D must be in [1, {MAX_D}], got {d}")
    if not 1 <= n <= MAX_N:
        raise ValueError(f"N must be in [1, {MAX_N}] (int32 indices), got {n}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")


def _check_device(x: Tensor, centroids: Tensor, what: str) -> None:
    if x.device.type != "cuda":
        raise NotImplementedError(f"{what} runs on the GPU only (csrc/gs_kmeans.hip); there is no CPU fallback")
    if centroids.device != x.device:
        raise ValueError(f"centroids are on {centroids.device}, the points on {x.device}")


@torch.no_grad()
def assign(x: Tensor, centroids: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (labels int32 [N], dist2 float32 [N]): for every row of `x` [N, D] the index of the nearest row of `centroids` [K, D] -- the
    smallest index among the centroids of minimal score, csrc/gs_kmeans.h -- and the squared distance to it.  Contiguous float32
    HIP tensors; runs on the current stream."""
    _check_points(x)
    _check_points(centroids, "centroids")
    if centroids.shape[1] != x.shape[1]:
        raise ValueError(f"centroids have {centroids.shape[1]} columns, the points {x.shape[1]}")
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(centroids.shape[0])
    _check_sizes(n, k, d)
    _check_device(x, centroids, "kmeans.assign")
    L, dev = nat.lib(), x.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        ws = torch.empty((int(L.gs_kmeans_workspace_bytes(n, k, d)),), dtype=torch.uint8, device=dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        dist2 = torch.empty((n,), dtype=torch.float32, device=dev)
        nat.check(L.gs_kmeans_assign(st, n, k, d, x.data_ptr(), centroids.data_ptr(), labels.data_ptr(), dist2.data_ptr(), ws.data_ptr()),
                  "gs_kmeans_assign")
    return labels, dist2


@torch.no_grad()
def update(x: Tensor, labels: Tensor, centroids: Tensor) -> Tensor:
    """Moves every row of `centroids` [K, D] IN PLACE to the mean of the rows of `x` labelled with it (fp64 sums in ascending point
    order, rounded once); a centroid nobody is labelled with keeps its bits.  -> counts int32 [K].  `labels`: int32 [N] in [0, K)."""
    _check_points(x)
    _check_points(centroids, "centroids")
    if centroids.shape[1] != x.shape[1]:
        raise ValueError(f"centroids have {centroids.shape[1]} columns, the points {x.shape[1]}")
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(centroids.shape[0])
    _check_sizes(n, k, d)
    if not isinstance(labels, Tensor) or labels.dtype != torch.int32 or labels.shape != (n,) or not labels.is_contiguous():
        raise ValueError(f"labels must be a contiguous int32 [{n}] tensor")
    _check_device(x, centroids, "kmeans.update")
    if labels.device != x.device:
        raise ValueError(f"labels are on {labels.device}, the points on {x.device}")
    L, dev = nat.lib(), x.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        order = torch.sort(labels, stable=True).indices.to(torch.int32)
        seg = torch.zeros((k + 1,), dtype=torch.int32, device=dev)
        seg[1:] = torch.cumsum(torch.bincount(labels, minlength=k)[:k], 0)
        counts = torch.empty((k,), dtype=torch.int32, device=dev)
        nat.check(L.gs_kmeans_update(st, n, k, d, x.data_ptr(), order.data_ptr(), seg.data_ptr(), centroids.data_ptr(), counts.data_ptr()),
                  "gs_kmeans_update")
    return counts


@torch.no_grad()
def kmeans(x: Tensor, k: int, iters: int = 5, init: Optional[Tensor] = None,
           generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor, List[Tensor]]:
    """-> (centroids float32 [K, D], labels int32 [N], inertia): `iters` Lloyd iterations (assign, update) and a closing assign, so
    the labels belong to the centroids returned.  `init`: the caller's [k, D] centroids (copied), or `x[randperm(N, generator)[:k]]`
    (the permutation is drawn on the generator's device -- the CPU without one -- so a seed gives the same codebook everywhere).
    `inertia`: one 0-d float64 device tensor per assignment (iters + 1 of them), the sum of dist2 in a fixed order; nothing is read
    back.  N <= k returns the points themselves as the codebook, labels = arange(N), and launches nothing.
    `x`: contiguous float32 [N, D]; with N > k it must be on a HIP device (`NotImplementedError` otherwise)."""
    _check_points(x)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"iters must be a non-negative integer, got {iters!r}")
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 1:
        raise ValueError("no points")
    if init is not None:
        _check_points(init, "init")
        if tuple(init.shape) != (k, d):
            raise ValueError(f"init must be [{k}, {d}], got {tuple(init.shape)}")
    if n <= k:
        return x.clone(), torch.arange(n, dtype=torch.int32, device=x.device), []
    _check_sizes(n, k, d)
    if x.device.type != "cuda":
        raise NotImplementedError("kmeans runs on the GPU only (csrc/gs_kmeans.hip); there is no CPU fallback")
    if init is not None:
        centroids = init.to(x.device).clone()
    else:
        perm = torch.randperm(n, generator=generator, device=generator.device if generator is not None else "cpu")
        centroids = x[perm[:k].to(x.device)].contiguous()
    inertia: List[Tensor] = []
    for _ in range(iters):
        labels, dist2 = assign(x, centroids)
        inertia.append(dist2.double().sum())
        update(x, labels, centroids)
    labels, dist2 = assign(x, centroids)
    inertia.append(dist2.double().sum())
    return centroids, labels, inertia
