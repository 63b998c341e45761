"""Exact k-nearest-neighbour distances of a point cloud on the device (csrc/gs_knn.hip): what `GaussianModel.from_pointcloud`
takes from `sklearn.neighbors.NearestNeighbors` on the host path -- `kneighbors(...)[0][:, 1:]` -- to size the initial Gaussians.

Two native stages with one `torch.sort` between them: Morton codes of the points inside their bounding box (`gs_knn_codes`), the
point indices sorted by code, then gather + boxes + search (`gs_knn_dists`).  The order only decides how fast the search goes; the
rows are the exact k smallest float32 distances whatever it is (include/gs_raster.h).  GPU only: there is no CPU fallback.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _native as nat

LEAF = nat.GS_KNN_LEAF      # points per leaf of the search (one wavefront of queries)
MAX_K = nat.GS_KNN_MAX_K
MAX_N = nat.GS_KNN_MAX_N


@torch.no_grad()
def knn_distances(points: Tensor, k: int = 3, check_finite: bool = True) -> Tensor:
    """-> `[N, k]` float32 on `points`' device: row i holds the k smallest of `{|p_i - p_j| : j != i}`, ascending, rows in the
    caller's order.  Self is excluded by index: coincident points are neighbours at exactly 0; no floor is applied.
    `points`: contiguous float32 `[N, 3]` on a HIP device, `1 <= k <= 8`, `N >= k + 1`.  `check_finite` reads one flag back and
    raises `ValueError` on a NaN or an infinity before anything is launched (without it such a cloud gives meaningless rows).
    Runs on the current stream; the scratch buffers are plain allocations (this runs once per training run)."""
    if not isinstance(points, Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be a [N, 3] tensor, got {tuple(points.shape) if isinstance(points, Tensor) else type(points).__name__}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if not points.is_contiguous():
        raise ValueError("points must be contiguous")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    n = int(points.shape[0])
    if n < k + 1:
        raise ValueError(f"{k} neighbours need at least {k + 1} points, got {n}")
    if n > MAX_N:
        raise ValueError(f"at most {MAX_N} points (int32 indices), got {n}")
    if check_finite and not bool(torch.isfinite(points).all()):
        raise ValueError("points contains NaN or infinity")
    if points.device.type != "cuda":
        raise NotImplementedError("knn_distances runs on the GPU only (csrc/gs_knn.hip); there is no CPU fallback -- "
                                  "GaussianModel.from_pointcloud(knn='host') is the host path")
    L, dev = nat.lib(), points.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        ws = torch.empty((int(L.gs_knn_workspace_bytes(n)),), dtype=torch.uint8, device=dev)
        codes = torch.empty((n,), dtype=torch.int64, device=dev)
        nat.check(L.gs_knn_codes(st, n, points.data_ptr(), ws.data_ptr(), codes.data_ptr()), "gs_knn_codes")
        order = torch.sort(codes, stable=True).indices.to(torch.int32)
        dists = torch.empty((n, k), dtype=torch.float32, device=dev)
        nat.check(L.gs_knn_dists(st, n, k, points.data_ptr(), order.data_ptr(), dists.data_ptr(), ws.data_ptr()), "gs_knn_dists")
    return dists
