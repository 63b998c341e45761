"""Brute-force reference for the k-nearest-neighbour distances (tests/test_knn_host.py, tests/test_gpu_knn.py): float64 on the
coordinates it is given, in row chunks, self excluded by INDEX (a coincident point is a neighbour at distance 0), the k smallest
of every row in ascending order.  A numpy version for the host tests and a torch-float64 version that runs on whatever device
its input is on; neither touches the package."""
import numpy as np
import torch


def knn_ref_numpy(points, k, chunk=512):
    """points [N, 3] (any float dtype; promoted to float64, exactly) -> [N, k] float64."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    assert p.ndim == 2 and p.shape[1] == 3 and 1 <= k < n
    out = np.empty((n, k), dtype=np.float64)
    for r0 in range(0, n, chunk):
        r1 = min(r0 + chunk, n)
        diff = p[r0:r1, None, :] - p[None, :, :]
        d2 = (diff * diff).sum(axis=2)
        d2[np.arange(r1 - r0), np.arange(r0, r1)] = np.inf
        out[r0:r1] = np.sqrt(np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1))
    return out


def knn_ref_torch(points, k, chunk=512):
    """points [N, 3] tensor on any device (promoted to float64, exactly) -> [N, k] float64 on the same device."""
    p = points.detach().to(torch.float64)
    n = p.shape[0]
    assert p.dim() == 2 and p.shape[1] == 3 and 1 <= k < n
    out = torch.empty((n, k), dtype=torch.float64, device=p.device)
    for r0 in range(0, n, chunk):
        r1 = min(r0 + chunk, n)
        d2 = torch.zeros((r1 - r0, n), dtype=torch.float64, device=p.device)
        for a in range(3):   # (dx^2 + dy^2) + dz^2, an axis at a time: no [chunk, N, 3] temporary
            d2 += (p[r0:r1, a, None] - p[None, :, a]) ** 2
        d2[torch.arange(r1 - r0, device=p.device), torch.arange(r0, r1, device=p.device)] = float("inf")
        out[r0:r1] = torch.sqrt(torch.topk(d2, k, dim=1, largest=False, sorted=True).values)
    return out
