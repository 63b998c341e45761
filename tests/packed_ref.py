"""What `rasterization(packed=True)` hands out, written down a second time from a dense `radii` [C,N] array alone.

The visible pairs are the (c, n) with radii[c, n] > 0 in row-major order -- camera-major, Gaussian ascending; the packed row of a
pair is its rank in that order; the seen Gaussians are the n some camera saw, ascending.  `*_loops` spell it with plain Python loops
(the definition, for hand-sized inputs); the tensor forms compute the same with torch on whatever device `radii` lives on and are
what the GPU tests apply to the dense call's meta."""
import torch


def pairs_loops(radii):
    """radii: nested lists [C][N] -> (camera_ids, gaussian_ids) as lists."""
    cams, gids = [], []
    for c, row in enumerate(radii):
        for n, r in enumerate(row):
            if r > 0:
                cams.append(c)
                gids.append(n)
    return cams, gids


def union_ids_loops(radii):
    n_gauss = len(radii[0]) if radii else 0
    return [n for n in range(n_gauss) if any(row[n] > 0 for row in radii)]


def renumber_loops(radii, flatten_ids):
    """Dense pair indices c*N + n -> packed rows (-1 for an index that is no visible pair: a list never holds one)."""
    n_gauss = len(radii[0]) if radii else 0
    cams, gids = pairs_loops(radii)
    row = {c * n_gauss + n: k for k, (c, n) in enumerate(zip(cams, gids))}
    return [row.get(int(f), -1) for f in flatten_ids]


def pairs(radii: torch.Tensor):
    """(camera_ids, gaussian_ids), int64 [nnz] each."""
    assert radii.dim() == 2
    idx = torch.nonzero(radii > 0)   # (row-major: lexicographic in (c, n))
    return idx[:, 0].contiguous(), idx[:, 1].contiguous()


def union_ids(radii: torch.Tensor) -> torch.Tensor:
    if radii.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.int64, device=radii.device)
    return torch.nonzero((radii > 0).any(dim=0))[:, 0].contiguous()


def renumber(radii: torch.Tensor, flatten_ids: torch.Tensor) -> torch.Tensor:
    vis = (radii > 0).reshape(-1)
    row = torch.cumsum(vis.to(torch.int64), 0) - 1
    row = torch.where(vis, row, torch.full_like(row, -1))
    return row[flatten_ids.long()].to(flatten_ids.dtype)


def pack_meta(dense: dict) -> dict:
    """The packed meta a dense call's meta stands for: ids, the per-pair arrays gathered, the list arrays."""
    radii = dense["radii"]
    cam, gid = pairs(radii)
    out = {"camera_ids": cam, "gaussian_ids": gid}
    for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss"):
        out[k] = dense[k][cam, gid]
    out["flatten_ids"] = renumber(radii, dense["flatten_ids"])
    out["isect_ids"], out["isect_offsets"] = dense["isect_ids"], dense["isect_offsets"]
    return out
