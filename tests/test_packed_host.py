"""`rasterization(packed=True, sparse_grad=True)` without a GPU: the refusals, the four entry points of gs_packed.hip in the header,
and tests/packed_ref.py -- the definition the GPU tests (tests/test_gpu_packed.py) hold the kernels to -- on hand-written cases."""
import pytest
import torch

import packed_ref as PR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.rendering import rasterization


def _args(N=4, C=1):
    return (torch.zeros(N, 3), torch.ones(N, 4), torch.ones(N, 3), torch.ones(N), torch.zeros(N, 1, 3),
            torch.eye(4)[None].repeat(C, 1, 1), torch.eye(3)[None].repeat(C, 1, 1), 32, 32)


def test_packed_on_cpu_tensors_is_refused_as_gpu_only():
    with pytest.raises(NotImplementedError, match="GPU only"):
        rasterization(*_args(), sh_degree=0, packed=True)
    with pytest.raises(NotImplementedError, match="GPU only"):
        rasterization(*_args(), sh_degree=0)   # gsplat's default
    with pytest.raises(NotImplementedError, match="GPU only"):
        rasterization(*_args(), sh_degree=0, packed=True, sparse_grad=True)


def test_sparse_grad_needs_packed():
    with pytest.raises(NotImplementedError, match="sparse_grad requires packed=True"):
        rasterization(*_args(), sh_degree=0, packed=False, sparse_grad=True)


@pytest.mark.parametrize("bad", [dict(_sh_grads="colors_pre"), dict(_grad_out={}), dict(_view_payload=torch.zeros(64))],
                         ids=["sh_grads", "grad_out", "view_payload"])
def test_packed_refuses_the_view_parallel_keywords(bad):
    with pytest.raises(ValueError, match="packed=True"):
        rasterization(*_args(), sh_degree=0, packed=True, **bad)


def test_header_declares_the_four_entry_points():
    P = nat.PARAMS
    assert P["gs_pack_flags"] == ["stream", "C", "N", "radii", "want_seen", "flags", "incl", "scan_workspace", "totals_host_mapped"]
    assert P["gs_pack_gather"][:6] == ["stream", "C", "N", "nnz", "radii", "incl"]
    assert P["gs_pack_gather"][-7:] == ["camera_ids", "gaussian_ids", "radii_out", "means2d_out", "depths_out", "conics_out", "opacities_out"]
    assert P["gs_pack_take"] == ["stream", "n_src", "n_out", "words", "incl", "base", "src", "out", "ids_out"]
    assert P["gs_pack_remap"] == ["stream", "n", "pairs", "flatten_ids", "incl", "out"]
    import ctypes as ct
    for name in ("gs_pack_flags", "gs_pack_gather", "gs_pack_take", "gs_pack_remap"):
        assert nat.SIGNATURES[name][0] is ct.c_int and nat.SIGNATURES[name][1][0] is ct.c_void_p


def test_fused_adam_refuses_a_sparse_grad_before_anything_moves():
    """(The refusal sits in front of everything `step` loads or launches: it needs neither the library nor a GPU.)"""
    from easy_gaussian_splatting_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.ones(5, 3))
    opt = FusedAdam([{"params": [p], "lr": 0.1, "name": "means"}])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3]]), torch.ones(2, 3), size=(5, 3))
    with pytest.raises(TypeError, match=r"step\(visible=.*torch\.optim\.SparseAdam"):
        opt.step()
    assert opt._step == 0 and torch.equal(p.detach(), torch.ones(5, 3))


# radii [C][N], camera_ids, gaussian_ids, union ids, a list of dense pair indices and its packed rows
HAND = {
    "empty": ([[], []], [], [], [], [], []),
    "all_culled": ([[0, 0, 0], [0, -1, 0]], [], [], [], [], []),
    "all_visible": ([[3, 1], [2, 9]], [0, 0, 1, 1], [0, 1, 0, 1], [0, 1], [3, 0, 2, 2, 1], [3, 0, 2, 2, 1]),
    "last_slot": ([[0, 0, 0], [0, 0, 5]], [1], [2], [2], [5, 5], [0, 0]),
    "mixed": ([[4, 0, 1, 0], [0, 0, 2, 7]], [0, 0, 1, 1], [0, 2, 2, 3], [0, 2, 3], [7, 0, 6, 2], [3, 0, 2, 1]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_packed_ref_on_hand_written_cases(name):
    radii, cams, gids, union, flat, rows = HAND[name]
    assert PR.pairs_loops(radii) == (cams, gids)
    assert PR.union_ids_loops(radii) == union
    assert PR.renumber_loops(radii, flat) == rows
    n = len(radii[0])
    r = torch.tensor(radii, dtype=torch.int32).reshape(len(radii), n)
    c, g = PR.pairs(r)
    assert c.dtype == g.dtype == torch.int64 and c.tolist() == cams and g.tolist() == gids
    assert PR.union_ids(r).tolist() == union
    assert PR.renumber(r, torch.tensor(flat, dtype=torch.int32)).tolist() == rows
    # the packed row of a listed pair indexes the pair back
    for f, k in zip(flat, rows):
        assert (cams[k], gids[k]) == (f // n, f % n)


def test_packed_ref_pack_meta_gathers_and_renumbers():
    radii = torch.tensor([[4, 0, 1, 0], [0, 0, 2, 7]], dtype=torch.int32)
    dense = {"radii": radii, "means2d": torch.arange(16.).reshape(2, 4, 2), "depths": torch.arange(8.).reshape(2, 4),
             "conics": torch.arange(24.).reshape(2, 4, 3), "opacities": torch.arange(4.)[None].expand(2, 4),
             "tiles_per_gauss": torch.tensor([[1, 0, 2, 0], [0, 0, 1, 1]], dtype=torch.int32),
             "flatten_ids": torch.tensor([7, 0, 6, 2], dtype=torch.int32), "isect_ids": torch.zeros(4, dtype=torch.int64),
             "isect_offsets": torch.zeros((2, 1, 1), dtype=torch.int32)}
    p = PR.pack_meta(dense)
    assert p["radii"].tolist() == [4, 1, 2, 7] and p["depths"].tolist() == [0., 2., 6., 7.] and p["opacities"].tolist() == [0., 2., 2., 3.]
    assert p["means2d"].tolist() == [[0., 1.], [4., 5.], [12., 13.], [14., 15.]] and p["tiles_per_gauss"].tolist() == [1, 2, 1, 1]
    assert p["flatten_ids"].tolist() == [3, 0, 2, 1] and p["isect_offsets"] is dense["isect_offsets"]
