"""Bilateral grids without a GPU: the per-pixel math of the kernels (csrc/gs_bilagrid.h) built with the host compiler -- the
device's own text -- against torch's grid_sample in fp64 (tests/bilagrid_ref.py states the bounds), the cell indices of hostile
pixels, the plain-torch path of `BilateralGrids`, the new entries of the C ABI and the refusals that must come before any device
work."""
import ctypes as ct
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import adam_ref as A
import bilagrid_ref as R
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.bilagrid import BilagridAdamState, BilateralGrids

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = {
    "gs_bilagrid_step_inputs": ["stream", "view", "n_views", "lr", "beta1", "beta2", "step", "rec_dev"],
    "gs_bilagrid_apply": ["stream", "height", "width", "n_views", "grid_x", "grid_y", "grid_l", "rec_dev", "view", "grids", "render", "out"],
    "gs_bilagrid_partials_doubles": ["height", "width", "grid_x", "grid_y", "grid_l"],
    "gs_bilagrid_bwd": ["stream", "height", "width", "n_views", "grid_x", "grid_y", "grid_l", "rec_dev", "view", "grids", "render", "v_image",
                        "partials", "v_slab"],
    "gs_bilagrid_tv": ["stream", "n_views", "grid_x", "grid_y", "grid_l", "grids", "tv_weight", "rec_dev", "view", "v_slab", "loss3", "tv_out",
                       "v_grids", "tv_ws"],
    "gs_bilagrid_adam": ["stream", "numel", "rec_dev", "grids", "exp_avg", "exp_avg_sq", "v_grids", "beta1", "beta2", "eps"],
}
N_VIEWS = 3


@pytest.fixture(scope="module")
def bm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bm") / "libbilagridmath.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "bilagridmath.cpp")], check=True)
    L = ct.CDLL(so)
    P, F, I = ct.c_void_p, ct.c_float, ct.c_int
    L.bm_cells.argtypes, L.bm_cells.restype = [P, I, I, I, I, I, P], None
    L.bm_axis_first.argtypes, L.bm_axis_first.restype = [I, I, P], None
    L.bm_apply.argtypes, L.bm_apply.restype = [P, P, I, I, I, I, I, P], None
    L.bm_vjp.argtypes, L.bm_vjp.restype = [P, P, P, I, I, I, I, I, P], None
    L.bm_adjoint.argtypes, L.bm_adjoint.restype = [P, P, I, I, I, I, I, P], None
    L.bm_tv.argtypes, L.bm_tv.restype = [P, I, I, I, I, F, P, P], None
    L.bm_adam.argtypes, L.bm_adam.restype = [P, P, P, P, ct.c_int64, F, F, F, F, F], None
    return L


def _ptr(a):
    return a.ctypes.data_as(ct.c_void_p)


@functools.lru_cache(maxsize=None)
def _case(H, W, Wg, Hg, L):
    """Inputs of one frame and grid size, computed once and shared (read-only) by the three views' tests."""
    rng = np.random.default_rng(100000 * H + 1000 * W + 100 * Wg + 10 * Hg + L)
    grids = R.random_grids(rng, N_VIEWS, Wg, Hg, L)
    img, v = R.random_images(rng, H, W, L)
    for x in (grids, img, v):
        x.setflags(write=False)
    return grids, img, v


@pytest.mark.parametrize("view", [0, 1, 2])
@pytest.mark.parametrize("Wg,Hg,L", R.GRIDS, ids=lambda x: str(x))
@pytest.mark.parametrize("H,W", R.FRAMES, ids=lambda x: str(x))
def test_apply_vjp_and_adjoint_keep_their_bounds_against_grid_sample_in_fp64(bm, H, W, Wg, Hg, L, view):
    grids, img, v = _case(H, W, Wg, Hg, L)
    assert R.kink_distance(img, L).min() >= R.KINK_MARGIN   # (asserted on the fp64 luminance: no pixel sits on a kink of the guide)
    luma = img.astype(np.float64) @ R.LUMA
    if H * W >= 100:
        assert (luma < 0).mean() >= 0.05 and (luma > 1).mean() >= 0.05
    slab = np.ascontiguousarray(grids[view])
    out, dv, v_slab = np.empty_like(img), np.empty_like(v), np.empty_like(slab)
    bm.bm_apply(_ptr(slab), _ptr(img), H, W, Wg, Hg, L, _ptr(out))
    bm.bm_vjp(_ptr(slab), _ptr(img), _ptr(v), H, W, Wg, Hg, L, _ptr(dv))
    bm.bm_adjoint(_ptr(img), _ptr(v), H, W, Wg, Hg, L, _ptr(v_slab))
    ref, b = R.slice64(grids, img, v, view), R.bounds64(slab, img, v)
    others = [r for r in range(N_VIEWS) if r != view]
    assert not ref["v_grids"][others].any()   # every other view's slab: exactly zero in the reference itself
    ratios = {"apply": R.worst_ratio(out, ref["out"], b["out"]), "vjp": R.worst_ratio(dv, ref["v_c"], b["v_c"]),
              "adjoint": R.worst_ratio(v_slab, ref["v_grids"][view], R.slab_bound(b, ref["v_grids"][view]))}
    print(f"{H}x{W} grid {(Wg, Hg, L)} view {view}: worst |error| / bound {ratios}")
    assert all(r < 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("Wg,Hg,L", R.GRIDS, ids=lambda x: str(x))
def test_identity_grids_return_the_input_bit_for_bit_and_pass_the_gradient_through(bm, Wg, Hg, L):
    rng = np.random.default_rng(5)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12, 1, 1, 1)
    slab = np.ascontiguousarray(np.broadcast_to(eye, (12, L, Hg, Wg)).astype(np.float32))
    img, v = R.random_images(rng, 37, 53, L)
    img[0, 0] = [np.float32(1e-42), np.float32(-3e38), np.float32(1.0)]   # a subnormal, a huge value
    out, dv = np.empty_like(img), np.empty_like(v)
    bm.bm_apply(_ptr(slab), _ptr(img), 37, 53, Wg, Hg, L, _ptr(out))
    assert np.array_equal(out.view(np.uint32), img.view(np.uint32))
    bm.bm_vjp(_ptr(slab), _ptr(img), _ptr(v), 37, 53, Wg, Hg, L, _ptr(dv))
    assert np.array_equal(dv, v)   # v_luma is exactly 0 and v_c = v_out
    zero = np.array([[[-0.0, 0.0, -0.0]]], dtype=np.float32)   # (a -0 comes back as a zero: +0)
    one = np.empty_like(zero)
    bm.bm_apply(_ptr(slab), _ptr(zero), 1, 1, Wg, Hg, L, _ptr(one))
    assert not one.any() and not np.signbit(one).any()


@pytest.mark.parametrize("Wg,Hg,L", R.GRIDS + [(64, 64, 16), (2, 64, 16)], ids=lambda x: str(x))
def test_hostile_pixels_give_cells_inside_the_slab(bm, Wg, Hg, L):
    H, W = 7, 9
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3.4e38, -3.4e38, 1.0, 0.0, -0.0, 0.5]
    rng = np.random.default_rng(11)
    img = rng.choice(np.array(bad, dtype=np.float32), size=(H, W, 3)).astype(np.float32)
    img[0, 0], img[0, 1], img[0, 2] = [np.inf, -np.inf, 0], [np.nan] * 3, [1e30, 1e30, -1e30]   # inf - inf, NaN, overflow
    cells = np.full((H, W, 3), -99, dtype=np.int32)
    with np.errstate(all="ignore"):
        bm.bm_cells(_ptr(img), H, W, Wg, Hg, L, _ptr(cells))
    for axis, n in enumerate((Wg, Hg, L)):
        assert cells[..., axis].min() >= 0 and cells[..., axis].max() <= n - 2, (axis, cells[..., axis].min(), cells[..., axis].max())


@pytest.mark.parametrize("n_pix", [1, 2, 11, 13, 37, 53, 72, 130, 208, 320, 1080, 1920, 4099])
def test_cells_partition_an_axis_into_the_pixel_ranges_the_blocks_take(bm, n_pix):
    """A block of the image kernels serves the pixels [first(c), first(c + 1)) of its cell: every pixel's own cell (bm_cells, the
    x axis of a one-row image) must be the cell whose range holds it -- a pixel outside every range would never be written, one
    inside two ranges would be read with the wrong nodes."""
    for n_nodes in (2, 3, 5, 16, 64):
        first = np.empty((n_nodes,), dtype=np.int32)
        bm.bm_axis_first(n_pix, n_nodes, _ptr(first))
        img = np.zeros((1, n_pix, 3), dtype=np.float32)
        cells = np.empty((1, n_pix, 3), dtype=np.int32)
        bm.bm_cells(_ptr(img), 1, n_pix, n_nodes, 2, 2, _ptr(cells))
        assert first[0] == 0 and first[-1] == n_pix and (np.diff(first) >= 0).all(), (n_nodes, first)
        owner = np.searchsorted(first[1:], np.arange(n_pix), side="right")   # the c with first[c] <= x < first[c + 1]
        assert np.array_equal(owner, cells[0, :, 0]), n_nodes


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("Wg,Hg,L", R.GRIDS, ids=lambda x: str(x))
def test_total_variation_value_and_gradient_keep_their_bounds(bm, n_views, Wg, Hg, L):
    grids = R.random_grids(np.random.default_rng(40 + n_views), n_views, Wg, Hg, L)
    tv, v_grids = np.empty((1,), dtype=np.float32), np.empty_like(grids)
    bm.bm_tv(_ptr(grids), n_views, Wg, Hg, L, 10.0, _ptr(tv), _ptr(v_grids))
    ref, ref_b, grad, grad_b = R.tv64(grids, 10.0)
    ratios = {"tv": R.worst_ratio(tv[0], ref, ref_b), "grad": R.worst_ratio(v_grids, grad, grad_b)}
    print(f"grid {(Wg, Hg, L)} x {n_views}: tv {ref:.6g}, worst |error| / bound {ratios}")
    assert ref > 0 and bool(grad.all()) and all(r < 1.0 for r in ratios.values()), ratios
    flat = np.ascontiguousarray(np.broadcast_to(grids[:1, :, :1, :1, :1], grids.shape))   # constant grids: no variation at all
    bm.bm_tv(_ptr(flat), n_views, Wg, Hg, L, 10.0, _ptr(tv), _ptr(v_grids))
    assert tv[0] == 0.0 and not v_grids.any()


def test_adam_element_keeps_the_bounds_of_the_fused_adam_kernels(bm):
    p, g, m, v = A.regime_inputs(4096, seed=12)
    lr, t, b1, b2, eps = 2e-3, 7, 0.9, 0.999, 1e-15
    bc1, bc2 = 1.0 - float(np.float32(b1)) ** t, 1.0 - float(np.float32(b2)) ** t
    ss, isbc2 = np.float32(float(np.float32(lr)) / bc1), np.float32(1.0 / np.sqrt(bc2))
    p1, m1, v1 = p.copy(), m.copy(), v.copy()
    bm.bm_adam(_ptr(p1), _ptr(g), _ptr(m1), _ptr(v1), p.size, b1, b2, eps, isbc2, ss)
    ratios = A.error_ratios((p1, m1, v1), p, A.adam_ref(p, g, m, v, lr, t, b1, b2, eps))
    print(f"bilagrid_adam1: error / bound {ratios}")
    assert ratios["p"] <= 1.0 and ratios["m"] <= 1.0 and ratios["v"] <= 1.0, ratios


# ---- the plain-torch path of BilateralGrids: the semantic reference ---------------------------------------------------------------
def test_module_is_the_identity_at_init_and_the_reference_expression_afterwards():
    grids = BilateralGrids(4)
    g = grids.grids
    assert g.shape == (4, 12, 8, 16, 16) and g.dtype == torch.float32 and g.is_contiguous()
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12)
    assert torch.equal(g.detach(), eye[None, :, None, None, None].expand(4, 12, 8, 16, 16))
    assert BilateralGrids(2, 5, 3, 2).grids.shape == (2, 12, 2, 3, 5)   # (grid_x, grid_y, grid_w) -> [.., L, Hg, Wg]
    rng = np.random.default_rng(3)
    img_np, _ = R.random_images(rng, 9, 7, 8)
    img = torch.from_numpy(img_np)
    for i in range(4):
        assert torch.allclose(grids(img, i), img, rtol=0, atol=1e-6)
    assert float(grids.tv_loss().detach()) == 0.0
    small = BilateralGrids(N_VIEWS, 5, 3, 2).double()
    grids_np = R.random_grids(rng, N_VIEWS, 5, 3, 2)
    with torch.no_grad():
        small.grids.copy_(torch.from_numpy(grids_np))
    img_np, v_np = R.random_images(rng, 11, 13, 2)
    ref = R.slice64(grids_np, img_np, v_np, 1)
    assert np.allclose(small(torch.from_numpy(img_np).double(), 1).detach().numpy(), ref["out"], rtol=1e-13, atol=1e-15)
    assert np.isclose(float(small.tv_loss().detach()), R.tv64(grids_np)[0], rtol=1e-13)
    with pytest.raises(IndexError):
        grids(img, 4)
    with pytest.raises(ValueError):
        grids(torch.zeros(4, 4), 0)
    for bad in ((0, 16, 16, 8), (3, 1, 16, 8), (3, 16, 65, 8), (3, 16, 16, 17), (3, 16, 16, 1), (2 ** 20, 64, 64, 16)):
        with pytest.raises(ValueError):
            BilateralGrids(*bad)
    with pytest.raises(ValueError, match="fused"):
        grids.tv_loss(fused=True)   # (the kernel form needs a device: refused, not replaced)


def test_grids_grad_is_dense_with_exact_zeros_on_every_other_view():
    rng = np.random.default_rng(8)
    grids = BilateralGrids(N_VIEWS, 5, 3, 2).double()
    grids_np = R.random_grids(rng, N_VIEWS, 5, 3, 2)
    with torch.no_grad():
        grids.grids.copy_(torch.from_numpy(grids_np))
    img_np, v_np = R.random_images(rng, 11, 13, 2)
    img = torch.from_numpy(img_np).double().requires_grad_(True)
    (grids(img, 1) * torch.from_numpy(v_np).double()).sum().backward()
    g = grids.grids.grad
    ref = R.slice64(grids_np, img_np, v_np, 1)
    assert g.shape == (N_VIEWS, 12, 2, 3, 5) and not g[0].any() and not g[2].any() and bool(g[1].any())
    assert np.allclose(g.numpy(), ref["v_grids"], rtol=1e-12, atol=1e-300)
    assert np.allclose(img.grad.numpy(), ref["v_c"], rtol=1e-12, atol=1e-300)
    opt = torch.optim.Adam(grids.parameters(), lr=2e-3, eps=1e-15)   # what the dense gradient is for
    before = grids.grids.detach().clone()
    opt.step()
    assert bool((grids.grids.detach()[1] != before[1]).any()) and torch.equal(grids.grids.detach()[0], before[0])


def test_state_dicts_round_trip():
    grids = BilateralGrids(3, 5, 3, 2)
    with torch.no_grad():
        grids.grids.copy_(torch.from_numpy(R.random_grids(np.random.default_rng(2), 3, 5, 3, 2)))
    other = BilateralGrids(3, 5, 3, 2)
    other.load_state_dict(grids.state_dict())
    assert torch.equal(other.grids, grids.grids) and list(grids.state_dict()) == ["grids"]
    st = BilagridAdamState(grids)
    assert st.exp_avg.shape == (3, 12, 2, 3, 5) and st.step == 0 and not st.exp_avg.any() and not st.exp_avg_sq.any()
    st.exp_avg.fill_(0.25); st.exp_avg_sq.fill_(0.5); st.step = 7
    saved = st.state_dict()
    fresh = BilagridAdamState(BilateralGrids(3, 5, 3, 2))
    keep = fresh.exp_avg.data_ptr()
    fresh.load_state_dict(saved)
    assert fresh.step == 7 and torch.equal(fresh.exp_avg, st.exp_avg) and torch.equal(fresh.exp_avg_sq, st.exp_avg_sq)
    assert fresh.exp_avg.data_ptr() == keep   # (in place: a captured step keeps reading the same buffers)
    with pytest.raises(ValueError):
        BilagridAdamState(BilateralGrids(2, 5, 3, 2)).load_state_dict(saved)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_bilagrid_entries():
    for name, params in NEW_ENTRIES.items():
        assert nat.PARAMS[name] == params, name
        assert nat.SIGNATURES[name][0] is (ct.c_size_t if name == "gs_bilagrid_partials_doubles" else ct.c_int)
    L = nat.lib()
    assert L.gs_version() >= 390 and all(hasattr(L, name) for name in NEW_ENTRIES)
    assert nat.GS_BILAGRID_REC_FLOATS == 4
    assert (nat.GS_BILAGRID_REC_SS, nat.GS_BILAGRID_REC_ISBC2, nat.GS_BILAGRID_REC_VIEW) == (0, 1, 2)
    assert (nat.GS_BILAGRID_MAX_XY, nat.GS_BILAGRID_MAX_L) == (64, 16)
    # 48 doubles per (cell, chunk, luminance node); a chunk is 8192 pixels of a cell, 2048 where the launch would have under 1024 blocks
    assert L.gs_bilagrid_partials_doubles(11, 13, 16, 16, 8) == 15 * 15 * 8 * 48
    assert L.gs_bilagrid_partials_doubles(72, 130, 2, 2, 2) == 5 * 2 * 48        # one cell of 9360 pixels (counted as 73 x 131): 5 chunks
    assert L.gs_bilagrid_partials_doubles(1080, 1920, 16, 16, 8) == 15 * 15 * 2 * 8 * 48


def test_the_entries_refuse_bad_arguments_before_any_launch():
    L = nat.lib()
    buf = (ct.c_float * 64)()   # (host memory: every call below returns before it looks at a pointer's target)
    p = (ct.addressof(buf) + 15) & ~15
    ERR = nat.GS_ERR_ARG
    for view, n_views, step in ((-1, 3, 1), (3, 3, 1), (0, 0, 1), (0, nat.GS_BILAGRID_MAX_VIEWS + 1, 1), (0, 3, 0)):
        assert L.gs_bilagrid_step_inputs(None, view, n_views, 2e-3, 0.9, 0.999, step, p) == ERR, (view, n_views, step)
    assert L.gs_bilagrid_step_inputs(None, 0, 3, 2e-3, 0.9, 0.999, 1, p + 4) == ERR   # the record: 16-byte aligned
    good = (3, 16, 16, 8)
    for H, W in ((0, 8), (8, 0), (-1, 8), (8, -1), (30000, 30000)):
        assert L.gs_bilagrid_apply(None, H, W, *good, None, 0, p, p, p + 16) == ERR
        assert L.gs_bilagrid_bwd(None, H, W, *good, None, 0, p, p, p + 16, p, p) == ERR
    assert L.gs_bilagrid_partials_doubles(0, 8, 16, 16, 8) == 0 and L.gs_bilagrid_partials_doubles(8, 8, 1, 16, 8) == 0
    for nv, gx, gy, gl in ((3, 1, 16, 8), (3, 16, 65, 8), (3, 16, 16, 1), (3, 16, 16, 17), (0, 16, 16, 8), (nat.GS_BILAGRID_MAX_VIEWS + 1, 2, 2, 2),
                  (2 ** 16, 64, 64, 16)):   # (the last: 2^16 x 12 x 16 x 64 x 64 = 3 x 2^34 elements)
        assert L.gs_bilagrid_apply(None, 8, 8, nv, gx, gy, gl, None, 0, p, p, p + 16) == ERR, (nv, gx, gy, gl)
        assert L.gs_bilagrid_bwd(None, 8, 8, nv, gx, gy, gl, None, 0, p, p, p + 16, p, p) == ERR, (nv, gx, gy, gl)
        assert L.gs_bilagrid_tv(None, nv, gx, gy, gl, p, 10.0, None, 0, None, None, p, p, p) == ERR, (nv, gx, gy, gl)
    for view in (-1, 3):   # by value (no record): the view must name a grid
        assert L.gs_bilagrid_apply(None, 8, 8, *good, None, view, p, p, p + 16) == ERR
        assert L.gs_bilagrid_bwd(None, 8, 8, *good, None, view, p, p, p + 16, p, p) == ERR
        assert L.gs_bilagrid_tv(None, *good, p, 10.0, None, view, p, None, p, p, p) == ERR
    assert L.gs_bilagrid_apply(None, 8, 8, *good, None, 0, p, p, p) == ERR            # out aliases render
    assert L.gs_bilagrid_apply(None, 8, 8, *good, None, 0, p, p + 4, p + 16) == ERR   # alignment
    assert L.gs_bilagrid_bwd(None, 8, 8, *good, None, 0, p, p, p, p, p) == ERR        # v_image aliases render
    assert L.gs_bilagrid_tv(None, *good, None, 10.0, None, 0, None, None, p, p, p) == ERR   # no grids
    assert L.gs_bilagrid_tv(None, *good, p, 10.0, None, 0, p, None, p, None, p) == ERR      # a slab without v_grids
    for numel in (0, 11, 2 ** 31 + 4):
        assert L.gs_bilagrid_adam(None, numel, p, p, p, p, p, 0.9, 0.999, 1e-15) == ERR, numel
    assert L.gs_bilagrid_adam(None, 24, None, p, p, p, p, 0.9, 0.999, 1e-15) == ERR
    assert b"invalid argument" in L.gs_last_error()


def test_runner_refusals_come_before_any_device_work():
    from easy_gaussian_splatting_amd import train_graph as TG
    from easy_gaussian_splatting_amd.exposure import ExposureTable
    grids = BilateralGrids(3, 5, 3, 2)
    runner = object.__new__(TG.TrainStepGraph)   # (no constructor: it would need a device; `step` validates first)
    runner.poses, runner.exposure, runner.bilagrid = None, None, grids
    frame = ({"w2c": torch.eye(4), "K": torch.eye(3), "width": 8, "height": 8}, torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match="view_index"):
        runner.step(*frame)
    with pytest.raises(ValueError, match="outside the 3 views of `bilagrid`"):
        runner.step(*frame, view_index=3)
    with pytest.raises(ValueError, match="outside the 3 views of `bilagrid`"):
        runner.step(*frame, view_index=-1)
    runner.bilagrid = None
    with pytest.raises(ValueError, match="view_index given"):
        runner.step(*frame, view_index=0)

    class _Model:   # (what the constructor looks at before it touches a device: the device of the means)
        means = torch.zeros(1, 3)
    with pytest.raises(ValueError, match="`exposure` and `bilagrid` together"):
        TG.TrainStepGraph(_Model(), None, None, {}, None, exposure=ExposureTable(3), bilagrid=grids)
    with pytest.raises(ValueError, match="bilagrid"):
        TG.ViewParallelGraphStep(None, None, None, None, None, bilagrid=grids)
    with pytest.raises(TypeError):
        TG.TrainStepGraph(_Model(), None, None, {}, None, bilagrid=torch.zeros(3, 12, 2, 3, 5))
    with pytest.raises(ValueError, match="contiguous float32"):
        TG.TrainStepGraph(_Model(), None, None, {}, None, bilagrid=BilateralGrids(3, 5, 3, 2).double())
    with pytest.raises(ValueError, match="contiguous float32"):
        TG.TrainStepGraph(_Model(), None, None, {}, None, bilagrid=BilateralGrids(3, 5, 3, 2).to("meta"))
