"""Exposure compensation without a GPU: the per-pixel math of the kernels (csrc/gs_exposure.h) built with the host compiler -- the
device's own text -- against fp64 numpy (tests/exposure_ref.py states the bounds), the plain-torch path of `ExposureTable`, the
new entries of the C ABI and the refusals that must come before any device work."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

import adam_ref as A
import exposure_ref as R
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.exposure import ExposureAdamState, ExposureTable

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = {
    "gs_exposure_step_inputs": ["stream", "view", "n_views", "lr", "beta1", "beta2", "step", "rec_dev"],
    "gs_exposure_apply": ["stream", "height", "width", "n_views", "rec_dev", "view", "table", "render", "out"],
    "gs_exposure_partials_doubles": ["height", "width"],
    "gs_exposure_bwd": ["stream", "height", "width", "n_views", "rec_dev", "view", "table", "render", "v_image", "partials", "v_affine12"],
    "gs_exposure_adam": ["stream", "n_views", "rec_dev", "table", "exp_avg", "exp_avg_sq", "v_affine12", "beta1", "beta2", "eps"],
}


@pytest.fixture(scope="module")
def em(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("em") / "libexposuremath.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "exposuremath.cpp")], check=True)
    L = ct.CDLL(so)
    P, F = ct.c_void_p, ct.c_float
    L.em_apply.argtypes, L.em_apply.restype = [P, P, ct.c_int64, P], None
    L.em_vjp.argtypes, L.em_vjp.restype = [P, P, ct.c_int64, P], None
    L.em_sums.argtypes, L.em_sums.restype = [P, P, ct.c_int64, P], None
    L.em_adam.argtypes, L.em_adam.restype = [P, P, P, P, ct.c_int64, F, F, F, F, F], None
    return L


def _ptr(a):
    return a.ctypes.data_as(ct.c_void_p)


@pytest.mark.parametrize("H,W", R.FRAMES[:3])
def test_apply_vjp_and_sums_keep_their_bounds_against_fp64(em, H, W):
    rng = np.random.default_rng(100 * H + W)
    T = np.ascontiguousarray(R.random_table(rng, 1)[0])
    img, v = R.random_images(rng, H, W)
    n = H * W
    out, dv, sums = np.empty_like(img), np.empty_like(v), np.empty((3, 4), dtype=np.float32)
    em.em_apply(_ptr(T), _ptr(img), n, _ptr(out))
    em.em_vjp(_ptr(T), _ptr(v), n, _ptr(dv))
    em.em_sums(_ptr(v), _ptr(img), n, _ptr(sums))
    ratios = {"apply": R.worst_ratio(out, *R.apply64(T, img)), "vjp": R.worst_ratio(dv, *R.vjp64(T, v)),
              "sums": R.worst_ratio(sums, *R.sums64(v, img))}
    print(f"{H}x{W}: worst |error| / bound {ratios}")
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_apply_at_the_identity_returns_its_input_bit_for_bit(em):
    rng = np.random.default_rng(5)
    T = np.ascontiguousarray(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32))
    img, _ = R.random_images(rng, 37, 53)
    img[0, 0] = [np.float32(1e-42), np.float32(-3e38), np.float32(1.0)]   # a subnormal, a huge value
    out = np.empty_like(img)
    em.em_apply(_ptr(T), _ptr(img), 37 * 53, _ptr(out))
    assert np.array_equal(out.view(np.uint32), img.view(np.uint32))
    zero = np.array([[-0.0, 0.0, -0.0]], dtype=np.float32)   # (a -0 comes back as a zero: +0, the sum of -0 and b = +0)
    em.em_apply(_ptr(T), _ptr(zero), 1, _ptr(out))
    assert not out.reshape(-1)[:3].any()


def test_adam_element_keeps_the_bounds_of_the_fused_adam_kernels(em):
    p, g, m, v = A.regime_inputs(4096, seed=12)
    lr, t, b1, b2, eps = 1e-2, 7, 0.9, 0.999, 1e-15
    bc1, bc2 = 1.0 - float(np.float32(b1)) ** t, 1.0 - float(np.float32(b2)) ** t
    ss, isbc2 = np.float32(float(np.float32(lr)) / bc1), np.float32(1.0 / np.sqrt(bc2))
    p1, m1, v1 = p.copy(), m.copy(), v.copy()
    em.em_adam(_ptr(p1), _ptr(g), _ptr(m1), _ptr(v1), p.size, b1, b2, eps, isbc2, ss)
    ratios = A.error_ratios((p1, m1, v1), p, A.adam_ref(p, g, m, v, lr, t, b1, b2, eps))
    print(f"exposure_adam1: error / bound {ratios}")
    assert ratios["p"] <= 1.0 and ratios["m"] <= 1.0 and ratios["v"] <= 1.0, ratios
    pe, me, ve = A.adam1_emulated(p, g, m, v, lr, t, b1, b2, eps)   # ... and it is adam1() of the library, contraction for contraction
    same = lambda x, y: float(np.mean(x.view(np.uint32) == y.view(np.uint32)))   # noqa: E731
    assert min(same(p1, pe), same(m1, me), same(v1, ve)) > 0.999   # (the emulation's double rounding: one case in 2^29)


# ---- the plain-torch path of ExposureTable: the semantic reference ----------------------------------------------------------------
def test_table_is_the_identity_at_init_and_the_affine_expression_afterwards():
    g = torch.Generator().manual_seed(3)
    table = ExposureTable(4)
    assert table.affine.shape == (4, 3, 4) and table.affine.dtype == torch.float32 and table.affine.is_contiguous()
    assert torch.equal(table.affine.detach(), torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).expand(4, 3, 4))
    img = torch.rand((9, 7, 3), generator=g) * 1.4 - 0.2
    for i in range(4):
        assert torch.equal(table(img, i), img)
    with torch.no_grad():
        table.affine.copy_(torch.from_numpy(R.random_table(np.random.default_rng(1), 4)))
    for dtype in (torch.float32, torch.float64):
        t = table.to(dtype)
        x = img.to(dtype)
        a = t.affine.detach()
        assert torch.equal(t(x, 2), x @ a[2, :, :3].T + a[2, :, 3])
    with pytest.raises(IndexError):
        table(img, 4)


def test_affine_grad_is_dense_with_exact_zeros_on_every_other_row():
    rng = np.random.default_rng(8)
    table = ExposureTable(3).double()
    with torch.no_grad():
        table.affine.copy_(torch.from_numpy(R.random_table(rng, 3)))
    img_np, v_np = R.random_images(rng, 11, 13)
    img = torch.from_numpy(img_np).double().requires_grad_(True)
    (table(img, 1) * torch.from_numpy(v_np).double()).sum().backward()
    g = table.affine.grad
    assert g.shape == (3, 3, 4) and not g[0].any() and not g[2].any() and bool(g[1].all())
    ref, _ = R.sums64(v_np, img_np)
    assert np.allclose(g[1].numpy(), ref, rtol=1e-12, atol=0)
    assert np.allclose(img.grad.numpy(), R.vjp64(table.affine.detach()[1].numpy(), v_np)[0], rtol=1e-12, atol=1e-300)
    opt = torch.optim.Adam(table.parameters(), lr=1e-2)   # what the dense gradient is for
    before = table.affine.detach().clone()
    opt.step()
    assert bool((table.affine.detach()[1] != before[1]).all()) and torch.equal(table.affine.detach()[0], before[0])


def test_state_dicts_round_trip():
    table = ExposureTable(3)
    with torch.no_grad():
        table.affine.copy_(torch.from_numpy(R.random_table(np.random.default_rng(2), 3)))
    other = ExposureTable(3)
    other.load_state_dict(table.state_dict())
    assert torch.equal(other.affine, table.affine) and list(table.state_dict()) == ["affine"]
    st = ExposureAdamState(table)
    assert st.exp_avg.shape == (3, 3, 4) and st.step == 0 and not st.exp_avg.any() and not st.exp_avg_sq.any()
    st.exp_avg.fill_(0.25); st.exp_avg_sq.fill_(0.5); st.step = 7
    saved = st.state_dict()
    fresh = ExposureAdamState(ExposureTable(3))
    keep = fresh.exp_avg.data_ptr()
    fresh.load_state_dict(saved)
    assert fresh.step == 7 and torch.equal(fresh.exp_avg, st.exp_avg) and torch.equal(fresh.exp_avg_sq, st.exp_avg_sq)
    assert fresh.exp_avg.data_ptr() == keep   # (in place: a captured step keeps reading the same buffers)
    with pytest.raises(ValueError):
        ExposureAdamState(ExposureTable(2)).load_state_dict(saved)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_exposure_entries():
    for name, params in NEW_ENTRIES.items():
        assert nat.PARAMS[name] == params, name
        assert nat.SIGNATURES[name][0] is (ct.c_size_t if name == "gs_exposure_partials_doubles" else ct.c_int)
    L = nat.lib()
    assert L.gs_version() >= 380 and all(hasattr(L, name) for name in NEW_ENTRIES)
    assert nat.GS_EXPOSURE_REC_FLOATS == 4
    assert (nat.GS_EXPOSURE_REC_SS, nat.GS_EXPOSURE_REC_ISBC2, nat.GS_EXPOSURE_REC_VIEW) == (0, 1, 2)
    # a multiple of 12 doubles per block, one block up to 1024 pixels, capped: a 1080p frame strides
    assert L.gs_exposure_partials_doubles(11, 11) == 12 and L.gs_exposure_partials_doubles(208, 320) == 12 * 65
    assert L.gs_exposure_partials_doubles(1080, 1920) == L.gs_exposure_partials_doubles(4320, 7680) == 12 * 1024


def test_the_entries_refuse_bad_arguments_before_any_launch():
    L = nat.lib()
    buf = (ct.c_float * 64)()   # (host memory, 16-byte aligned or not: every call below returns before it looks at a pointer's target)
    p = ct.addressof(buf) & ~15
    ERR = nat.GS_ERR_ARG
    for view, n_views, step in ((-1, 3, 1), (3, 3, 1), (0, 0, 1), (0, nat.GS_EXPOSURE_MAX_VIEWS + 1, 1), (0, 3, 0)):
        assert L.gs_exposure_step_inputs(None, view, n_views, 1e-2, 0.9, 0.999, step, p) == ERR, (view, n_views, step)
    for H, W in ((0, 8), (8, 0), (-1, 8), (8, -1)):
        assert L.gs_exposure_apply(None, H, W, 3, None, 0, p, p, p) == ERR
        assert L.gs_exposure_bwd(None, H, W, 3, None, 0, p, p, p, p, p) == ERR
        assert L.gs_exposure_partials_doubles(H, W) == 0
    for view, n_views in ((-1, 3), (3, 3), (0, 0)):   # by value (no record): the view must name a row
        assert L.gs_exposure_apply(None, 8, 8, n_views, None, view, p, p, p) == ERR
        assert L.gs_exposure_bwd(None, 8, 8, n_views, None, view, p, p, p, p, p) == ERR
    assert L.gs_exposure_adam(None, 0, p, p, p, p, p, 0.9, 0.999, 1e-15) == ERR
    assert b"invalid argument" in L.gs_last_error()


def test_runner_refusals_come_before_any_device_work():
    from easy_gaussian_splatting_amd import train_graph as TG
    table = ExposureTable(3)
    runner = object.__new__(TG.TrainStepGraph)   # (no constructor: it would need a device; `step` validates first)
    runner.poses, runner.exposure = None, table
    frame = ({"w2c": torch.eye(4), "K": torch.eye(3), "width": 8, "height": 8}, torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match="view_index"):
        runner.step(*frame)
    with pytest.raises(ValueError, match="outside the 3 views of `exposure`"):
        runner.step(*frame, view_index=3)
    from easy_gaussian_splatting_amd.pose import CameraDeltas
    runner.poses = CameraDeltas(2)   # one index for both tables: it must name a row of each
    with pytest.raises(ValueError, match="outside the 2 views of `poses`"):
        runner.step(*frame, view_index=2)
    with pytest.raises(ValueError, match="exposure"):
        TG.ViewParallelGraphStep(None, None, None, None, None, exposure=table)
    with pytest.raises(TypeError):
        TG.TrainStepGraph(None, None, None, None, None, exposure=torch.zeros(3, 3, 4))
