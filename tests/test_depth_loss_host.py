"""Depth supervision without a GPU: the per-pixel math of the kernels (csrc/gs_depth_loss.h) built with the host compiler -- the
device's own text -- against fp64 numpy (tests/depth_loss_ref.py states the bounds), the plain-torch path of `depth_loss`, the new
entries of the C ABI and the refusals that must come before any device work."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

import depth_loss_ref as R
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.depth_loss import DepthSupervision, depth_loss

HERE = os.path.dirname(os.path.abspath(__file__))
_BWD_ADAM = ["stream", "N", "K", "sh_degree", "params", "exp_avg", "exp_avg_sq", "offsets_host", "viewmats", "Ks", "width", "height", "eps2d",
             "near_plane", "far_plane", "radii", "colors_post", "tiles_per_gauss", "cum_tiles", "rows", "row_base", "qmask", "v_means2d_abs",
             "beta1", "beta2", "eps", "hyper_dev", "applied_dev", "max_radii", "grad_norm_accum", "counts", "sh_jac"]
NEW_ENTRIES = {
    "gs_depth_step_inputs": ["stream", "lambda_depth", "mode", "target", "rec_dev"],
    "gs_depth_loss_partials_doubles": ["height", "width"],
    "gs_depth_loss_split": ["stream", "height", "width", "rec_dev", "lambda_depth", "mode", "target", "mask", "img_slots", "colors4", "alphas",
                            "image3", "depth", "partials"],
    "gs_depth_loss_finish": ["stream", "height", "width", "rec_dev", "lambda_depth", "staged", "partials", "loss3"],
    "gs_depth_loss_fwd": ["stream", "height", "width", "rec_dev", "mode", "target", "mask", "depth", "partials"],
    "gs_depth_loss_join": ["stream", "height", "width", "rec_dev", "lambda_depth", "mode", "target", "mask", "img_slots", "colors4", "alphas",
                           "depth", "v_render", "v_colors4", "v_alphas"],
    "gs_depth_loss_bwd": ["stream", "height", "width", "rec_dev", "mode", "target", "mask", "depth", "v_loss", "v_depth"],
    "gs_depth_grads_z": ["stream", "C", "N", "lane", "radii", "tiles_per_gauss", "cum_tiles", "rows", "row_base", "qmask", "v_depths"],
    "gs_project_bwd_adam_depth": _BWD_ADAM + ["scale_reg", "max_ratio", "lambda", "budget", "a", "b", "v_depths"],
}


@pytest.fixture(scope="module")
def dl(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dl") / "libdepthlossmath.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "depthlossmath.cpp")], check=True)
    L = ct.CDLL(so)
    P = ct.c_void_p
    L.dl_value.argtypes, L.dl_value.restype = [ct.c_int, P, P, P, ct.c_int64, P], None
    L.dl_grad.argtypes, L.dl_grad.restype = [ct.c_int, P, P, P, ct.c_int64, ct.c_float, P], None
    L.dl_valid.argtypes, L.dl_valid.restype = [P, ct.c_int64, P], None
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ct.c_void_p)


def _host(dl, mode, d, t, m, upstream=1.0):
    """(value, 1 / sum(w), gradient) of the header on the host, the gradient scaled as the kernels scale it: fl(upstream * inv_w)."""
    d, t = np.ascontiguousarray(d), np.ascontiguousarray(t)
    m = None if m is None else np.ascontiguousarray(m)
    out, g = np.empty(2, dtype=np.float32), np.empty_like(d)
    dl.dl_value(R.MODES.index(mode), _ptr(d), _ptr(t), _ptr(m), d.size, _ptr(out))
    dl.dl_grad(R.MODES.index(mode), _ptr(d), _ptr(t), _ptr(m), d.size, float(np.float32(upstream) * out[1]), _ptr(g))
    return out[0], out[1], g


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("H,W", R.HOST_FRAMES)
def test_value_and_gradient_keep_their_bounds_against_fp64(dl, H, W, mode, mask):
    rng = np.random.default_rng(100 * H + W + (7 if mask else 0))
    d, t, m = R.make_case(rng, H, W, mask)
    value, inv_w, g = _host(dl, mode, d, t, m, upstream=0.37)
    ref, bound = R.value64(d, t, m, mode)
    gref, gbound = R.grad64(d, t, m, mode, upstream=0.37)
    ratios = {"value": abs(float(value) - ref) / bound, "grad": R.worst_ratio(g, gref, gbound)}
    print(f"{H}x{W} {mode} mask={mask}: value {value} (ref {ref}), worst |error| / bound {ratios}")
    assert ref > 0 and np.isfinite(g).all()
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert bool(np.any(gref != 0)) and not g[gref == 0].any()   # exact zeros stay exact zeros: holes, masked pixels, e == 0


def test_validity_is_positive_and_finite(dl):
    t = np.array([1.0, 1e-45, 3.4028235e38, 0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    valid = np.empty(t.size, dtype=np.int32)
    dl.dl_valid(_ptr(t), t.size, _ptr(valid))
    assert valid.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("mode", R.MODES)
def test_a_frame_without_a_measurement_gives_zeros_never_a_nan(dl, mode):
    rng = np.random.default_rng(3)
    d, _, m = R.make_case(rng, 11, 13)
    for t in (np.zeros_like(d), np.full_like(d, np.nan), np.full_like(d, -2.0), np.full_like(d, np.inf)):
        value, inv_w, g = _host(dl, mode, d, t, m)
        assert value == 0.0 and inv_w == 0.0 and not g.any() and np.isfinite(g).all()
    _, t, _ = R.make_case(rng, 11, 13)
    value, inv_w, g = _host(dl, mode, d, t, np.ones_like(d))   # every pixel masked out: sum(w) == 0 as well
    assert value == 0.0 and inv_w == 0.0 and not g.any()


@pytest.mark.parametrize("mode", R.MODES)
def test_nan_and_inf_target_pixels_are_ignored(dl, mode):
    rng = np.random.default_rng(4)
    d = rng.uniform(0.5, 8.0, (11, 11)).astype(np.float32)
    t = (d * 1.1).astype(np.float32)
    t_holes = t.copy()
    holes = rng.random(t.shape) < 0.3
    t_holes[holes] = np.where(rng.random(int(holes.sum())) < 0.5, np.nan, np.inf).astype(np.float32)
    v0, _, g0 = _host(dl, mode, d[~holes], t[~holes], None)   # the frame without those pixels
    v1, _, g1 = _host(dl, mode, d, t_holes, None)
    assert v0 == v1 and np.array_equal(g1[~holes], g0) and not g1[holes].any()


def test_zero_error_has_zero_gradient_and_zero_depth_counts_in_the_value_only(dl):
    d = np.array([2.0, 3.0, 0.0, -1.0, 4.0], dtype=np.float32)
    t = np.array([2.0, 2.0, 2.0, 2.0, 0.0], dtype=np.float32)
    # depth: e = {0, 1, -2, -3, -}: sign(0) = 0
    value, inv_w, g = _host(dl, "depth", d, t, None)
    assert value == np.float32(6.0 / 4.0) and inv_w == np.float32(0.25)
    assert g.tolist() == [0.0, 0.25, -0.25, -0.25, 0.0]
    # disparity: e = {0, 1/3 - 1/2, 0 - 1/2, 0 - 1/2, -}: d <= 0 counts in the value, with no gradient
    value, inv_w, g = _host(dl, "disparity", d, t, None)
    e1 = abs(float(np.float32(1.0) / np.float32(3.0) - np.float32(0.5)))
    assert value == np.float32((e1 + 0.5 + 0.5) / 4.0)
    assert g[0] == 0.0 and g[2] == 0.0 and g[3] == 0.0 and g[4] == 0.0
    assert g[1] == np.float32(-(np.float32(-0.25) / np.float32(3.0)) / np.float32(3.0)) and g[1] > 0   # e < 0, -1 / d^2 < 0


# ---- the plain-torch path: the semantic reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
def test_plain_torch_path_is_the_formula(mode, mask):
    rng = np.random.default_rng(21)
    d_np, t_np, m_np = R.make_case(rng, 37, 53, mask)
    d = torch.from_numpy(d_np).double().reshape(37, 53, 1).requires_grad_(True)   # [H, W, 1], as the model returns it
    m = None if m_np is None else torch.from_numpy(m_np).double()
    loss = depth_loss(d, torch.from_numpy(t_np).double(), m, mode=mode, fused=False)
    assert loss.dim() == 0 and loss.dtype == torch.float64
    (0.37 * loss).backward()
    ref, _ = R.value64(d_np, t_np, m_np, mode)
    gref, _ = R.grad64(d_np, t_np, m_np, mode, upstream=0.37)
    assert abs(float(loss.detach()) - ref) <= 1e-12 * ref
    g = d.grad.numpy().reshape(37, 53)
    assert np.isfinite(g).all() and np.allclose(g, gref, rtol=1e-12, atol=1e-300) and not g[gref == 0].any()
    # [H, W] and float32 inputs take the same path; a frame without a measurement is an exact zero with a zero gradient
    d32 = torch.from_numpy(d_np).requires_grad_(True)
    l32 = depth_loss(d32, torch.from_numpy(t_np), None if m_np is None else torch.from_numpy(m_np), mode=mode, fused=False)
    assert l32.dtype == torch.float32 and abs(float(l32.detach()) - ref) <= 1e-5 * ref
    d0 = torch.from_numpy(d_np).requires_grad_(True)
    l0 = depth_loss(d0, torch.zeros(37, 53), None, mode=mode, fused=False)
    l0.backward()
    assert float(l0) == 0.0 and not d0.grad.any() and bool(torch.isfinite(d0.grad).all())


def test_settings_object_and_the_eager_refusals():
    s = DepthSupervision(lambda_depth=0.5, mode="depth")
    assert (s.lambda_depth, s.mode) == (0.5, "depth") and DepthSupervision().mode == "disparity"
    for bad in (dict(mode="inverse"), dict(lambda_depth=-1.0), dict(lambda_depth=float("nan"))):
        with pytest.raises(ValueError):
            DepthSupervision(**bad)
    d, t = torch.ones(8, 6, 1), torch.ones(8, 6)
    for fused in (False, True):   # (shapes and modes are refused before the device is looked at)
        with pytest.raises(ValueError, match="gt_depth of shape"):
            depth_loss(d, torch.ones(6, 8), fused=fused)
        with pytest.raises(ValueError, match="mask of shape"):
            depth_loss(d, t, torch.ones(8, 7), fused=fused)
        with pytest.raises(ValueError, match="render_depth of shape"):
            depth_loss(torch.ones(8, 6, 3), t, fused=fused)
        with pytest.raises(ValueError, match="mode"):
            depth_loss(d, t, mode="log", fused=fused)
    with pytest.raises(ValueError, match="HIP device"):
        depth_loss(d, t, fused=True)   # host tensors: the kernels are HIP only, and nothing falls back
    with pytest.raises(ValueError, match="float32"):
        depth_loss(d.double(), t, fused=True)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_depth_supervision_entries():
    for name, params in NEW_ENTRIES.items():
        assert nat.PARAMS[name] == params, name
        assert nat.SIGNATURES[name][0] is (ct.c_size_t if name == "gs_depth_loss_partials_doubles" else ct.c_int)
    L = nat.lib()
    assert L.gs_version() >= 400 and all(hasattr(L, name) for name in NEW_ENTRIES)
    assert (nat.GS_DEPTH_MODE_DEPTH, nat.GS_DEPTH_MODE_DISPARITY) == (0, 1)
    assert nat.GS_DEPTH_REC_FLOATS == 8
    assert (nat.GS_DEPTH_REC_LAMBDA, nat.GS_DEPTH_REC_MODE, nat.GS_DEPTH_REC_TARGET, nat.GS_DEPTH_REC_VALUE, nat.GS_DEPTH_REC_INV_W) == (0, 1, 2, 4, 5)
    # the existing fused entries keep their parameter lists: the depth gradient comes through an entry of its own
    assert nat.PARAMS["gs_project_bwd_adam"] == _BWD_ADAM and nat.PARAMS["gs_project_bwd_adam_mcmc"][-5:] == ["scale_reg", "max_ratio", "lambda", "a", "b"]
    # two doubles per block, one block up to 1024 pixels, capped: a 1080p frame strides
    assert L.gs_depth_loss_partials_doubles(11, 11) == 2 and L.gs_depth_loss_partials_doubles(208, 320) == 2 * 65
    assert L.gs_depth_loss_partials_doubles(1080, 1920) == L.gs_depth_loss_partials_doubles(4320, 7680) == 2 * 1024


def test_the_entries_refuse_bad_arguments_before_any_launch():
    L = nat.lib()
    buf = (ct.c_float * 64)()   # (host memory: every call below returns before it looks at a pointer's target)
    p = (ct.addressof(buf) + 15) & ~15
    ERR = nat.GS_ERR_ARG
    for lam, mode, target, rec in ((float("nan"), 0, p, p), (1.0, 2, p, p), (1.0, -1, p, p), (1.0, 0, None, p), (1.0, 0, p + 4, p), (1.0, 0, p, None),
                                   (1.0, 0, p, p + 8)):
        assert L.gs_depth_step_inputs(None, lam, mode, target, rec) == ERR, (lam, mode, target, rec)
    for H, W in ((0, 8), (8, 0), (-1, 8), (8, -1)):
        assert L.gs_depth_loss_split(None, H, W, p, 1.0, 0, p, None, None, p + 64, p, p + 128, p + 192, p) == ERR
        assert L.gs_depth_loss_finish(None, H, W, p, 1.0, 0, p, None) == ERR
        assert L.gs_depth_loss_fwd(None, H, W, p, 0, p, None, p, p) == ERR
        assert L.gs_depth_loss_join(None, H, W, p, 1.0, 0, p, None, None, p, p, p, p, p + 64, p + 128) == ERR
        assert L.gs_depth_loss_bwd(None, H, W, p, 0, p, None, p, p, p + 64) == ERR
        assert L.gs_depth_loss_partials_doubles(H, W) == 0
    assert L.gs_depth_loss_fwd(None, 8, 8, p, 2, p, None, p, p) == ERR             # an unknown mode, by value
    assert L.gs_depth_loss_fwd(None, 8, 8, p, 0, None, None, p, p) == ERR          # the eager form has no record to read a target from
    assert L.gs_depth_loss_fwd(None, 8, 8, p, 0, p + 4, None, p, p) == ERR         # a misaligned target
    assert L.gs_depth_loss_fwd(None, 8, 8, None, 0, p, None, p, p) == ERR          # no record
    assert L.gs_depth_loss_split(None, 8, 8, p, 1.0, 0, p, None, None, p + 64, p, p + 64, p + 192, p) == ERR   # image3 aliases colors4
    assert L.gs_depth_loss_join(None, 8, 8, p, 1.0, 0, p, None, None, p, p + 16, p + 32, p + 64, p + 64, p + 128) == ERR   # v_colors4 aliases v_render
    assert L.gs_depth_loss_finish(None, 8, 8, p, 1.0, 2, p, None) == ERR
    assert L.gs_depth_grads_z(None, 1, 8, 4, p, p, p, p, p, p, p) == ERR           # lane outside 0..3
    assert L.gs_depth_grads_z(None, 1, 8, 3, p, p, p, p, p, p, None) == ERR        # no output
    assert b"invalid argument" in L.gs_last_error()


def test_runner_refusals_come_before_any_device_work():
    from easy_gaussian_splatting_amd import train_graph as TG
    from easy_gaussian_splatting_amd.pose import CameraDeltas
    sup = DepthSupervision(0.1, "disparity")
    data = {"w2c": torch.eye(4), "K": torch.eye(3), "width": 8, "height": 6}
    with pytest.raises(TypeError):
        TG.TrainStepGraph(None, None, None, data, None, depth=0.1)
    with pytest.raises(ValueError, match="poses"):
        TG.TrainStepGraph(None, None, None, data, None, depth=sup, gt_depth=torch.ones(6, 8), poses=CameraDeltas(2))
    with pytest.raises(ValueError, match="rounds='on'"):
        TG.TrainStepGraph(None, None, None, data, None, depth=sup, gt_depth=torch.ones(6, 8), rounds="on")
    with pytest.raises(ValueError, match="gt_depth"):
        TG.TrainStepGraph(None, None, None, data, None, depth=sup)
    with pytest.raises(ValueError, match="gt_depth of shape"):
        TG.TrainStepGraph(None, None, None, data, None, depth=sup, gt_depth=torch.ones(8, 6))
    with pytest.raises(ValueError, match="depth"):
        TG.ViewParallelGraphStep(None, None, None, data, None, depth=sup, gt_depth=torch.ones(6, 8))
    runner = object.__new__(TG.TrainStepGraph)   # (no constructor: it would need a device)
    runner.depth = sup
    with pytest.raises(NotImplementedError, match="depth"):
        TG.HostFeed(runner)
    runner.depth, runner.poses, runner.exposure = None, None, None
    with pytest.raises(ValueError, match="without `depth`"):   # a target handed to a runner that supervises no depth
        runner.step(data, torch.zeros(6, 8, 3), gt_depth=torch.ones(6, 8))
