"""The pose math of the captured step (csrc/gs_pose.h) built with the host compiler -- the device's own text -- against
`pose.CameraDeltas` in float64 (tests/pose_ref.py): the composed view matrix to one fp32 ulp, the chain from the view matrix'
gradient to the 6-vector to 1e-9 (both sides fp64: only the series cut-over can show), the new entries of the C ABI, and the
refusals that must come before any device work."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

import pose_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = {
    "gs_pose_step_inputs": ["stream", "view", "n_views", "w2c_dev", "w2c_host", "lr", "beta1", "beta2", "step", "rec_dev"],
    "gs_pose_compose": ["stream", "n_views", "rec_dev", "deltas", "viewmat_out"],
    "gs_cam_grad_sums": ["stream", "N", "K", "sh_degree", "means", "quats", "scales", "sh_rest", "viewmats", "Ks", "width", "height", "eps2d",
                         "near_plane", "far_plane", "radii", "colors_post", "activations", "sh_jac", "row_sums", "cam_partials", "v_viewmats",
                         "v_campos"],
    "gs_project_bwd_adam_sums": ["stream", "N", "K", "sh_degree", "params", "exp_avg", "exp_avg_sq", "offsets_host", "viewmats", "Ks", "width",
                                 "height", "eps2d", "near_plane", "far_plane", "radii", "colors_post", "tiles_per_gauss", "cum_tiles", "row_sums",
                                 "v_means2d_abs", "beta1", "beta2", "eps", "hyper_dev", "applied_dev", "max_radii", "grad_norm_accum", "counts",
                                 "sh_jac", "scale_reg", "max_ratio", "lambda", "budget", "a", "b"],
    "gs_pose_adam": ["stream", "n_views", "rec_dev", "deltas", "exp_avg", "exp_avg_sq", "v_viewmats", "v_campos", "v_delta", "beta1", "beta2",
                     "eps"],
}


@pytest.fixture(scope="module")
def pm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pm") / "libposemath.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "posemath.cpp")], check=True)
    L = ct.CDLL(so)
    P = ct.c_void_p
    L.pm_compose.argtypes, L.pm_compose.restype = [P, P, P], None
    L.pm_vjp.argtypes, L.pm_vjp.restype = [P, P, P, P, P, P], None
    L.pm_coeffs.argtypes, L.pm_coeffs.restype = [ct.c_double, P], None
    return L


def _ptr(a):
    return a.ctypes.data_as(ct.c_void_p)


def compose(L, delta32, w2c32):
    out = np.empty(16, dtype=np.float32)
    L.pm_compose(_ptr(delta32), _ptr(w2c32), _ptr(out))
    return out.reshape(4, 4)


def vjp(L, delta, w2c, v_A, v_t, v_campos):
    args = [np.ascontiguousarray(x, dtype=np.float64) for x in (delta, w2c, v_A, v_t, v_campos)]
    out = np.empty(6, dtype=np.float64)
    L.pm_vjp(*[_ptr(x) for x in args], _ptr(out))
    return out


@pytest.mark.parametrize("theta", R.THETAS)
def test_compose_is_camera_deltas_forward_to_one_fp32_ulp(pm, theta):
    rng = np.random.default_rng(int(theta * 1e6) % 1000 + 3)
    worst = 0.0
    for _ in range(8):
        delta = R.delta_at(rng, theta).astype(np.float32)
        w2c = np.ascontiguousarray(R.random_rigid(rng).astype(np.float32))
        got = compose(pm, delta, w2c.reshape(-1)).astype(np.float64)
        ref = R.compose64(delta, w2c).numpy()
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        bound = np.maximum(ulp, 2.0 ** -24 * np.abs(ref).max(axis=1, keepdims=True))   # (entries that cancel: their row's scale)
        worst = max(worst, float((np.abs(got - ref) / bound).max()))
    print(f"theta = {theta}: worst |error| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_compose_of_zero_delta_is_w2c_bit_for_bit(pm):
    rng = np.random.default_rng(11)
    for _ in range(8):
        w2c = np.ascontiguousarray(R.random_rigid(rng).astype(np.float32)).reshape(-1)
        w2c[rng.integers(0, 12)] = -0.0   # (a product with the identity would hand back +0)
        got = compose(pm, np.zeros(6, dtype=np.float32), w2c)
        assert got.reshape(-1).view(np.uint32).tolist() == w2c.view(np.uint32).tolist()


@pytest.mark.parametrize("scale", [1.0, 1.01], ids=["rigid", "scaled_1.01"])
@pytest.mark.parametrize("theta", R.THETAS)
def test_vjp_is_float64_autograd_of_camera_deltas(pm, theta, scale):
    rng = np.random.default_rng(int(theta * 1e6) % 1000 + 29)
    worst = 0.0
    for _ in range(8):
        delta = R.delta_at(rng, theta)
        w2c = R.random_rigid(rng)
        w2c[:3, :3] *= scale   # (non-orthonormal: a transposed inverse or an assumed R^T shows here)
        G, g = rng.standard_normal((3, 4)), rng.standard_normal(3)
        got = vjp(pm, delta, w2c.reshape(-1), G[:, :3], G[:, 3], g)
        ref = R.vjp64(delta, w2c, G, g)
        worst = max(worst, float(np.abs(got - ref).max() / (1e-9 * np.abs(ref).max())))
    print(f"theta = {theta}, scale = {scale}: worst |error| / (1e-9 max|v_delta|) = {worst:.3e}")
    assert worst <= 1.0


def test_coefficients_are_continuous_across_the_series_cut_over(pm):
    abc = np.empty((2, 3))
    for row, t2 in enumerate((1e-2 * (1 - 1e-12), 1e-2 * (1 + 1e-12))):
        pm.pm_coeffs(t2, _ptr(abc[row]))
    assert np.abs(abc[0] - abc[1]).max() <= 1e-13
    th = 0.1
    assert np.allclose(abc[1], [np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3], rtol=1e-10, atol=0)


def test_header_declares_the_pose_entries():
    from easy_gaussian_splatting_amd import _native as nat
    for name, params in NEW_ENTRIES.items():
        assert nat.PARAMS[name] == params, name
        assert nat.SIGNATURES[name][0] is ct.c_int
    if os.path.exists(nat.LIB_PATH):   # (a built tree: the library is this ABI's)
        L = nat.lib()
        assert L.gs_version() >= 370 and all(hasattr(L, name) for name in NEW_ENTRIES)
    assert nat.GS_POSE_REC_FLOATS == 20 and (nat.GS_POSE_REC_SS, nat.GS_POSE_REC_ISBC2, nat.GS_POSE_REC_VIEW) == (16, 17, 18)


def test_pose_adam_state_round_trips():
    from easy_gaussian_splatting_amd.pose import CameraDeltas, PoseAdamState
    st = PoseAdamState(CameraDeltas(3))
    st.exp_avg.fill_(0.25); st.exp_avg_sq.fill_(0.5); st.step = 7
    saved = st.state_dict()
    other = PoseAdamState(CameraDeltas(3))
    keep = other.exp_avg.data_ptr()
    other.load_state_dict(saved)
    assert other.step == 7 and torch.equal(other.exp_avg, st.exp_avg) and torch.equal(other.exp_avg_sq, st.exp_avg_sq)
    assert other.exp_avg.data_ptr() == keep   # (in place: a captured step keeps reading the same buffers)
    with pytest.raises(ValueError):
        PoseAdamState(CameraDeltas(2)).load_state_dict(saved)


def test_refusals_come_before_any_device_work():
    from easy_gaussian_splatting_amd import train_graph as TG
    from easy_gaussian_splatting_amd.distributed import ViewParallelStep
    from easy_gaussian_splatting_amd.pose import CameraDeltas
    poses = CameraDeltas(3)
    runner = object.__new__(TG.TrainStepGraph)   # (no constructor: it would need a device; `step` validates first)
    runner.poses = poses
    with pytest.raises(ValueError, match="view_index"):
        runner.step({"w2c": torch.eye(4), "K": torch.eye(3), "width": 8, "height": 8}, torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match="outside"):
        runner.step({"w2c": torch.eye(4), "K": torch.eye(3), "width": 8, "height": 8}, torch.zeros(8, 8, 3), view_index=3)
    runner.poses = None
    with pytest.raises(ValueError, match="without `poses`"):
        runner.step({"w2c": torch.eye(4), "K": torch.eye(3), "width": 8, "height": 8}, torch.zeros(8, 8, 3), view_index=0)
    # a w2c that requires grad is still refused, with or without poses, and the message names the captured recipe
    runner.poses = poses
    with pytest.raises(ValueError, match="poses=pose.CameraDeltas"):
        runner.step({"w2c": torch.eye(4, requires_grad=True), "K": torch.eye(3), "width": 8, "height": 8}, torch.zeros(8, 8, 3), view_index=0)
    with pytest.raises(ValueError, match="poses"):
        TG.ViewParallelGraphStep(None, None, None, None, None, poses=poses)
    with pytest.raises(ValueError, match="poses"):
        ViewParallelStep(None, None, poses=poses)
