"""Depth render modes ("D", "ED", "RGB+D", "RGB+ED"), host side: what the front end admits and refuses, the argument checks of the
new entry points (gs_rec_depth, gs_depth_grads, gs_expected_depth_fwd / _bwd) and their arithmetic -- the depth_* / expected_depth*
functions of gs_math.h compiled for the host (tests/hostmath/depthmath.cpp) against fp64 torch autograd.  Nothing here launches a
kernel."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

import cameras
import depth_ref as DR

HM = os.path.join(os.path.dirname(__file__), "hostmath")
GRAD_RTOL = 1e-3   # the project's gradient contract (tests/test_camgrad_host.py)


def _args(N=4, C=1, **over):
    a = dict(means=torch.zeros(N, 3), quats=torch.ones(N, 4), scales=torch.ones(N, 3), opacities=torch.ones(N),
             colors=torch.zeros(N, 16, 3), viewmats=torch.eye(4)[None].repeat(C, 1, 1), Ks=torch.eye(3)[None].repeat(C, 1, 1), width=32,
             height=32, sh_degree=3, packed=False)
    a.update(over)
    return a


@pytest.mark.parametrize("mode", DR.MODES)
def test_the_four_modes_pass_the_argument_checks_and_end_in_the_gpu_only_refusal(mode):
    from easy_gaussian_splatting_amd.rendering import rasterization
    forms = [_args(), _args(backgrounds=torch.zeros(1, 3)), _args(colors=(torch.zeros(4, 1, 3), torch.zeros(4, 15, 3))),
             _args(colors=torch.zeros(4, 25, 3), sh_degree=4), _args(colors=torch.zeros(4, 3), sh_degree=None),
             _args(C=2, colors=torch.zeros(2, 4, 1), sh_degree=None, backgrounds=torch.zeros(2, 1)),
             _args(_activations="exp_sigmoid", absgrad=True, _tile_culling="tight"), _args(_camera_grads=True)]
    for a in forms:
        with pytest.raises(NotImplementedError, match="GPU only") as e:
            rasterization(**a, render_mode=mode)
        assert isinstance(e.value, RuntimeError) and "no CPU fallback" in str(e.value) and mode in str(e.value)


def test_four_features_plus_depth_exceed_the_channel_limit():
    from easy_gaussian_splatting_amd.rendering import rasterization
    for mode in ("RGB+D", "RGB+ED"):
        with pytest.raises(NotImplementedError, match="4"):
            rasterization(**_args(colors=torch.zeros(4, 4), sh_degree=None), render_mode=mode)
    with pytest.raises(NotImplementedError, match="GPU only"):   # (the depth alone replaces the colours: no limit reached)
        rasterization(**_args(colors=torch.zeros(4, 4), sh_degree=None), render_mode="D")


@pytest.mark.parametrize("mode", DR.MODES)
def test_backgrounds_keep_the_colour_channel_count(mode):
    from easy_gaussian_splatting_amd.rendering import rasterization
    with pytest.raises(AssertionError):
        rasterization(**_args(backgrounds=torch.zeros(1, 4)), render_mode=mode)
    with pytest.raises(AssertionError):
        rasterization(**_args(colors=torch.zeros(4, 2), sh_degree=None, backgrounds=torch.zeros(1, 3)), render_mode=mode)


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("extra", [dict(_sh_grads="colors_pre"), dict(_grad_out={"means": torch.zeros(4, 3)}),
                                   dict(_sh_grads="colors_pre", _view_payload=torch.zeros(32))])
def test_depth_modes_are_refused_with_the_view_parallel_extensions(mode, extra):
    from easy_gaussian_splatting_amd.rendering import rasterization
    with pytest.raises(ValueError, match="render_mode"):
        rasterization(**_args(), render_mode=mode, **extra)


def test_the_model_layer_validates_its_depth_argument():
    from easy_gaussian_splatting_amd.model import GaussianModel
    import inspect
    sig = inspect.signature(GaussianModel.forward)
    assert sig.parameters["depth"].default is None and list(sig.parameters)[:4] == ["self", "data", "clamp", "depth"]


# ---- the entry points ----

def test_entry_points_are_declared_bound_and_check_their_arguments():
    from easy_gaussian_splatting_amd import _native as nat
    P, I, L64 = ct.c_void_p, ct.c_int, ct.c_int64
    sig = nat.SIGNATURES
    assert sig["gs_rec_depth"] == (ct.c_int, [P, I, L64, I, P, P, P])
    assert sig["gs_depth_partials_doubles"] == (ct.c_size_t, [I, L64])
    assert sig["gs_depth_grads"] == (ct.c_int, [P, I, L64, I] + [P] * 12)
    assert sig["gs_expected_depth_fwd"] == (ct.c_int, [P, L64, I, P, P, P])
    assert sig["gs_expected_depth_bwd"] == (ct.c_int, [P, L64, I] + [P] * 6)
    L = nat.lib()
    assert L.gs_version() >= 320
    buf = (ct.c_float * 64)()
    p = ct.addressof(buf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p = p if p % 16 == 0 else p + 8
    err = lambda: L.gs_last_error().decode()
    # (argument lists built in a loop go through these names; the written-out calls below are what
    #  tests/test_native_header.py counts against the header)
    rec_depth, depth_grads, ed_fwd, ed_bwd = L.gs_rec_depth, L.gs_depth_grads, L.gs_expected_depth_fwd, L.gs_expected_depth_bwd
    # lane outside 0..3
    for bad in (-1, 4):
        assert L.gs_rec_depth(None, 1, 8, bad, p, p, p) == -1 and "lane" in err()
        assert L.gs_depth_grads(None, 1, 8, bad, p, p, p, p, p, p, p, p, p, None, None, None) == -1 and "lane" in err()
    for bad in (0, 5):
        assert L.gs_expected_depth_fwd(None, 8, bad, p, p, p) == -1 and "channels" in err()
        assert L.gs_expected_depth_bwd(None, 8, bad, p, p, p, None, p, p) == -1 and "channels" in err()
    # null pointers
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert rec_depth(None, 1, 8, 3, *a) == -1 and "null pointer" in err()
        assert ed_fwd(None, 8, 4, *a) == -1 and "null pointer" in err()
    for k in range(9):
        a = [p] * 9
        a[k] = None
        assert depth_grads(None, 1, 8, 3, *a, None, None, None) == -1 and "null pointer" in err(), k
    for k in (0, 1, 2, 4, 5):   # (v_alphas_in, argument 3, may be NULL)
        a = [p] * 6
        a[k] = None
        assert ed_bwd(None, 8, 4, *a) == -1 and "null pointer" in err(), k
    # the camera term: v_viewmats and its scratch come together
    assert L.gs_depth_grads(None, 1, 8, 3, p, p, p, p, p, p, p, p, p, None, p, None) == -1 and "come together" in err()
    assert L.gs_depth_grads(None, 1, 8, 3, p, p, p, p, p, p, p, p, p, None, None, p) == -1 and "come together" in err()
    # misaligned buffers: rec; rows / qmask; the pixels of 4- and 2-channel images
    assert L.gs_rec_depth(None, 1, 8, 3, p, p, p + 4) == -1 and "16-byte" in err()
    for k in (5, 7):   # rows, qmask
        a = [p] * 9
        a[k] = p + 4
        assert depth_grads(None, 1, 8, 3, *a, None, None, None) == -1 and "16-byte" in err(), k
    assert L.gs_expected_depth_fwd(None, 8, 4, p + 8, p, p) == -1 and "aligned" in err()
    assert L.gs_expected_depth_fwd(None, 8, 2, p, p, p + 4) == -1 and "aligned" in err()
    assert L.gs_expected_depth_bwd(None, 8, 4, p, p, p, None, p + 8, p) == -1 and "aligned" in err()
    # sizes: 256 Gaussians per block, 4 doubles per (camera, block); nothing to do is no error
    assert L.gs_depth_partials_doubles(1, 1) == 4 and L.gs_depth_partials_doubles(2, 257) == 2 * 2 * 4 and L.gs_depth_partials_doubles(0, 5) == 0
    assert L.gs_rec_depth(None, 1, 0, 3, None, None, None) == 0
    assert L.gs_depth_grads(None, 2, 0, 0, None, None, None, None, None, None, None, None, None, None, None, None) == 0


# ---- the arithmetic ----

@pytest.fixture(scope="module")
def dm():
    so = os.path.join(HM, "libdepthmath.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "depthmath.cpp")], check=True)
    return ct.CDLL(so)


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ct.c_void_p)


@pytest.mark.parametrize("name", ["inside", "outside"])
def test_depth_vjp_against_autograd_on_general_poses(dm, name):
    """v_means and the row-2 terms of v_viewmats for an upstream gradient of the depths, under tests/cameras.py's general poses (no
    rotation is symmetric: a transposed A shows), against fp64 autograd of the oracle's projection."""
    from oracle import torch_oracle as TO
    sc, proj = cameras.config_scene(name, n=1500, W=96, H=64, C=2)
    N, C = sc["means"].shape[0], 2
    f64 = lambda k: torch.from_numpy(sc[k].astype(np.float64))
    means, V = f64("means").requires_grad_(True), f64("viewmats").requires_grad_(True)
    radii, _, depths, _ = TO.project(means, f64("quats"), f64("scales"), V, f64("Ks"), 96, 64, **proj)
    vis = (radii > 0).numpy()
    assert vis.mean() > 0.15
    v_z = np.random.default_rng(3).standard_normal((C, N)) * vis   # (culled Gaussians have no rows: their v_z is 0)
    ref_m, ref_V = torch.autograd.grad((depths * torch.from_numpy(v_z)).sum(), (means, V))
    base = np.random.default_rng(4).standard_normal((N, 3)).astype(np.float32)   # what the projection backward left in v_means
    got_m, sums = base.copy(), np.zeros((C, 4), np.float64)
    dm.dm_depth_grads(C, N, _p(sc["means"]), _p(sc["viewmats"]), _p(np.ascontiguousarray(v_z, dtype=np.float32)), _p(got_m), _p(sums))
    d_m = got_m.astype(np.float64) - base
    assert np.abs(d_m - ref_m.numpy()).max() <= GRAD_RTOL * np.abs(ref_m.numpy()).max()
    for c in range(C):
        ref = ref_V[c].numpy()
        assert np.all(ref[[0, 1, 3]] == 0) and np.abs(ref[2]).max() > 0   # (the depth reaches row 2 of the view matrix alone)
        assert np.abs(sums[c] - ref[2]).max() <= GRAD_RTOL * np.abs(ref[2]).max(), (c, sums[c], ref[2])
    A = sc["viewmats"][0, :3, :3].astype(np.float64)
    assert np.abs(A - A.T).max() > 0.05


def test_expected_depth_forward_and_vjp_against_torch(dm):
    """ED = acc / alpha.clamp(min=1e-10) and its VJP, fp32 against fp64 torch autograd on the same float32 inputs: ordinary alphas,
    alpha = 0 (an uncovered pixel: exactly 0, zero alpha gradient), alpha = 1e-10 exactly (the clamp passes the gradient: equality
    included) and the next float below it (it does not)."""
    floor = np.float32(1e-10)
    below = np.nextafter(floor, np.float32(0))
    rng = np.random.default_rng(5)
    alpha = np.concatenate([rng.uniform(0.004, 1.0, 64).astype(np.float32), np.array([0.0, 0.0, floor, floor, below, below], np.float32)])
    acc = (rng.uniform(0.5, 9.0, alpha.size) * alpha).astype(np.float32)
    acc[64:66] = 0.0, 0.0
    acc[66:] = np.float32(3e-10), np.float32(-2e-10), np.float32(3e-10), np.float32(-2e-10)
    v_out = rng.standard_normal(alpha.size).astype(np.float32)
    out, v_acc, v_alpha = (np.zeros_like(alpha) for _ in range(3))
    dm.dm_expected_depth(alpha.size, _p(acc), _p(alpha), _p(v_out), _p(out), _p(v_acc), _p(v_alpha))
    A, D = torch.from_numpy(alpha.astype(np.float64)).requires_grad_(True), torch.from_numpy(acc.astype(np.float64)).requires_grad_(True)
    # (the floor as the float32 value the kernels and torch's float32 clamp use)
    ref = D / A.clamp(min=float(floor))
    r_acc, r_alpha = torch.autograd.grad((ref * torch.from_numpy(v_out.astype(np.float64))).sum(), (D, A))
    assert np.isfinite(out).all() and np.isfinite(v_acc).all() and np.isfinite(v_alpha).all()
    # three float32 roundings at most per result (2.4e-7 relative: the storage bound of the parity suite)
    for got, want in ((out, ref.detach().numpy()), (v_acc, r_acc.numpy()), (v_alpha, r_alpha.numpy())):
        assert np.all(np.abs(got - want) <= 2.4e-7 * np.abs(want)), (got, want)
    assert out[64] == 0.0 and out[65] == 0.0 and v_alpha[64] == 0.0 and v_alpha[65] == 0.0
    assert v_alpha[66] != 0.0 and v_alpha[67] != 0.0 and r_alpha[66] != 0 and r_alpha[67] != 0   # alpha == 1e-10: passed
    assert v_alpha[68] == 0.0 and v_alpha[69] == 0.0 and r_alpha[68] == 0 and r_alpha[69] == 0   # the next float below: not
    # and the same floats as torch's own float32 evaluation
    t32 = torch.from_numpy(acc) / torch.from_numpy(alpha).clamp(min=1e-10)
    assert np.abs(out - t32.numpy()).max() <= 2.4e-7 * np.abs(t32.numpy()).max()
