"""Camera models, host side (no GPU): the reference's closed-form Jacobian against autograd of its own mean map and its continuity
onto the optical axis; the camera-model instantiations of gs_math.h's projection chain and VJP, compiled for the host
(tests/hostmath/camera_models.cpp), against the reference at the bounds tests/test_hostmath.py uses; the pinhole instantiation against
today's hm_forward / hm_backward, bit for bit; and what the front end (rasterization, the COLMAP reader, TrainStepGraph) admits and
refuses."""
import ctypes as ct
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import camera_model_ref as CM
from scenes import make_scene

HM = os.path.join(os.path.dirname(__file__), "hostmath")
GRAD_RTOL = 1e-3   # the project's gradient contract: within 1e-3 of the largest entry (tests/test_hostmath.py)
MODEL_ID = {"pinhole": 0, "ortho": 1, "fisheye": 2}
F = ct.c_float


@pytest.fixture(scope="module")
def cm():
    so = os.path.join(HM, "libcameramodels.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "camera_models.cpp")], check=True)
    return ct.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(HM, "libhostmath.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "hostmath.cpp")], check=True)
    return ct.CDLL(so)


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ct.c_void_p)


def _f64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


# ---- 1. the reference itself ----

def _points():
    """Camera-space points: scene X's radii (rho = 0 .. 1 at z = 2, and the axis at eight depths) and a random cloud."""
    rng = np.random.default_rng(1)
    pts = []
    for rho in CM.X_RHOS:
        for j in range(8):
            phi = 2 * np.pi * (j + 0.3) / 8
            pts.append((rho * 2 * np.cos(phi), rho * 2 * np.sin(phi), 2.0 + (0.25 * j if rho == 0 else 0.0)))
    pts += [tuple(p) for p in np.concatenate([rng.uniform(-3, 3, (200, 2)), rng.uniform(0.05, 6, (200, 1))], axis=1)]
    return torch.tensor(pts, dtype=torch.float64)


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
def test_reference_jacobian_is_the_derivative_of_its_mean_map(model):
    p = _points().requires_grad_(True)
    fx, fy, cx, cy = (torch.tensor(v, dtype=torch.float64) for v in (40.9, 37.3, 50.0, 40.0))
    u, v = CM.mean_map(model, p[:, 0], p[:, 1], p[:, 2], fx, fy, cx, cy)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(v).all())   # (the axis included: theta / r at r = 0)
    (gu,) = torch.autograd.grad(u.sum(), p, retain_graph=True)
    (gv,) = torch.autograd.grad(v.sum(), p)
    J = CM.jacobian(model, p[:, 0], p[:, 1], p[:, 2], fx, fy).detach()
    err = (torch.stack([gu, gv], dim=1) - J).abs().max().item()
    print(f"{model}: max |J - autograd| = {err:.3g}")
    assert bool(torch.isfinite(gu).all()) and bool(torch.isfinite(gv).all())
    assert err <= 1e-12 * float(J.abs().max())


def test_reference_fisheye_is_continuous_onto_the_axis():
    """k -> 1 / z and g -> -2 / (3 z^3): the values at r = 0 (the `where` branch) against those a hair off the axis (the closed form)."""
    z = torch.tensor([0.3, 1.0, 2.0, 3.75], dtype=torch.float64)
    k0, g0 = CM.fisheye_kg(torch.zeros_like(z), torch.zeros_like(z), z)
    assert torch.equal(k0, 1.0 / z) and torch.allclose(g0, -2.0 / (3.0 * z ** 3), rtol=1e-15)
    r = 1e-3 * z
    k1, g1 = CM.fisheye_kg(r, torch.zeros_like(z), z)
    assert ((k1 - k0).abs() * z).max().item() < 1e-6          # k z = 1 - rho^2 / 3 + ...
    assert ((g1 - g0).abs() * z ** 3).max().item() < 1e-5     # g z^3 = -2/3 + 4/5 rho^2 - ... (the closed form's own eps / rho^2 included)
    fx = fy = torch.tensor(40.0, dtype=torch.float64)
    J0 = CM.jacobian("fisheye", torch.zeros_like(z), torch.zeros_like(z), z, fx, fy)
    J1 = CM.jacobian("fisheye", r, torch.zeros_like(z), z, fx, fy)
    assert ((J1 - J0).abs().amax((-1, -2)) * z).max().item() < 40.0 * 2e-3   # (J02 = -fx x / d^2 is first order in rho)


def test_device_radial_terms_match_their_closed_forms_across_the_series_threshold(cm):
    """fisheye_terms in double on both sides of the series threshold rho^2 = 1/256: against the closed forms in float64 where those are
    good (rho >= 1e-2), against the on-axis limits where they are not, and without a step at the threshold."""
    z = 2.0
    rho = np.array([0.0, 1e-7, 1e-5, 1e-3, 1e-2, 0.06, 0.0624, 0.0626, 0.07, 0.1, 0.5, 1.0, 3.0])
    xyz = np.ascontiguousarray(np.stack([rho * z * 0.6, rho * z * 0.8, np.full_like(rho, z)], axis=1))
    out = np.zeros((len(rho), 4))
    cm.cm_fisheye_terms(len(rho), _p(xyz), _p(out))
    assert np.isfinite(out).all()
    r2 = (rho * z) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.arctan2(np.sqrt(r2), z) / np.sqrt(r2)
        e = 1.0 / (r2 + z * z)
        g = (z * e - k) / r2
        h = -(2 * z * e * e + 3 * g) / r2
    assert np.allclose(out[:, 1], e, rtol=1e-15)
    good = rho >= 1e-2   # the closed forms' own error there: eps / rho^2 = 1e-12 (g), eps / rho^4 = 1e-8 (h)
    assert np.allclose(out[good, 0], k[good], rtol=1e-13) and np.allclose(out[good, 2], g[good], rtol=1e-10) and np.allclose(out[good, 3], h[good], rtol=2e-7)
    small = rho <= 1e-3  # the limits, to their first neglected term
    assert np.allclose(out[small, 0] * z, 1.0, atol=1e-6) and np.allclose(out[small, 2] * z ** 3, -2.0 / 3, atol=1e-6)
    assert np.allclose(out[small, 3] * z ** 5, 8.0 / 5, atol=1e-5)
    # no step at the threshold (rho = 1/16): neighbours on either side agree to the slope between them
    i, j = list(rho).index(0.0624), list(rho).index(0.0626)
    for col, scale in ((0, z), (2, z ** 3), (3, z ** 5)):
        assert abs(out[i, col] - out[j, col]) * scale < 2e-3


# ---- 2. gs_math.h on the host against the reference ----

def _host_forward(cm, sc, model):
    W, H = int(sc["width"]), int(sc["height"])
    C, N, K = sc["viewmats"].shape[0], sc["means"].shape[0], sc["shs"].shape[1]
    out = dict(radii=np.zeros((C, N), np.int32), means2d=np.zeros((C, N, 2), np.float32), depths=np.zeros((C, N), np.float32),
               conics=np.zeros((C, N, 3), np.float32), colors=np.zeros((C, N, 3), np.float32), tpg=np.zeros((C, N), np.int32))
    rc = cm.cm_forward(MODEL_ID[model], C, N, K, int(sc["sh_degree"]), _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["shs"]),
                       _p(sc["viewmats"]), _p(sc["Ks"]), W, H, 16, F(0.3), F(0.01), F(1e10), F(0.0), _p(out["radii"]), _p(out["means2d"]),
                       _p(out["depths"]), _p(out["conics"]), _p(out["colors"]), _p(out["tpg"]))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", ["F1", "O1", "X"])
def test_host_chain_and_vjp_against_the_reference(cm, name):
    sc, model = CM.scene(name)
    W, H = int(sc["width"]), int(sc["height"])
    C, N = sc["viewmats"].shape[0], sc["means"].shape[0]
    ins = [_f64(sc[k]).requires_grad_(True) for k in ("means", "quats", "scales")]
    V = _f64(sc["viewmats"]).requires_grad_(True)
    radii, m2, dep, con = CM.project(model, *ins, V, _f64(sc["Ks"]), W, H)
    ref_r = radii.numpy()
    vis = int((ref_r > 0).sum())
    assert vis >= CM.VISIBLE[name] // 2 and (name != "X" or vis == 64)
    got = _host_forward(cm, sc, model)
    # the forward, at tests/test_hostmath.py's bounds
    assert (got["radii"] != ref_r).mean() < 2e-3
    same = got["radii"] == ref_r
    assert name != "X" or same.all()
    assert np.abs(got["means2d"] - m2.detach().numpy())[same].max() < 1e-3
    assert np.abs(got["depths"] - dep.detach().numpy())[same].max() < 1e-5
    cn = con.detach().numpy()
    assert (np.abs(got["conics"] - cn) / (np.abs(cn) + 1e-2))[same].max() < 1e-3
    tw, th = -(-W // 16), -(-H // 16)
    tpg, _, _ = CM.TO.isect_tiles(m2.detach(), radii, dep.detach(), 16, tw, th)
    assert (got["tpg"] != tpg.numpy())[same].mean() < 2e-3
    cols = CM.TO.spherical_harmonics(int(sc["sh_degree"]), ins[0].detach(), V.detach(), _f64(sc["shs"]), radii).numpy()
    assert np.abs(got["colors"] - cols)[same & (ref_r > 0)].max() < 1e-5
    # the VJP (the depth's gradient included) and the view matrix's share, against autograd
    rng = np.random.default_rng(0)
    vm, vcn, vd = rng.standard_normal((C, N, 2)), rng.standard_normal((C, N, 3)), rng.standard_normal((C, N))
    keep = torch.from_numpy(same)
    loss = (m2 * _f64(vm))[keep].sum() + (con * _f64(vcn))[keep].sum() + (dep * _f64(vd))[keep].sum()
    ref = torch.autograd.grad(loss, ins + [V])
    assert all(bool(torch.isfinite(g).all()) for g in ref)
    rad_use = np.ascontiguousarray(np.where(same, ref_r, 0).astype(np.int32))
    hv = [np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32)]
    sums = np.zeros((C, 12))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    rc = cm.cm_backward(MODEL_ID[model], C, N, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H, F(0.3),
                        F(0.01), F(1e10), _p(rad_use), _p(f32(vm)), _p(f32(vcn)), _p(f32(vd)), _p(hv[0]), _p(hv[1]), _p(hv[2]), _p(sums))
    assert rc == 0
    for nm, a, b in zip(("means", "quats", "scales"), hv, ref[:3]):
        b = b.numpy()
        assert np.isfinite(a).all(), nm
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{name} v_{nm}: {err:.3g}")
        assert err <= GRAD_RTOL, (nm, err)
        if name == "X":   # ... and row by row: the on-axis and the series groups are not hidden behind the largest Gaussian
            rows = np.abs(a - b).max(-1) / np.maximum(np.abs(b).max(-1), 1e-3 * np.abs(b).max())
            assert rows.max() <= GRAD_RTOL, (nm, int(rows.argmax()), rows.max())
    gv = ref[3].numpy()
    cam = np.concatenate([sums[:, :9].reshape(C, 3, 3), sums[:, 9:, None]], axis=2)
    for c in range(C):
        err = np.abs(cam[c] - gv[c, :3]).max() / np.abs(gv[c, :3]).max()
        print(f"{name} v_viewmats[{c}]: {err:.3g}")
        assert err <= GRAD_RTOL, (c, err)


def test_pinhole_instantiation_is_todays_chain_bit_for_bit(cm, hm):
    N, W, H, C, K, deg = 1500, 96, 64, 2, 16, 3
    sc = make_scene(N, W, H, sh_degree=deg, n_views=C, seed=14, k_store=K, scale_range=(0.02, 0.4), dist=3.0)
    got = _host_forward(cm, sc, "pinhole")
    want = dict(radii=np.zeros((C, N), np.int32), means2d=np.zeros((C, N, 2), np.float32), depths=np.zeros((C, N), np.float32),
                conics=np.zeros((C, N, 3), np.float32), colors=np.zeros((C, N, 3), np.float32), tpg=np.zeros((C, N), np.int32))
    hm.hm_forward(C, N, K, deg, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["shs"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H, 16,
                  F(0.3), F(0.01), F(1e10), F(0.0), _p(want["radii"]), _p(want["means2d"]), _p(want["depths"]), _p(want["conics"]),
                  _p(want["colors"]), _p(want["tpg"]))
    assert (want["radii"] > 0).sum() > N // 2
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    rng = np.random.default_rng(2)
    vm, vcn = rng.standard_normal((C, N, 2)).astype(np.float32), rng.standard_normal((C, N, 3)).astype(np.float32)
    vc = np.zeros((C, N, 3), np.float32)   # (no colour gradient: hm_backward then adds the projection's VJP alone)
    a = [np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32)]
    b = [np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32)]
    sums, v_shs = np.zeros((C, 12)), np.zeros((N, K, 3), np.float32)
    cm.cm_backward(0, C, N, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H, F(0.3), F(0.01), F(1e10),
                   _p(want["radii"]), _p(vm), _p(vcn), None, _p(a[0]), _p(a[1]), _p(a[2]), _p(sums))
    hm.hm_backward(C, N, K, deg, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["shs"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H,
                   F(0.3), F(0.01), F(1e10), _p(want["radii"]), _p(want["colors"]), _p(vm), _p(vcn), _p(vc), _p(b[0]), _p(b[1]), _p(b[2]),
                   _p(v_shs), 0)
    for x, y, nm in zip(a, b, ("means", "quats", "scales")):
        assert np.abs(y).max() > 0 and np.array_equal(x, y), nm


# ---- 3. the front end ----

def _args(n=4):
    return (torch.zeros((n, 3)), torch.ones((n, 4)), torch.ones((n, 3)), torch.ones(n), torch.zeros((n, 1, 3)), torch.eye(4)[None],
            torch.eye(3)[None], 32, 32)


def test_rasterization_refuses_unknown_models_and_the_view_parallel_keywords():
    from easy_gaussian_splatting_amd.rendering import CAMERA_MODELS, rasterization
    assert sorted(CAMERA_MODELS) == ["fisheye", "ortho", "pinhole"]
    with pytest.raises(ValueError, match="camera_model"):
        rasterization(*_args(), sh_degree=0, packed=False, camera_model="equirect")
    for model in ("ortho", "fisheye"):
        for bad in (dict(_sh_grads="colors_pre"), dict(_grad_out={}), dict(_view_payload=torch.zeros(64))):
            with pytest.raises(ValueError, match="camera_model"):
                rasterization(*_args(), sh_degree=0, packed=False, camera_model=model, **bad)
        # CPU tensors raise as they do today
        with pytest.raises(RuntimeError, match="GPU only"):
            rasterization(*_args(), sh_degree=0, packed=False, camera_model=model)
        # ... and what today's tests lock stays locked under the keyword
        with pytest.raises(NotImplementedError):
            rasterization(*_args(), sh_degree=0, packed=True, camera_model=model)
        with pytest.raises(NotImplementedError):
            rasterization(*_args(), sh_degree=0, packed=False, rasterize_mode="antialiased", camera_model=model)
    with pytest.raises(RuntimeError, match="GPU only"):
        rasterization(*_args(), sh_degree=0, packed=False, camera_model="pinhole")


def _write_cameras(path: Path, cams):
    """cameras.bin: u64 count | per camera: i32 id, i32 model id, u64 w, u64 h, f64 params[]."""
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, model_id, w, h, params in cams:
            f.write(struct.pack("<iiQQ", cid, model_id, w, h))
            f.write(struct.pack("<" + "d" * len(params), *params))


def test_colmap_reader_takes_an_undistorted_opencv_fisheye(tmp_path):
    from easy_gaussian_splatting_amd import scene as S
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    from make_synthetic_dataset import write_colmap
    write_colmap(tmp_path, n_images=3, n_points=20, model="PINHOLE", with_masks=False)
    cams_bin = tmp_path / "sparse" / "0" / "cameras.bin"
    _write_cameras(cams_bin, [(7, 8, 64, 48, [31.5, 30.25, 32.5, 23.75, 0.0, 0.0, 0.0, 0.0])])
    cams = S.load_intrinsics_binary(cams_bin)
    assert cams[7].model_name == "OPENCV_FISHEYE" and cams[7].camera_model == "fisheye"
    assert (cams[7].fx, cams[7].fy, cams[7].cx, cams[7].cy) == (31.5, 30.25, 32.5, 23.75)
    frames, _, _, _ = S.load_colmap_data(str(tmp_path), False, 0, False, 0.0, False)
    assert len(frames) == 3 and all(f.camera_model == "fisheye" for f in frames)
    d = frames[0].to_data()
    assert d["camera_model"] == "fisheye" and d["K"][0, 0].item() == 31.5
    # distortion terms: the images must be undistorted first
    for k in range(4):
        params = [31.5, 30.25, 32.5, 23.75, 0.0, 0.0, 0.0, 0.0]
        params[4 + k] = 1e-3
        _write_cameras(cams_bin, [(7, 8, 64, 48, params)])
        with pytest.raises(ValueError, match="undistorted"):
            S.load_intrinsics_binary(cams_bin)
    # a pinhole model is what it was: no key in the frame's dict
    _write_cameras(cams_bin, [(7, 1, 64, 48, [55.5, 54.25, 32.5, 23.75])])
    frames, _, _, _ = S.load_colmap_data(str(tmp_path), False, 0, False, 0.0, False)
    assert all(f.camera_model == "pinhole" for f in frames) and "camera_model" not in frames[0].to_data()
    # mixed camera models keep raising, and so do the models the reader does not know
    _write_cameras(cams_bin, [(7, 1, 64, 48, [55.5, 54.25, 32.5, 23.75]), (8, 8, 64, 48, [31.5, 30.25, 32.5, 23.75, 0.0, 0.0, 0.0, 0.0])])
    with pytest.raises(AssertionError):
        S.load_intrinsics_binary(cams_bin)
    _write_cameras(cams_bin, [(7, 4, 64, 48, [31.5, 30.25, 32.5, 23.75, 0.0, 0.0, 0.0, 0.0])])   # (OPENCV)
    with pytest.raises(ValueError, match="unsupported camera model id"):
        S.load_intrinsics_binary(cams_bin)
    with pytest.raises(ValueError, match="camera_model"):
        S.Frame(tmp_path / "a.png", None, 0, 64, 48, 30.0, 30.0, 32.0, 24.0, np.eye(4), False, camera_model="equirect")


def test_model_and_viewer_pass_the_camera_model_through(monkeypatch):
    from easy_gaussian_splatting_amd import model as M
    seen = {}

    def fake(**kw):
        seen.update(kw)
        raise RuntimeError("stop here")
    monkeypatch.setattr(M, "rasterization", fake)
    m = M.GaussianModel(means=torch.zeros((4, 3)), log_scales=torch.zeros((4, 3)), quats=torch.ones((4, 4)), sh_0=torch.zeros((4, 1, 3)),
                        sh_rest=torch.zeros((4, 3, 3)), logit_opacities=torch.zeros(4), sh_degree=1, white_background=True)
    data = {"w2c": torch.eye(4), "K": torch.eye(3), "width": 32, "height": 32}
    with pytest.raises(RuntimeError, match="stop here"):
        m(dict(data, camera_model="fisheye"))
    assert seen["camera_model"] == "fisheye"
    seen.clear()
    with pytest.raises(RuntimeError, match="stop here"):
        m(data)
    assert "camera_model" not in seen   # (the pinhole call is the call as it was)
    from easy_gaussian_splatting_amd.viewer import FrameRenderer
    with pytest.raises(ValueError, match="camera_model"):
        FrameRenderer(m, camera_model="equirect")


def test_train_step_graph_refuses_what_has_no_fused_kernel_yet():
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph, ViewParallelGraphStep
    data = {"w2c": torch.eye(4), "K": torch.eye(3), "width": 32, "height": 32}
    gt = torch.zeros((32, 32, 3))
    stub = object()   # (every refusal comes before the runner looks at its model, optimizer or loss)
    with pytest.raises(ValueError, match="camera_model"):
        TrainStepGraph(stub, stub, stub, data, gt, camera_model="equirect")
    for model in ("ortho", "fisheye"):
        for kw, names in ((dict(mcmc=stub), "gs_project_bwd_adam_mcmc"), (dict(poses=stub), "gs_project_bwd_adam_sums"),
                          (dict(depth=stub), "gs_project_bwd_adam_depth"), (dict(rounds="on"), "rblk")):
            with pytest.raises(ValueError, match=names):
                TrainStepGraph(stub, stub, stub, data, gt, camera_model=model, **kw)
        with pytest.raises(ValueError, match="SUMS"):
            ViewParallelGraphStep(stub, stub, stub, data, gt, vp=stub, camera_model=model)
        with pytest.raises(ValueError, match="data\\['camera_model'\\]"):
            TrainStepGraph(stub, stub, stub, dict(data, camera_model="pinhole"), gt, camera_model=model)
