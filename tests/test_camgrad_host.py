"""Camera gradients, host side: the camera-gradient functions of gs_math.h compiled for the host (tests/hostmath/camgrad.cpp) and
summed per camera in double, against fp64 autograd of the oracle w.r.t. `viewmats`; and the front end's keyword
`_camera_grads` with what it admits and refuses (no GPU needed)."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

import cameras
from oracle import torch_oracle as TO
from scenes import make_scene

HM = os.path.join(os.path.dirname(__file__), "hostmath")
GRAD_RTOL = 1e-3   # the project's gradient contract: within 1e-3 of the largest entry (tests/test_hostmath.py, tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def cg():
    so = os.path.join(HM, "libcamgrad.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "camgrad.cpp")], check=True)
    return ct.CDLL(so)


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ct.c_void_p)


@pytest.mark.parametrize("use_jac", [0, 1])
@pytest.mark.parametrize("deg,C,K", [(0, 1, 1), (1, 1, 4), (2, 2, 16), (3, 2, 16)])
def test_camera_gradient_sums_against_autograd(cg, deg, C, K, use_jac):
    N, W, H = 1500, 96, 64
    sc = make_scene(N, W, H, sh_degree=deg, n_views=C, seed=11 + deg, k_store=K, scale_range=(0.02, 0.4), dist=3.0)
    _camera_gradient_sums(cg, sc, deg, K, use_jac)


@pytest.mark.parametrize("use_jac", [0, 1])
@pytest.mark.parametrize("name", ["inside", "outside"])
def test_camera_gradient_sums_on_general_poses(cg, name, use_jac):
    """The same sums under tests/cameras.py's cameras: no rotation is symmetric (a transposed R in the camera-centre term or in
    sh_dir_term_jac shows), t has all three components, fx != fy and the principal point is off the centre (the FOV clamp is about
    the optical axis, W/2 / fx, whatever cx is), with each configuration's near / far / eps2d."""
    sc, proj = cameras.config_scene(name, n=1500, W=96, H=64, C=2)
    _camera_gradient_sums(cg, sc, 3, 16, use_jac, min_visible=0.15, **proj)


def _camera_gradient_sums(cg, sc, deg, K, use_jac, min_visible=0.25, near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3):
    N, C, W, H = sc["means"].shape[0], sc["viewmats"].shape[0], int(sc["width"]), int(sc["height"])
    f64 = lambda k: torch.from_numpy(sc[k].astype(np.float64))
    means, quats, scales, shs, Ks = (f64(k) for k in ("means", "quats", "scales", "shs", "Ks"))
    rng = np.random.default_rng(0)
    vm, vcn, vc = rng.standard_normal((C, N, 2)), rng.standard_normal((C, N, 3)), rng.standard_normal((C, N, 3))

    # fp64 autograd of the oracle's projection and SH colours w.r.t. the view matrices (culled entries carry no gradient)
    V = f64("viewmats").requires_grad_(True)
    radii, m2, _, con = TO.project(means, quats, scales, V, Ks, W, H, eps2d, near_plane, far_plane, radius_clip)
    (ref_proj,) = torch.autograd.grad((m2 * torch.from_numpy(vm)).sum() + (con * torch.from_numpy(vcn)).sum(), V)
    cols = TO.spherical_harmonics(deg, means, V, shs, radii)
    vis = radii > 0
    v_cols = torch.from_numpy(vc) * vis[..., None]   # (culled Gaussians: no colour, no gradient -- gsplat's masks)
    # (degree 0: the colour does not depend on the direction, so not on the camera)
    ref_sh = torch.autograd.grad(cols, V, v_cols)[0] if cols.requires_grad else torch.zeros_like(V)
    assert int(vis.sum()) > min_visible * C * N

    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    rad = np.ascontiguousarray(radii.numpy().astype(np.int32))
    sums = np.zeros((C, 16), np.float64)
    gm, gq, gs_ = np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32)
    rm, rq, rs = np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32)
    counts = np.zeros(2, np.int64)
    F = ct.c_float
    cg.cg_camera_grads(C, N, K, deg, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["shs"]), _p(sc["viewmats"]), _p(sc["Ks"]),
                       W, H, F(eps2d), F(near_plane), F(far_plane), _p(rad), _p(f32(cols.detach().numpy())), _p(f32(vm)), _p(f32(vcn)), _p(f32(vc)),
                       use_jac, _p(sums), _p(gm), _p(gq), _p(gs_), _p(rm), _p(rq), _p(rs), _p(counts))
    # the clamped branch of the perspective Jacobian is in the sum
    assert counts[0] > 0, "no visible Gaussian beyond the FOV clamp: the scene does not exercise the clamped branch"
    # project_vjp_cam leaves project_vjp's geometry gradients, and the direction term on its own is what sh_vjp adds: bit for bit
    assert np.array_equal(gm, rm) and np.array_equal(gq, rq) and np.array_equal(gs_, rs)
    assert counts[1] == 0

    for c in range(C):
        got = np.zeros((4, 4))
        got[:3, :3] = sums[c, :9].reshape(3, 3)
        got[:3, 3] = sums[c, 9:12]
        ref = ref_proj[c].numpy()
        assert np.all(ref[3] == 0)
        assert np.abs(got - ref).max() <= GRAD_RTOL * np.abs(ref).max(), (c, np.abs(got - ref).max() / np.abs(ref).max())
    # SH direction part: v_campos through the VJP of the 4x4 inverse, all 16 entries
    Vl = f64("viewmats").requires_grad_(True)
    campos = torch.linalg.inv(Vl)[:, :3, 3]
    (got_sh,) = torch.autograd.grad(campos, Vl, torch.from_numpy(sums[:, 12:15].copy()))
    if deg == 0:
        assert float(ref_sh.abs().max()) == 0.0 and np.all(sums[:, 12:15] == 0)
    else:
        for c in range(C):
            g, r = got_sh[c].numpy(), ref_sh[c].numpy()
            assert np.abs(g - r).max() <= GRAD_RTOL * np.abs(r).max(), (c, np.abs(g - r).max() / np.abs(r).max())


def _frontend_args(requires_grad=True, K_grad=False):
    N = 4
    V = torch.eye(4)[None].clone().requires_grad_(requires_grad)
    Ks = torch.eye(3)[None].clone().requires_grad_(K_grad)
    return dict(means=torch.zeros(N, 3), quats=torch.ones(N, 4), scales=torch.ones(N, 3), opacities=torch.ones(N),
                colors=torch.zeros(N, 16, 3), viewmats=V, Ks=Ks, width=32, height=32, sh_degree=3, packed=False)


def test_frontend_admits_view_matrices_that_require_grad_when_asked():
    from easy_gaussian_splatting_amd.rendering import rasterization
    # past the refusal: CPU tensors then meet the product path's refusal to fall back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(**_frontend_args(), _camera_grads=True)
    # without the keyword the refusal stays, and names the keyword
    with pytest.raises(NotImplementedError, match="_camera_grads"):
        rasterization(**_frontend_args())
    # the keyword with constant cameras is an ordinary call
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(**_frontend_args(requires_grad=False), _camera_grads=True)


def test_frontend_still_refuses_intrinsics_gradients():
    from easy_gaussian_splatting_amd.rendering import rasterization
    with pytest.raises(NotImplementedError):
        rasterization(**_frontend_args(K_grad=True), _camera_grads=True)
    with pytest.raises(NotImplementedError):
        rasterization(**_frontend_args(requires_grad=False, K_grad=True))


@pytest.mark.parametrize("extra", [dict(_sh_grads="colors_pre"), dict(_grad_out={"means": torch.zeros(4, 3)}),
                                   dict(_sh_grads="colors_pre", _view_payload=torch.zeros(32))])
def test_frontend_refuses_camera_grads_with_the_view_parallel_extensions(extra):
    from easy_gaussian_splatting_amd.rendering import rasterization
    with pytest.raises(ValueError, match="_camera_grads"):
        rasterization(**_frontend_args(), _camera_grads=True, **extra)


def test_entry_points_are_declared_and_bound():
    from easy_gaussian_splatting_amd import _native as nat
    sig = nat.SIGNATURES
    assert sig["gs_project_bwd_cam"][1] == sig["gs_project_bwd"][1] + [ct.c_void_p, ct.c_void_p, ct.c_void_p]
    assert sig["gs_cam_partials_doubles"] == (ct.c_size_t, [ct.c_int, ct.c_int64])
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gs_raster.h")).read()
    assert "int gs_project_bwd_cam(" in header and "size_t gs_cam_partials_doubles(" in header
    L = nat.lib()
    assert L.gs_version() >= 310
    # 256 Gaussians per block, 16 doubles per (camera, block)
    assert L.gs_cam_partials_doubles(1, 1) == 16 and L.gs_cam_partials_doubles(2, 257) == 2 * 2 * 16
    assert L.gs_cam_partials_doubles(1, 1_000_000) == 3907 * 16


def test_pose_module_is_the_identity_at_zero_and_differentiable_there():
    from easy_gaussian_splatting_amd.pose import CameraDeltas
    cd = CameraDeltas(3)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.1, -0.2, 4.0])
    out = cd(w2c, 1)
    assert out.shape == (4, 4) and torch.equal(out, w2c)
    out.sum().backward()
    g = cd.deltas.grad
    assert torch.isfinite(g).all() and float(g[1].abs().max()) > 0 and float(g[0].abs().max()) == 0 and float(g[2].abs().max()) == 0
    # a small rotation about z and a translation: [[exp([w]x), tau], [0, 1]] @ w2c
    with torch.no_grad():
        cd.deltas[2] = torch.tensor([0.0, 0.0, 0.01, 0.03, -0.02, 0.04])
    got = cd(w2c, 2).detach()
    c, s = np.cos(0.01), np.sin(0.01)
    D = torch.tensor([[c, -s, 0, 0.03], [s, c, 0, -0.02], [0, 0, 1, 0.04], [0, 0, 0, 1]], dtype=torch.float32)
    assert torch.allclose(got, D @ w2c, atol=1e-6)
