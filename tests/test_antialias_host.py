"""The antialiased rasterize mode, host side (no GPU): the reference's own checks (tests/antialias_ref.py) -- the closed-form gradient of
rho against autograd, the range of rho on the scenes, and what the mode MEANS: the alpha a lone Gaussian deposits --; the AA = true
instantiations of gs_math.h's projection chain and VJP, compiled for the host (tests/hostmath/antialias.cpp), against the reference at
the bounds tests/test_hostmath.py uses; the AA = false instantiation against today's hm_forward / hm_backward bit for bit; the
degenerate scene; and what the front end (rasterization, GaussianModel, TrainStepGraph) admits and refuses."""
import ctypes as ct
import math
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

import antialias_ref as AR
from scenes import make_scene

HM = os.path.join(os.path.dirname(__file__), "hostmath")
GRAD_RTOL = 1e-3   # the project's gradient contract: within 1e-3 of the largest entry (tests/test_hostmath.py)
F = ct.c_float
_f64 = AR._f64


@pytest.fixture(scope="module")
def aa():
    so = os.path.join(HM, "libantialias.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "antialias.cpp")], check=True)
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


# ---- 1. the reference itself ----

def test_closed_form_gradient_of_rho_is_autograds():
    """G += w [[c0 - rho^2 c, -b (1 - rho^2)], [., a0 - rho^2 a]] / det with w = v_rho / (2 rho) -- the increments of DESIGN.md section 24
    with the 1e-6 guard removed -- against fp64 autograd of rho over the entries of cov2_0, to 1e-12 of the largest entry."""
    g = torch.Generator().manual_seed(3)
    n, eps = 4000, 0.3
    s1 = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(math.log(0.06), math.log(30.0), generator=g))
    s2 = s1 * torch.empty(n, dtype=torch.float64).uniform_(1.0, 8.0, generator=g)
    th = torch.empty(n, dtype=torch.float64).uniform_(0, math.pi, generator=g)
    a0 = (s1 * torch.cos(th)) ** 2 + (s2 * torch.sin(th)) ** 2
    c0 = (s1 * torch.sin(th)) ** 2 + (s2 * torch.cos(th)) ** 2
    b = (s1 * s1 - s2 * s2) * torch.sin(th) * torch.cos(th)
    # off-diagonal as two entries b01 = b10 = b: the per-entry gradient, which is how g01 is counted
    a0, b01, b10, c0 = (t.clone().requires_grad_(True) for t in (a0, b, b, c0))
    det0 = a0 * c0 - b01 * b10
    det = (a0 + eps) * (c0 + eps) - b01 * b10
    rho = torch.sqrt(det0 / det)
    v_rho = torch.randn(n, generator=g, dtype=torch.float64)
    ga, g01, g10, gc = torch.autograd.grad((rho * v_rho).sum(), (a0, b01, b10, c0))
    with torch.no_grad():
        a, c, r2 = a0 + eps, c0 + eps, rho * rho
        w = v_rho * 0.5 / rho
        G00, G11, G01 = w * ((c - eps) - r2 * c) / det, w * ((a - eps) - r2 * a) / det, w * (-b * (1 - r2)) / det
    for nm, got, want in (("G00", G00, ga), ("G11", G11, gc), ("G01", G01, g01), ("G10", G01, g10)):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"{nm}: {err:.3g}")
        assert err <= 1e-12, (nm, err)
    assert 0.0 < float(rho.detach().min()) < 0.02 and 0.99 < float(rho.detach().max()) < 1.0


def test_rho_is_inside_the_unit_interval_and_reaches_zero_only_on_the_degenerate_scene():
    lo_hi = {}
    for name in "ABZ":
        sc = AR.scene(name)
        with torch.no_grad():
            fw = AR.forward(sc)
        vis = fw["radii"] > 0
        rho = fw["rho"][vis]
        lo_hi[name] = (float(rho.min()), float(rho.max()), int(vis.sum()), vis.numel())
        assert bool((fw["rho"][~vis] == 0).all()) and bool((fw["opacities"][~vis] == 0).all())
        if name == "Z":
            d = AR.Z_DEGENERATE
            assert bool(vis[0, :d].all()) and bool((fw["rho"][0, :d] == 0).all()) and bool((fw["rho"][0, d:] > 0.3).all())
        else:
            assert 1e-2 <= float(rho.min()) and float(rho.max()) < 1.0, (name, lo_hi[name])
    print(lo_hi)   # (the realised ranges: A 0.0142 .. 0.9967 over 300 of 300, B 0.0373 .. 0.99991 over 240 of 240)
    assert lo_hi["A"][0] < 0.02 and lo_hi["A"][1] > 0.99 and lo_hi["A"][2] == 300
    assert lo_hi["B"][2] >= 200 and lo_hi["B"][1] > 0.999   # (whole-frame footprints: rho -> 1)


@pytest.mark.parametrize("sigma", [0.4, 1.0, 3.0])
def test_an_isolated_gaussian_deposits_the_alpha_of_the_unblurred_gaussian(sigma):
    """What the mode means.  A lone Gaussian of opacity o and projected sigma s deposits sum_pixels alpha.  Antialiased: o rho times the
    blurred Gaussian, whose integral is 2 pi sqrt(det) -- together 2 pi o sqrt(det0), the mass of the Gaussian as it is, whatever
    eps2d blurs it to; within 5 %: the 3-sigma truncation <= 1.2 %, sampling a Gaussian of sigma >= 0.55 px at the pixel centres
    <= 0.6 %, the 1/255 cut <= 1 / (255 * 0.4) = 1 %.  Classic: o times the blurred Gaussian: an overshoot by 1 / rho (2.9 x at 0.4 px, where rho = 0.348)."""
    W, H, o, z0 = 65, 49, 0.9, 3.0
    Ks = AR._pinhole(W, H, 1)
    f = float(Ks[0, 0, 0])
    # centred on the pixel centre (32.5, 24.5) = the principal point: mean on the optical axis
    sc = dict(means=np.zeros((1, 3), np.float32), quats=np.array([[1, 0, 0, 0]], np.float32), scales=np.full((1, 3), sigma * z0 / f, np.float32),
              opacities=np.array([o], np.float32), shs=np.zeros((1, 1, 3), np.float32), viewmats=AR._view(z0)[None], Ks=Ks, width=W, height=H, sh_degree=0)
    with torch.no_grad():
        on, off = AR.forward(sc), AR.forward(sc, antialiased=False)
    rho = float(on["rho"][0, 0])
    s2 = float(sc["scales"][0, 0]) ** 2 * (f / z0) ** 2
    assert abs(rho - s2 / (s2 + 0.3)) < 1e-6 and rho >= 0.34   # (0.4 px: 0.348; the isotropic closed form)
    mass = 2 * math.pi * o * s2   # 2 pi o sqrt(det0)
    got_on, got_off = float(on["alpha"].sum()), float(off["alpha"].sum())
    print(f"sigma {sigma}: rho {rho:.4f}, sum alpha / (2 pi o sqrt(det0)): antialiased {got_on / mass:.4f}, classic {got_off / mass:.4f} (1 / rho = {1 / rho:.4f})")
    assert abs(got_on / mass - 1.0) <= 0.05
    assert abs(got_off / (mass / rho) - 1.0) <= 0.05 and got_off / mass >= (1.0 / rho) * 0.95


# ---- 2. the host build of the chain and the VJP ----

def _host_forward(aa, sc, on=1):
    W, H = int(sc["width"]), int(sc["height"])
    C, N = sc["viewmats"].shape[0], sc["means"].shape[0]
    out = dict(radii=np.zeros((C, N), np.int32), means2d=np.zeros((C, N, 2), np.float32), depths=np.zeros((C, N), np.float32),
               conics=np.zeros((C, N, 3), np.float32), rho=np.zeros((C, N), np.float32), op_eff=np.zeros((C, N), np.float32),
               extents=np.zeros((C, N, 2), np.float32))
    rc = aa.aa_forward(on, C, N, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["opacities"]), _p(sc["viewmats"]), _p(sc["Ks"]),
                       W, H, 16, F(0.3), F(0.01), F(1e10), F(0.0), *(_p(out[k]) for k in ("radii", "means2d", "depths", "conics", "rho", "op_eff", "extents")))
    assert rc == 0
    return out


def _host_backward(aa, sc, radii, vm, vcn, vd, vo, on=1):
    W, H = int(sc["width"]), int(sc["height"])
    C, N = sc["viewmats"].shape[0], sc["means"].shape[0]
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    hv = [np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32), np.zeros((N,), np.float32)]
    sums = np.zeros((C, 12))
    rc = aa.aa_backward(on, C, N, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["opacities"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H,
                        F(0.3), F(0.01), F(1e10), _p(np.ascontiguousarray(radii, dtype=np.int32)), _p(f32(vm)), _p(f32(vcn)), _p(f32(vd)), _p(f32(vo)),
                        *(_p(h) for h in hv), _p(sums))
    assert rc == 0
    return hv, sums


def _reference_vjp(sc, vm, vcn, vd, vo, keep):
    ins = [_f64(sc[k]).requires_grad_(True) for k in AR.GEO]
    V = _f64(sc["viewmats"]).requires_grad_(True)
    radii, m2, dep, con, rho = AR.project(ins[0], ins[1], ins[2], V, _f64(sc["Ks"]), int(sc["width"]), int(sc["height"]))
    op_eff = ins[3][None, :] * rho
    k = torch.from_numpy(keep)
    loss = (m2 * _f64(vm))[k].sum() + (con * _f64(vcn))[k].sum() + (dep * _f64(vd))[k].sum() + (op_eff * _f64(vo))[k].sum()
    return torch.autograd.grad(loss, ins + [V]), dict(radii=radii.numpy(), rho=rho.detach().numpy(), op_eff=op_eff.detach().numpy())


@pytest.mark.parametrize("name", ["A", "B"])
def test_host_chain_and_vjp_against_the_reference(aa, name):
    sc = AR.scene(name)
    C, N = sc["viewmats"].shape[0], sc["means"].shape[0]
    got = _host_forward(aa, sc)
    rng = np.random.default_rng(0)
    vm, vcn, vd, vo = rng.standard_normal((C, N, 2)), rng.standard_normal((C, N, 3)), rng.standard_normal((C, N)), rng.standard_normal((C, N))
    same = np.ones((C, N), bool)
    ref, fw = _reference_vjp(sc, vm, vcn, vd, vo, same)
    assert np.array_equal(got["radii"], fw["radii"]) and (fw["radii"] > 0).sum() >= C * N * 0.8
    vis = fw["radii"] > 0
    for k in ("rho", "op_eff"):
        err = (np.abs(got[k] - fw[k])[vis] / fw[k][vis]).max()
        print(f"{name} {k}: max rel err {err:.3g}")
        assert err <= 1e-6 and not got[k][~vis].any(), (k, err)
    hv, sums = _host_backward(aa, sc, fw["radii"], vm, vcn, vd, vo)
    for nm, a, b in zip(AR.GEO, hv, ref[:4]):
        b = b.numpy()
        assert np.isfinite(a).all(), nm
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{name} v_{nm}: {err:.3g}")
        assert err <= GRAD_RTOL, (nm, err)
    gv = ref[4].numpy()
    cam = np.concatenate([sums[:, :9].reshape(C, 3, 3), sums[:, 9:, None]], axis=2)
    for c in range(C):
        err = np.abs(cam[c] - gv[c, :3]).max() / np.abs(gv[c, :3]).max()
        print(f"{name} v_viewmats[{c}]: {err:.3g}")
        assert err <= GRAD_RTOL, (c, err)
    # the increment is not a rounding: without v_rho the scales' gradient misses the bound by far
    hv0, _ = _host_backward(aa, sc, fw["radii"], vm, vcn, vd, 0 * vo)
    ref0, _ = _reference_vjp(sc, vm, vcn, vd, 0 * vo, same)
    assert np.abs(hv[2] - hv0[2]).max() > 0.1 * np.abs(ref[2].numpy()).max()
    assert np.abs(hv0[2] - ref0[2].numpy()).max() <= GRAD_RTOL * np.abs(ref0[2].numpy()).max()


def test_classic_instantiation_is_todays_chain_bit_for_bit(aa, hm):
    N, W, H, C, K, deg = 1500, 96, 64, 2, 16, 3
    sc = make_scene(N, W, H, sh_degree=deg, n_views=C, seed=14, k_store=K, scale_range=(0.02, 0.4), dist=3.0)
    got = _host_forward(aa, sc, on=0)
    want = dict(radii=np.zeros((C, N), np.int32), means2d=np.zeros((C, N, 2), np.float32), depths=np.zeros((C, N), np.float32),
                conics=np.zeros((C, N, 3), np.float32), colors=np.zeros((C, N, 3), np.float32), tpg=np.zeros((C, N), np.int32))
    hm.hm_forward(C, N, K, deg, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["shs"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H, 16,
                  F(0.3), F(0.01), F(1e10), F(0.0), _p(want["radii"]), _p(want["means2d"]), _p(want["depths"]), _p(want["conics"]),
                  _p(want["colors"]), _p(want["tpg"]))
    assert (want["radii"] > 0).sum() > N // 2
    for k in ("radii", "means2d", "depths", "conics"):
        assert np.array_equal(got[k], want[k]), k
    vis = want["radii"] > 0
    assert np.array_equal(got["op_eff"][vis], np.broadcast_to(sc["opacities"], (C, N))[vis]) and not got["rho"].any()
    # ... and the antialiased instantiation leaves radii, means2d, depths and conics alone (the host has no FMA contraction to differ by)
    on = _host_forward(aa, sc, on=1)
    for k in ("radii", "means2d", "depths", "conics"):
        assert np.array_equal(on[k], want[k]), k
    rng = np.random.default_rng(2)
    vm, vcn = rng.standard_normal((C, N, 2)).astype(np.float32), rng.standard_normal((C, N, 3)).astype(np.float32)
    vo = rng.standard_normal((C, N)).astype(np.float32)
    vc = np.zeros((C, N, 3), np.float32)
    a, _ = _host_backward(aa, sc, want["radii"], vm, vcn, None, vo, on=0)
    b = [np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 3), np.float32)]
    v_shs = np.zeros((N, K, 3), np.float32)
    hm.hm_backward(C, N, K, deg, _p(sc["means"]), _p(sc["quats"]), _p(sc["scales"]), _p(sc["shs"]), _p(sc["viewmats"]), _p(sc["Ks"]), W, H,
                   F(0.3), F(0.01), F(1e10), _p(want["radii"]), _p(want["colors"]), _p(vm), _p(vcn), _p(vc), _p(b[0]), _p(b[1]), _p(b[2]),
                   _p(v_shs), 0)
    for x, y, nm in zip(a, b, ("means", "quats", "scales")):
        assert np.abs(y).max() > 0 and np.array_equal(x, y), nm


def test_rank_deficient_covariances_through_the_host_build(aa):
    sc = AR.scene("Z")
    d, N = AR.Z_DEGENERATE, sc["means"].shape[0]
    got = _host_forward(aa, sc)
    assert (got["radii"] > 0).all()
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    assert not got["rho"][0, :d].any() and not got["op_eff"][0, :d].any() and (got["rho"][0, d:] > 0.3).all()
    assert (got["extents"][0, :d] < 0).all() and (got["extents"][0, d:] > 0).all()   # (no extent: nothing is listed under tight culling)
    rng = np.random.default_rng(4)
    vm, vcn, vd, vo = rng.standard_normal((1, N, 2)), rng.standard_normal((1, N, 3)), rng.standard_normal((1, N)), rng.standard_normal((1, N))
    hv, sums = _host_backward(aa, sc, got["radii"], vm, vcn, vd, vo)
    for a in hv + [sums]:
        assert np.isfinite(a).all()
    # through rho the gradient is bounded by the guard: |w| <= |v_rho| / (2e-6)
    hv0, _ = _host_backward(aa, sc, got["radii"], vm, vcn, vd, 0 * vo)
    assert np.abs(hv[2][:d] - hv0[2][:d]).max() < 1e9 and not hv[3][:d].any()
    # and where the blend leaves no gradient of the record's opacity (no pixel takes an opacity of 0), rho adds nothing at all
    vo[0, :d] = 0
    hv1, _ = _host_backward(aa, sc, got["radii"], vm, vcn, vd, vo)
    for x, y in zip(hv1[:3], hv0[:3]):
        assert np.array_equal(x[:d], y[:d])


# ---- 3. the front end ----

def _args(n=4):
    return (torch.zeros((n, 3)), torch.ones((n, 4)), torch.ones((n, 3)), torch.ones(n), torch.zeros((n, 1, 3)), torch.eye(4)[None],
            torch.eye(3)[None], 32, 32)


def test_rasterization_refusals():
    from easy_gaussian_splatting_amd.rendering import RASTERIZE_MODES, rasterization
    assert RASTERIZE_MODES == ("classic", "antialiased")
    aa_kw = dict(sh_degree=0, packed=False, rasterize_mode="antialiased")
    with pytest.raises(ValueError, match="rasterize_mode"):
        rasterization(*_args(), sh_degree=0, packed=False, rasterize_mode="mip")
    for bad in (dict(_sh_grads="colors_pre"), dict(_grad_out={}), dict(_view_payload=torch.zeros(64))):
        with pytest.raises(ValueError, match="rasterize_mode"):
            rasterization(*_args(), **aa_kw, **bad)
    for model in ("ortho", "fisheye"):
        with pytest.raises(NotImplementedError, match="gs_project_fwd_aa"):
            rasterization(*_args(), **aa_kw, camera_model=model)
    # CPU tensors in the mode keep raising NotImplementedError (tests/test_capi.py locks it), with the depth modes' wording
    with pytest.raises(NotImplementedError, match="GPU only"):
        rasterization(*_args(), **aa_kw)
    with pytest.raises(NotImplementedError):
        rasterization(*_args(), sh_degree=0, packed=True, rasterize_mode="antialiased")
    # classic on CPU tensors: as ever
    with pytest.raises(RuntimeError, match="GPU only") as e:
        rasterization(*_args(), sh_degree=0, packed=False, rasterize_mode="classic")
    assert not isinstance(e.value, NotImplementedError)


def _model():
    from easy_gaussian_splatting_amd import model as M
    return M.GaussianModel(means=torch.zeros((4, 3)), log_scales=torch.zeros((4, 3)), quats=torch.ones((4, 4)), sh_0=torch.zeros((4, 1, 3)),
                           sh_rest=torch.zeros((4, 3, 3)), logit_opacities=torch.zeros(4), sh_degree=1, white_background=True)


def test_model_passes_its_rasterize_mode_and_old_pickles_are_classic(monkeypatch):
    from easy_gaussian_splatting_amd import model as M
    seen = {}

    def fake(**kw):
        seen.update(kw)
        raise RuntimeError("stop here")
    monkeypatch.setattr(M, "rasterization", fake)
    m = _model()
    data = {"w2c": torch.eye(4), "K": torch.eye(3), "width": 32, "height": 32}
    assert M.GaussianModel.rasterize_mode == "classic" and "rasterize_mode" not in m.__dict__
    with pytest.raises(RuntimeError, match="stop here"):
        m(data)
    assert "rasterize_mode" not in seen   # (the classic call is the call as it was)
    old = pickle.loads(pickle.dumps(m))   # (a checkpoint from before the attribute: nothing in its __dict__)
    assert "rasterize_mode" not in old.__dict__ and old.rasterize_mode == "classic"
    m.rasterize_mode = "antialiased"
    seen.clear()
    with pytest.raises(RuntimeError, match="stop here"):
        m(data)
    assert seen["rasterize_mode"] == "antialiased"
    assert pickle.loads(pickle.dumps(m)).rasterize_mode == "antialiased"


def test_train_step_graph_refuses_what_has_no_fused_kernel_yet():
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph, ViewParallelGraphStep
    data = {"w2c": torch.eye(4), "K": torch.eye(3), "width": 32, "height": 32}
    gt = torch.zeros((32, 32, 3))
    stub = object()   # (every refusal comes before the runner looks at its optimizer or loss)
    m = _model()
    with pytest.raises(ValueError, match="rasterize_mode"):
        TrainStepGraph(m, stub, stub, data, gt, rasterize_mode="mip")
    with pytest.raises(ValueError, match="the model's rasterize_mode is 'classic'"):
        TrainStepGraph(m, stub, stub, data, gt, rasterize_mode="antialiased")
    m.rasterize_mode = "antialiased"
    with pytest.raises(ValueError, match="the model's rasterize_mode is 'antialiased'"):
        TrainStepGraph(m, stub, stub, data, gt, rasterize_mode="classic")
    for explicit in ({}, dict(rasterize_mode="antialiased")):   # (the default is the model's attribute)
        for kw, names in ((dict(mcmc=stub), "gs_project_bwd_adam_mcmc"), (dict(poses=stub), "gs_project_bwd_adam_sums"),
                          (dict(depth=stub), "gs_project_bwd_adam_depth"), (dict(rounds="on"), "rblk")):
            with pytest.raises(ValueError, match=names):
                TrainStepGraph(m, stub, stub, data, gt, **explicit, **kw)
        with pytest.raises(ValueError, match="SUMS"):
            ViewParallelGraphStep(m, stub, stub, data, gt, vp=stub, **explicit)
    for model in ("ortho", "fisheye"):
        with pytest.raises(ValueError):
            TrainStepGraph(m, stub, stub, dict(data, camera_model=model), gt, camera_model=model)
