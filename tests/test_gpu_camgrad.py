"""Camera gradients on the GPU (`rasterization(_camera_grads=True)`, gs_project_bwd_cam): parity of dL/d viewmats with fp64
autograd of the torch oracle over the colour paths, bit-identity of everything else with the ordinary call, the reduction at
scale against an identity that needs no oracle, determinism, a pose-only optimisation and the model-level path.

Bound: the project's gradient contract, 1e-3 of the largest entry against the fp64 oracle (GRAD_RTOL of tests/test_gpu_parity.py,
`_rel` of tests/test_gpu_sh4.py), per camera over the whole [4,4] block.  As in tests/test_gpu_parity.py and
tests/test_gpu_channels.py the upstream gradient is zero on the razor pixels (within 1e-4 of a blend discontinuity, where fp32 and
fp64 may legitimately take different contributor sets)."""
import numpy as np
import pytest
import torch

import sh4_ref
from oracle import c_oracle as CO
from oracle import torch_oracle as TO
from scenes import config_bench_1m, make_scene

pytestmark = pytest.mark.gpu
GRAD_RTOL = 1e-3
GEO = ("means", "quats", "scales", "opacities")
CULLING = ("gsplat", "tight", "gsplat_eager")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _case(kind, C, seed, cameras=None):
    """Scene + colour tensors of one case; `cameras`: (viewmats, Ks) that replace the scene's orbit.  Returns (sc, geometry as
    float32 numpy in the form the GPU call takes, colours as a list of float32 numpy leaves, kwargs of rasterization, the
    activated fp64 scales / opacities of the oracle)."""
    W, H, N = 160, 112, 3000
    deg = {"sh0": 0, "sh3": 3, "sh3_split_act": 3, "sh4": 4}.get(kind)
    sc = make_scene(N, W, H, sh_degree=deg if deg is not None else 0, n_views=C, seed=seed, scale_range=(0.02, 0.2), dist=4.0)
    if cameras is not None:
        sc["viewmats"], sc["Ks"] = cameras
    geo = {k: sc[k] for k in GEO}
    kw = dict(sh_degree=deg)
    if kind == "sh3_split_act":   # the model's raw parameters and its two SH tensors
        op = np.clip(sc["opacities"], 1e-4, 1 - 1e-4)
        geo["scales"], geo["opacities"] = np.log(sc["scales"]).astype(np.float32), np.log(op / (1 - op)).astype(np.float32)
        kw["_activations"] = "exp_sigmoid"
        cols = [np.ascontiguousarray(sc["shs"][:, :1]), np.ascontiguousarray(sc["shs"][:, 1:])]
        act = (np.exp(geo["scales"].astype(np.float64)), 1.0 / (1.0 + np.exp(-geo["opacities"].astype(np.float64))))
    else:
        act = (sc["scales"].astype(np.float64), sc["opacities"].astype(np.float64))
        if deg is None:
            D = int(kind[-1])
            cols = [np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)]
            sc["backgrounds"] = np.random.default_rng(seed + 1).random((C, D)).astype(np.float32)
        else:
            cols = [sc["shs"]]
    return sc, geo, cols, kw, act


def _upstream(sc, act, D, seed):
    """Random upstream gradients of the image and the alphas, zero on the razor pixels (the contributor sets do not depend on
    the colours)."""
    W, H = int(sc["width"]), int(sc["height"])
    fw = CO.render(sc["means"], sc["quats"], act[0], act[1], np.zeros((sc["means"].shape[0], 3)), sc["viewmats"], sc["Ks"], W, H,
                   sh_degree=None, dtype=np.float64)
    razor = CO.blend_margin(fw, mu_tol_ulps=1.0, conic_rtol=2.4e-7) < 1e-4
    assert razor.mean() < 0.05, razor.mean()
    g = torch.Generator().manual_seed(seed)
    keep = torch.from_numpy(~razor).double()[..., None]
    C = razor.shape[0]
    return torch.randn((C, H, W, D), generator=g, dtype=torch.float64) * keep, torch.randn((C, H, W, 1), generator=g, dtype=torch.float64) * keep


def _gpu(sc, geo, cols, kw, vc, va, cam, culling="gsplat"):
    """One forward + backward on the GPU.  cam: viewmats requires grad and `_camera_grads=True`; otherwise the call as it is made
    without the feature."""
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = _dev()
    ins = [torch.from_numpy(np.ascontiguousarray(geo[k])).to(d).requires_grad_(True) for k in GEO]
    leaves = [torch.from_numpy(c).to(d).requires_grad_(True) for c in cols]
    V = torch.from_numpy(sc["viewmats"]).to(d).requires_grad_(cam)
    extra = dict(_camera_grads=True) if cam else {}
    img, alpha, meta = rasterization(*ins, tuple(leaves) if len(leaves) == 2 else leaves[0], V, torch.from_numpy(sc["Ks"]).to(d),
                                     int(sc["width"]), int(sc["height"]), packed=False, backgrounds=torch.from_numpy(sc["backgrounds"]).to(d),
                                     absgrad=True, _tile_culling=culling, **kw, **extra)
    loss = (img * vc.to(d).float()).sum() + (alpha * va.to(d).float()).sum()
    gs = torch.autograd.grad(loss, ins + leaves + ([V] if cam else []))
    torch.cuda.synchronize()
    out = dict(img=img.detach(), alpha=alpha.detach(), radii=meta["radii"], absgrad=meta["means2d"].absgrad,
               grads=list(gs[:len(ins) + len(leaves)]))
    if cam:
        out["v_viewmats"] = gs[-1]
    return out


def _assert_nothing_else_moves(a, b):
    """Image, alphas, radii, every other gradient and .absgrad: bit-identical with and without camera gradients."""
    for k in ("img", "alpha", "radii", "absgrad"):
        assert torch.equal(a[k], b[k]), k
    assert len(a["grads"]) == len(b["grads"])
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert torch.equal(x, y), f"gradient {i}"


def _check_cameras(got, ref):
    got, ref = got.detach().cpu().double().numpy(), ref.numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    for c in range(ref.shape[0]):   # per camera, all 16 entries
        print(f"camera {c}: rel err of v_viewmats {_rel(got[c], ref[c]):.3g} (largest entry {np.abs(ref[c]).max():.4g})")
    for c in range(ref.shape[0]):
        assert _rel(got[c], ref[c]) < GRAD_RTOL, (c, _rel(got[c], ref[c]))
    return [_rel(got[c], ref[c]) for c in range(ref.shape[0])]


def _oracle_v_viewmats(sc, cols, kw, act, vc, va):
    """dL/d viewmats by fp64 autograd of the torch oracle (SH up to degree 3, or colour features)."""
    f64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    V = f64(sc["viewmats"]).requires_grad_(True)
    colors64 = torch.cat([f64(c) for c in cols], dim=1) if len(cols) == 2 else f64(cols[0])
    img, alpha, _ = TO.rasterization(f64(sc["means"]), f64(sc["quats"]), f64(act[0]), f64(act[1]), colors64, V, f64(sc["Ks"]),
                                     int(sc["width"]), int(sc["height"]), sh_degree=kw["sh_degree"], packed=False,
                                     backgrounds=f64(sc["backgrounds"]))
    (ref,) = torch.autograd.grad((img * vc).sum() + (alpha * va).sum(), V)
    if kw["sh_degree"] is not None and kw["sh_degree"] >= 1:
        assert float(ref[:, 3].abs().max()) > 0   # (the inverse's VJP reaches the bottom row, as gsplat's torch.inverse does)
    return ref


def _oracle_v_viewmats_degree4(sc, act, vc, va):
    """The oracle's SH stops at degree 3: the degree-4 colours restated in fp64 torch (tests/sh4_ref.py) with the camera centre
    under autograd, fed to the oracle as [C,N,3] features of the same `viewmats` leaf."""
    f64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    V = f64(sc["viewmats"]).requires_grad_(True)
    campos = torch.linalg.inv(V)[:, :3, 3]
    means64 = f64(sc["means"])
    feats = sh4_ref.sh_colors(f64(sc["shs"]), means64, campos, 4)   # [C,N,3]  (culled Gaussians are in no list: no gradient)
    img, alpha, _ = TO.rasterization(means64, f64(sc["quats"]), f64(act[0]), f64(act[1]), feats, V, f64(sc["Ks"]),
                                     int(sc["width"]), int(sc["height"]), sh_degree=None, packed=False, backgrounds=f64(sc["backgrounds"]))
    (ref,) = torch.autograd.grad((img * vc).sum() + (alpha * va).sum(), V)
    return ref


KINDS = ("sh0", "sh3", "sh3_split_act", "feat1", "feat3", "feat4")


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_view_matrix_gradient_matches_the_oracle_and_nothing_else_moves(kind, C):
    i = KINDS.index(kind)
    sc, geo, cols, kw, act = _case(kind, C, seed=60 + 2 * i + C)
    D = cols[0].shape[-1] if kw["sh_degree"] is None else 3
    vc, va = _upstream(sc, act, D, seed=i)
    culling = CULLING[(i + C) % 3]   # (all three list modes, with one and with two cameras)
    with_cam = _gpu(sc, geo, cols, kw, vc, va, True, culling)
    plain = _gpu(sc, geo, cols, kw, vc, va, False, culling)
    _assert_nothing_else_moves(with_cam, plain)

    ref = _oracle_v_viewmats(sc, cols, kw, act, vc, va)
    _check_cameras(with_cam["v_viewmats"], ref)


@pytest.mark.parametrize("C", [1, 2])
def test_view_matrix_gradient_at_degree4(C):
    sc, geo, cols, kw, act = _case("sh4", C, seed=80 + C)
    vc, va = _upstream(sc, act, 3, seed=4)
    with_cam = _gpu(sc, geo, cols, kw, vc, va, True)
    plain = _gpu(sc, geo, cols, kw, vc, va, False)
    _assert_nothing_else_moves(with_cam, plain)

    ref = _oracle_v_viewmats_degree4(sc, act, vc, va)
    _check_cameras(with_cam["v_viewmats"], ref)


def _bench_geometry_call(retain=False):
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = _dev()
    sc = config_bench_1m()
    t = {k: torch.from_numpy(v).to(d) for k, v in sc.items() if isinstance(v, np.ndarray)}
    means = t["means"].clone().requires_grad_(True)
    V = t["viewmats"].clone().requires_grad_(True)
    img, _, _ = rasterization(means, t["quats"], t["scales"], t["opacities"], t["shs"][:, :1].contiguous(), V, t["Ks"],
                              int(sc["width"]), int(sc["height"]), sh_degree=0, packed=False, backgrounds=t["backgrounds"],
                              _camera_grads=True)
    vc = torch.randn(img.shape, generator=torch.Generator().manual_seed(2)).to(d)
    return (img * vc).sum(), means, V


def test_translation_gradient_identity_at_one_million_gaussians():
    """Degree-0 colours: every dependence on `means` and on t goes through p_c = A p + t, so v_viewmats[0,:3,3] = A sum_n v_means[n]
    -- no oracle needed.  Each fp32 v_means entry carries a rounding of 2^-24 relative and the fp32 A is orthonormal to a few
    2^-24, so |difference| <= 8 * 2^-24 * sum_n |v_means[n]|_1 per component.  Catches a reduction that drops blocks, double
    counts the tail block (1 M is not a multiple of the block size) or sums in fp32."""
    loss, means, V = _bench_geometry_call()
    v_means, v_V = torch.autograd.grad(loss, (means, V))
    torch.cuda.synchronize()
    assert means.shape[0] == 1_000_000 and means.shape[0] % 256 != 0
    A = V.detach()[0, :3, :3].double().cpu()
    vm = v_means.double().cpu()
    want = A @ vm.sum(0)
    got = v_V[0, :3, 3].double().cpu()
    bound = 8 * 2.0 ** -24 * float(vm.abs().sum())
    print(f"v_t {got.tolist()}  A sum v_means {want.tolist()}  |diff| {(got - want).abs().tolist()}  bound {bound:.4g}  "
          f"sum |v_means|_1 / |v_t|_inf {float(vm.abs().sum()) / float(want.abs().max()):.1f}")
    assert float(want.abs().max()) > 0 and torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= bound, ((got - want).abs().tolist(), bound)
    assert float(v_V[0, 3].abs().max()) == 0.0   # (no SH direction: nothing reaches the bottom row)


def test_two_backward_passes_give_the_same_bits():
    loss, means, V = _bench_geometry_call()
    a = torch.autograd.grad(loss, V, retain_graph=True)[0].clone()
    b = torch.autograd.grad(loss, V)[0]
    torch.cuda.synchronize()
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    # SH degree 3, two cameras: the direction part and the per-camera partials as well
    sc, geo, cols, kw, act = _case("sh3", 2, seed=9)
    vc, va = _upstream(sc, act, 3, seed=1)
    r1 = _gpu(sc, geo, cols, kw, vc, va, True)["v_viewmats"]
    r2 = _gpu(sc, geo, cols, kw, vc, va, True)["v_viewmats"]
    assert torch.equal(r1, r2)


def test_pose_only_optimisation_recovers_a_perturbed_camera():
    """Frozen scene, the six numbers of one CameraDeltas row the only leaf.  On the CPU with the oracle alone this goes from
    1.18 deg / 0.0539 to 0.009 deg / 0.0003 (loss 0.071 -> 0.0007); the condition -- a tenth of the start in rotation, translation
    and loss -- separates "works" from "wrong sign / missing term", not rounding."""
    from easy_gaussian_splatting_amd.pose import CameraDeltas
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = _dev()
    W, H = 96, 64
    sc = make_scene(600, W, H, sh_degree=0, seed=5, scale_range=(0.02, 0.2), dist=4.0)
    t = {k: torch.from_numpy(v).to(d) for k, v in sc.items() if isinstance(v, np.ndarray)}

    def render(viewmats, **kw):
        return rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["shs"], viewmats, t["Ks"], W, H, sh_degree=0,
                             packed=False, backgrounds=t["backgrounds"], **kw)[0].clamp(0.0, 1.0)

    with torch.no_grad():
        target = render(t["viewmats"])
    cd = CameraDeltas(1).to(d)
    with torch.no_grad():
        cd.deltas[0] = torch.tensor([0.01, -0.015, 0.01, 0.03, -0.02, 0.04], device=d)
    err = lambda: (float(cd.deltas.detach()[0, :3].norm()), float(cd.deltas.detach()[0, 3:].norm()))
    rot0, tr0 = err()
    assert abs(np.degrees(rot0) - 1.18) < 0.01 and abs(tr0 - 0.0539) < 1e-4
    opt = torch.optim.Adam(cd.parameters(), lr=2e-3)
    losses = []
    for _ in range(120):
        opt.zero_grad()
        loss = (render(cd(t["viewmats"][0], 0)[None], _camera_grads=True) - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float((render(cd(t["viewmats"][0], 0)[None]) - target).abs().mean())
    rot1, tr1 = err()
    print(f"rotation {np.degrees(rot0):.3f} -> {np.degrees(rot1):.4f} deg, translation {tr0:.4f} -> {tr1:.5f}, loss {losses[0]:.4f} -> {final:.5f}")
    assert rot1 <= 0.1 * rot0 and tr1 <= 0.1 * tr0, (rot0, rot1, tr0, tr1)
    assert final < 0.1 * losses[0], (losses[0], final)


def _model(n=4000, W=128, H=96):
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
    d = _dev()
    sc = make_scene(n, W, H, sh_degree=3, n_views=1, seed=3, scale_range=(0.01, 0.08), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"]) * 0.5
    m = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=shs[:, :1].contiguous(),
                      sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                      white_background=True).to(d)
    opt = build_optimizers(m, 1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2, fused="hip")
    data = {"w2c": T(sc["viewmats"][0]).to(d), "K": T(sc["Ks"][0]).to(d), "width": W, "height": H}
    return m, opt, data


def test_model_forward_hands_the_gradient_to_camera_deltas():
    from easy_gaussian_splatting_amd.pose import CameraDeltas
    from easy_gaussian_splatting_amd.rendering import rasterization
    m, _, data = _model()
    d = _dev()
    cd = CameraDeltas(2).to(d)
    with torch.no_grad():
        cd.deltas[1] = torch.tensor([0.004, -0.002, 0.003, 0.01, 0.02, -0.01], device=d)
    vc = torch.randn((data["height"], data["width"], 3), generator=torch.Generator().manual_seed(0)).to(d)
    out = m({**data, "w2c": cd(data["w2c"], 1)}, clamp=False)
    (out["render_img"] * vc).sum().backward()
    g = cd.deltas.grad.clone()
    assert torch.isfinite(g).all() and float(g[1].abs().min()) > 0 and float(g[0].abs().max()) == 0
    assert all(getattr(m, k).grad is not None for k in m.param_names)   # (the scene's gradients arrive as before)
    # the same through rasterization() directly, on the model's own tensors
    cd.deltas.grad = None
    img, _, _ = rasterization(m.means, m.quats, m.log_scales, m.logit_opacities, (m.sh_0, m.sh_rest), cd(data["w2c"], 1)[None],
                              data["K"][None], data["width"], data["height"], sh_degree=m.active_sh_degree, packed=False,
                              backgrounds=m.BACKGROUND[None], _activations="exp_sigmoid", _tile_culling="tight", _camera_grads=True)
    (img[0] * vc).sum().backward()
    assert _rel(g[1].cpu().numpy(), cd.deltas.grad[1].cpu().numpy()) < GRAD_RTOL


def test_train_step_graph_refuses_a_camera_that_requires_grad():
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    m, opt, data = _model()
    gt = torch.rand((data["height"], data["width"], 3), generator=torch.Generator().manual_seed(1)).to(_dev())
    lc = LossComputer(0.2, clamp_input=True)
    live = {**data, "w2c": data["w2c"].clone().requires_grad_(True)}
    with pytest.raises(ValueError, match="w2c"):
        TrainStepGraph(m, opt, lc, live, gt)
    runner = TrainStepGraph(m, opt, lc, data, gt)
    with pytest.raises(ValueError, match="w2c"):
        runner.step(live, gt)
    runner.step(data, gt)   # (and it still steps on a constant camera)
    runner.finish()
    assert runner.report()["steps"] == 1
