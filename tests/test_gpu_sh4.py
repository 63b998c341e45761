"""Spherical harmonics of degree 4 (25 coefficients) on the GPU: parity with the oracle (whose SH stops at degree 3, so the
degree-4 colours are restated here, tests/sh4_ref.py, and fed to the oracle's blend as colour features), K = 25 storage at a
lower active degree against compact storage, the captured train step against the eager loop, the view-parallel SH kernels
and a checkpoint round trip."""
import numpy as np
import pytest
import torch

import sh4_ref
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.rendering import rasterization, sh_grad_views
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from oracle import c_oracle as CO
from scenes import make_scene

pytestmark = pytest.mark.gpu
LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("C,split,act", [(1, False, "none"), (2, True, "none"), (1, True, "exp_sigmoid"), (2, False, "exp_sigmoid")])
def test_degree4_matches_the_oracle(C, split, act):
    """rasterization(sh_degree=4) against the fp64 oracle: projection and blend from oracle.c_oracle, the degree-4 colours (and
    their clamp) restated in fp64 torch and differentiated by autograd -- image to 1e-4 off the razor pixels, all gradients
    (.absgrad included) to 1e-3 relative."""
    dev = _dev()
    W, H, N = 160, 112, 3000
    sc = make_scene(N, W, H, sh_degree=4, n_views=C, seed=40 + C, scale_range=(0.02, 0.2), dist=4.0)
    assert sc["shs"].shape == (N, 25, 3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
    raw_sc, raw_op = sc["scales"], sc["opacities"]
    if act == "exp_sigmoid":   # the model's raw parameters, activated inside the kernels
        op = np.clip(sc["opacities"], 1e-4, 1 - 1e-4)
        raw_sc, raw_op = np.log(sc["scales"]).astype(np.float32), np.log(op / (1 - op)).astype(np.float32)
    ins = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (sc["means"], sc["quats"], raw_sc, raw_op)]
    if split:
        sh = (t["shs"][:, :1].contiguous().requires_grad_(True), t["shs"][:, 1:].contiguous().requires_grad_(True))
        colors, sh_leaves = sh, list(sh)
    else:
        colors = t["shs"].clone().requires_grad_(True)
        sh_leaves = [colors]
    img, alpha, meta = rasterization(*ins, colors, t["viewmats"], t["Ks"], W, H, sh_degree=4, packed=False,
                                     backgrounds=t["backgrounds"], absgrad=True, _activations=act)
    vc = torch.randn(img.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    grads = torch.autograd.grad((img * vc).sum(), ins + sh_leaves)
    torch.cuda.synchronize()

    # oracle: fp64 activations, the SH colours as features, the oracle's projection + blend
    f64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    means64, shs64 = f64(sc["means"]).requires_grad_(True), f64(sc["shs"]).requires_grad_(True)
    scales64 = f64(sc["scales"]) if act == "none" else torch.exp(f64(raw_sc))
    opac64 = f64(sc["opacities"]) if act == "none" else torch.sigmoid(f64(raw_op))
    vm64 = f64(sc["viewmats"])
    campos = torch.linalg.inv(vm64)[:, :3, 3]
    cols64 = sh4_ref.sh_colors(shs64, means64, campos, 4)                        # [C,N,3]
    fw = CO.render(sc["means"], sc["quats"], scales64.numpy(), opac64.numpy(), cols64.detach().numpy(), sc["viewmats"], sc["Ks"],
                   W, H, sh_degree=None, backgrounds=sc["backgrounds"], dtype=np.float64)
    assert fw["colors"].shape == (C, N, 3)
    bw = CO.backward(fw, vc.cpu().numpy().astype(np.float64))
    vis = torch.from_numpy(fw["radii"] > 0)
    v_cols = torch.from_numpy(bw["v_colors"]) * vis[..., None]   # (culled Gaussians: no colour, no gradient -- gsplat's masks)
    v_shs, v_mdir = torch.autograd.grad(cols64, (shs64, means64), v_cols)
    ref = {"means": bw["v_means"] + v_mdir.numpy(), "quats": bw["v_quats"], "scales": bw["v_scales"], "opacities": bw["v_opacities"]}
    if act == "exp_sigmoid":
        ref["scales"] = ref["scales"] * scales64.numpy()
        o = opac64.numpy()
        ref["opacities"] = ref["opacities"] * o * (1 - o)
    ref["shs"] = v_shs.numpy()

    err = np.abs(img.detach().cpu().numpy() - fw["render_colors"]).max(-1)
    assert np.array_equal(meta["radii"].cpu().numpy(), fw["radii"]), "radii differ from the oracle's"
    razor = CO.blend_margin(fw, mu_tol_ulps=1.0, conic_rtol=2.4e-7) < 1e-4
    assert razor.mean() < 0.01, razor.mean()
    assert err[~razor].max() <= 1e-4, err[~razor].max()
    names = ["means", "quats", "scales", "opacities"]
    for name, g in zip(names, grads[:4]):
        assert _rel(g.cpu().numpy(), ref[name]) < 1e-3, (name, _rel(g.cpu().numpy(), ref[name]))
    g_sh = torch.cat([g.cpu() for g in grads[4:]], dim=1).numpy()
    assert g_sh.shape == (N, 25, 3)
    assert _rel(g_sh, ref["shs"]) < 1e-3, _rel(g_sh, ref["shs"])
    assert _rel(meta["means2d"].absgrad.cpu().numpy(), bw["v_means2d_abs"]) < 1e-3


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_k25_storage_equals_compact_storage(deg, split):
    """The degree schedule: K = 25 stored, degree d active, must render and differentiate exactly like K = (d+1)^2 storage."""
    dev = _dev()
    W, H, N = 176, 112, 2500
    sc = make_scene(N, W, H, sh_degree=4, n_views=2, seed=7 + deg, scale_range=(0.03, 0.2), dist=4.0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
    vc = torch.randn((2, H, W, 3), generator=torch.Generator().manual_seed(deg)).to(dev)
    ka = (deg + 1) ** 2

    def run(K):
        ins = [t[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")]
        shs = t["shs"][:, :K].contiguous()
        leaves = [shs[:, :1].contiguous().requires_grad_(True), shs[:, 1:].contiguous().requires_grad_(True)] if split else \
            [shs.requires_grad_(True)]
        colors = tuple(leaves) if split else leaves[0]
        img, alpha, meta = rasterization(*ins, colors, t["viewmats"], t["Ks"], W, H, sh_degree=deg, packed=False,
                                         backgrounds=t["backgrounds"], absgrad=True)
        gs = torch.autograd.grad((img * vc).sum() + alpha.sum(), ins + leaves, allow_unused=True)
        gsh = [torch.zeros_like(x) if g is None else g for g, x in zip(gs[4:], leaves)]
        return img, alpha, gs[:4], torch.cat(gsh, dim=1) if split else gsh[0], meta["means2d"].absgrad

    i_c, a_c, g_c, sh_c, ab_c = run(ka)
    i_f, a_f, g_f, sh_f, ab_f = run(25)
    assert torch.equal(i_c, i_f) and torch.equal(a_c, a_f) and torch.equal(ab_c, ab_f)
    for x, y in zip(g_c, g_f):
        assert torch.equal(x, y)
    assert sh_f.shape == (N, 25, 3)
    assert torch.equal(sh_f[:, :ka], sh_c[:, :ka]) and float(sh_f[:, ka:].abs().max()) == 0.0


def _setup(n=12000, W=256, H=176, n_views=3, seed=3, sh_degree=4):
    dev = _dev()
    sc = make_scene(n, W, H, sh_degree=sh_degree, n_views=n_views, seed=seed, scale_range=(0.01, 0.08), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"]) * 0.5

    def make():
        m = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]),
                          sh_0=shs[:, :1].contiguous(), sh_rest=shs[:, 1:].contiguous(),
                          logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=sh_degree, white_background=True,
                          means_lr_schedule_max_steps=40).to(dev)
        return m, build_optimizers(m, *LRS, fused="hip")

    datas = [{"w2c": T(sc["viewmats"][v]).to(dev), "K": T(sc["Ks"][v]).to(dev), "width": W, "height": H} for v in range(n_views)]
    g = torch.Generator().manual_seed(11)
    gts = [torch.rand((H, W, 3), generator=g).to(dev) for _ in range(n_views)]
    return dev, make, datas, gts


def _eager_step(model, opt, lc, data, gt):
    out = model(data, clamp=False)
    loss = lc.get_loss_dict(out["render_img"], gt, None)
    loss["total"].backward()
    model.update_statistics(data, out)
    opt.step()
    opt.zero_grad()
    return torch.stack([loss["l1"].detach(), loss["ssim"].detach(), loss["total"].detach()])


def _assert_same(ma, oa, mb, ob, what=""):
    for k in ma.param_names:
        assert torch.equal(getattr(ma, k).detach(), getattr(mb, k).detach()), (what, k)
        for x, y in zip(oa.moments_of(getattr(ma, k)), ob.moments_of(getattr(mb, k))):
            assert torch.equal(x, y), (what, k, "moment")
    for k in ("max_radii", "grad_norm_accum", "collecting_counts"):
        assert torch.equal(getattr(ma, k), getattr(mb, k)), (what, k)
    assert oa._step == ob._step


@pytest.mark.parametrize("rounds", ["off", "on"])
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_captured_step_equals_eager_step_at_degree4(fuse_adam, rounds, monkeypatch):
    monkeypatch.setenv("GS_ROUNDS", rounds)
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    assert ma.active_sh_degree == 4 and ma.sh_rest.shape[1] == 24 and oa.flat_param.numel() > 0
    lc = LossComputer(0.2, clamp_input=True)
    runner = TrainStepGraph(mb, ob, lc, datas[0], gts[0], None, check_every=2, fuse_adam=fuse_adam)
    for it in range(5):
        v = it % 3
        ma.update_learning_rate(it); mb.update_learning_rate(it)
        l_ref = _eager_step(ma, oa, lc, datas[v], gts[v])
        out = runner.step(datas[v], gts[v])
        runner.finish()
        assert torch.equal(out["loss3"], l_ref), it
        _assert_same(ma, oa, mb, ob, f"step {it}")
    rep = runner.report()
    assert rep["steps"] == 5 and rep["overflows"] == 0 and rep["captures"] == 1


def test_degree_schedule_0_to_4_with_refinement_in_the_captured_step():
    """K = 25 from step 0, the active degree climbing 0 -> 4 (re-capture at every change), a densify_and_prune at K = 25 on
    the way: the captured step stays the eager loop bit for bit."""
    dev, make, datas, gts = _setup(n=8000)
    (ma, oa), (mb, ob) = make(), make()
    for m in (ma, mb):
        m.active_sh_degree = 0
        m.DENSIFY_GRAD_THRESH = 0.0
    lc = LossComputer(0.2, clamp_input=True)
    runner = TrainStepGraph(mb, ob, lc, datas[0], gts[0], check_every=3)
    it = 0
    for deg in range(5):
        assert ma.active_sh_degree == mb.active_sh_degree == deg
        for _ in range(2):
            _eager_step(ma, oa, lc, datas[it % 3], gts[it % 3]); runner.step(datas[it % 3], gts[it % 3])
            it += 1
        runner.finish()
        _assert_same(ma, oa, mb, ob, f"degree {deg}")
        if deg == 2:
            n0 = ma.nbr_gaussians
            for m in (ma, mb):
                m.densify_and_prune(generator=torch.Generator(device=dev).manual_seed(5))
            assert ma.nbr_gaussians == mb.nbr_gaussians > n0 and ma.sh_rest.shape[1] == 24
            _assert_same(ma, oa, mb, ob, "after densify")
        ma.up_sh_degree(); mb.up_sh_degree()
    assert ma.active_sh_degree == 4
    assert runner.report()["rebuilds"] >= 5


def _sh_grad_views_check(sc, deg, split, **proj):
    """The view-parallel step's SH rebuild (gs_sh_grad_views) against the dense projection backward on scene `sc`."""
    dev = _dev()
    W, H, C, K = int(sc["width"]), int(sc["height"]), sc["viewmats"].shape[0], sc["shs"].shape[1]
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
    vc = torch.randn((C, H, W, 3), generator=torch.Generator().manual_seed(1)).to(dev)

    def run(mode):
        ins = [t[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")]
        sh0 = t["shs"][:, :1].contiguous().requires_grad_(True)
        shr = t["shs"][:, 1:].contiguous().requires_grad_(True)
        shs = t["shs"].clone().requires_grad_(True)
        img, _, meta = rasterization(*ins, (sh0, shr) if split else shs, t["viewmats"], t["Ks"], W, H, sh_degree=deg,
                                     packed=False, backgrounds=t["backgrounds"], absgrad=True, _sh_grads=mode, **proj)
        (img * vc).sum().backward()
        return [p.grad for p in ins], ((sh0.grad, shr.grad) if split else (shs.grad,)), meta

    g_dense, sh_dense, _ = run("dense")
    g_fact, _, meta = run("colors_pre")
    for a, b in zip(g_fact, g_dense):
        assert _rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-6
    rebuilt = sh_grad_views(t["means"], t["viewmats"], meta["means2d"].colors_pre_grad, deg, K, split=split)
    rebuilt = rebuilt if split else (rebuilt,)
    for a, b in zip(rebuilt, sh_dense):
        assert a.shape == b.shape and float(b.abs().max()) > 0
        assert _rel(a.cpu().numpy(), b.cpu().numpy()) < 2e-6


@pytest.mark.parametrize("split", [False, True])
def test_sh_grad_views_at_degree4_matches_dense_path(split):
    """The view-parallel step's SH rebuild (gs_sh_grad_views) at degree 4 equals the dense projection backward."""
    _sh_grad_views_check(make_scene(2500, 176, 112, sh_degree=4, n_views=3, seed=35, scale_range=(0.03, 0.2), dist=4.0), 4, split)


def _identity_rotation_cameras(R, g):
    cams = torch.eye(4).repeat(R, 1, 1)
    cams[:, :3, 3] = torch.randn((R, 3), generator=g) + torch.tensor([0.0, 0.0, 6.0])
    return cams


def _sh_adam_views_check(deg, cams=None, K=25):
    """gs_sh_adam_views (SH rebuild over the views' records + Adam in one launch) against sh_grad_views followed by FusedAdam,
    two steps, bit for bit.  `cams` [R,4,4]: the view matrices of the records (default: identity rotations)."""
    from easy_gaussian_splatting_amd import _native as nat
    from easy_gaussian_splatting_amd.optim import FusedAdam
    dev = _dev()
    N, R = 3001, 2
    g = torch.Generator().manual_seed(5 + deg)
    means = (torch.rand((N, 3), generator=g) * 2 - 1).to(dev)
    cams = (_identity_rotation_cameras(R, g) if cams is None else cams).to(dev)
    assert cams.shape == (R, 4, 4)

    def make():
        gg = torch.Generator().manual_seed(11)
        ps = {"sh_0": torch.nn.Parameter(torch.randn((N, 1, 3), generator=gg).to(dev)),
              "sh_rest": torch.nn.Parameter(torch.randn((N, K - 1, 3), generator=gg).to(dev)),
              "means": torch.nn.Parameter(means.clone())}
        return ps, FusedAdam([{"params": [p], "lr": 1e-2 * (i + 1), "name": k} for i, (k, p) in enumerate(ps.items())])

    pa, oa = make()
    pb, ob = make()
    rad_a, rad_b = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    P = 4 * N + 16
    for it in range(2):
        rec = torch.zeros((R, P), device=dev)
        pre = torch.randn((R, N, 3), generator=g).to(dev)
        pre[torch.rand((R, N), generator=g).to(dev) < 0.3] = 0.0
        rad = torch.rand((R, N), generator=g).to(dev)
        rec[:, :3 * N] = pre.reshape(R, -1); rec[:, 3 * N:4 * N] = rad; rec[:, 4 * N:] = cams.reshape(R, 16)
        v0, vr = sh_grad_views(means, cams, pre, deg, K)
        pa["sh_0"].grad, pa["sh_rest"].grad = v0, vr
        oa.step(only=("sh_0", "sh_rest"), grad_scale=1.0 / R)
        torch.maximum(rad_a, rad.max(0).values, out=rad_a)
        ob._step += 1
        m0, s0 = ob.moments_of(pb["sh_0"]); mr, sr = ob.moments_of(pb["sh_rest"])
        nat.check(nat.lib().gs_sh_adam_views(torch.cuda.current_stream().cuda_stream, R, N, K, deg, means.data_ptr(), rec.data_ptr(), P,
                                             pb["sh_0"].data_ptr(), m0.data_ptr(), s0.data_ptr(), pb["sh_rest"].data_ptr(), mr.data_ptr(),
                                             sr.data_ptr(), 1e-2, 2e-2, 0.9, 0.999, 1e-8, ob._step, 1.0 / R, rad_b.data_ptr()),
                  "gs_sh_adam_views")
    for k in ("sh_0", "sh_rest"):
        assert torch.equal(pa[k].detach(), pb[k].detach()), k
        for x, y in zip(oa.moments_of(pa[k]), ob.moments_of(pb[k])):
            assert torch.equal(x, y), k
    assert torch.equal(rad_a, rad_b)


@pytest.mark.parametrize("deg", [4, 2])
def test_sh_adam_views_at_k25_equals_rebuild_plus_adam(deg):
    _sh_adam_views_check(deg)


def test_degree4_checkpoint_round_trip(tmp_path):
    from easy_gaussian_splatting_amd import checkpoint as ckpt
    dev, make, datas, gts = _setup(n=4000)
    m, opt = make()
    lc = LossComputer(0.2, clamp_input=True)
    for it in range(3):
        _eager_step(m, opt, lc, datas[it], gts[it])
    ckpt.save_gaussian_model(tmp_path / "checkpoints" / "iterations_3.pth", m, save_optimizer=True)
    b = ckpt.load_gaussian_model(tmp_path, 3, device="cuda:0", optimizer="hip")
    assert b.MAX_SH_DEGREE == 4 and b.active_sh_degree == m.active_sh_degree == 4 and b.sh_rest.shape == (m.nbr_gaussians, 24, 3)
    for k in m.param_names:
        assert torch.equal(getattr(m, k).detach(), getattr(b, k).detach()), k
    with torch.no_grad():
        ia, ib = m(datas[0])["render_img"], b(datas[0])["render_img"]
    assert torch.equal(ia, ib)
