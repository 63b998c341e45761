"""`rasterization(rasterize_mode="antialiased")` on the GPU (gs_project_fwd_aa, gs_project_bwd_aa, gs_project_bwd_cam_aa,
gs_project_bwd_adam_aa, gs_project_bwd_adam_reg_aa) against the fp64 reference composed in tests/antialias_ref.py.

Bounds: those of tests/test_gpu_camera_models.py -- colours and alphas 1e-4 abs outside the razor pixels (within 1e-4 of a blend
discontinuity; at most 1 % of the frame: checked on the reference alone when a scene is first used), each gradient within 1e-3 of its
tensor's largest reference magnitude with the upstream gradient zeroed on the razor pixels, view-matrix gradients 1e-3 of the largest
entry per camera.  rho >= 1e-2 in scenes A and B, so the 1e-6 guard of the backward moves a gradient by at most 1e-4 relative.
`meta["opacities"]` is held to the reference's op_eff to 1e-6 relative: rho rounded to fp32 (6e-8), its product with the opacity
(6e-8), and with in-kernel activations the sigmoid's expf and reciprocal (a few 1e-7 together).
radii, means2d, conics and depths are the classic call's bit for bit.  The captured step is held to the eager loop as
tests/test_gpu_camera_models.py and tests/test_gpu_scale_reg.py hold theirs."""
import functools

import numpy as np
import pytest
import torch

import antialias_ref as AR
from test_gpu_depth import _check_forward as _check_depth_forward

pytestmark = pytest.mark.gpu
FWD_ATOL = 1e-4
GRAD_RTOL = 1e-3
RAZOR_SHARE = 0.01
OPEFF_RTOL = 1e-6


def _rel(got, ref):
    ref = ref.double()
    return ((got.detach().cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc = AR.scene(name)
    rz = AR.razor(sc)
    assert rz.mean() <= RAZOR_SHARE, (name, rz.mean())
    return sc, rz


def _check(name, out, ref, rz, n_leaves, cam=False, depth_mode=None):
    C, N = ref["radii"].shape
    vis = ref["radii"] > 0
    print(f"{name}: {int(vis.sum())}/{C * N} visible, razor share {rz.mean():.4%}, rho {float(ref['rho'][vis].min()):.3g} .. {float(ref['rho'][vis].max()):.4g}")
    assert int(vis.sum()) >= C * N // 2
    assert torch.equal(out["meta"]["radii"].cpu(), ref["radii"])
    op = out["meta"]["opacities"].cpu().double()
    assert op.shape == (C, N) and bool((op[~vis] == 0).all())
    pos = vis & (ref["opacities"] > 0)   # (op_eff = 0 where rho = 0: held to exactly 0)
    assert bool((op[vis & ~pos] == 0).all())
    e_op = ((op - ref["opacities"]).abs()[pos] / ref["opacities"][pos]).max().item()
    print(f"  op_eff: max rel err {e_op:.3g}")
    assert e_op <= OPEFF_RTOL, e_op
    keep = torch.from_numpy(~rz)
    if depth_mode is not None:
        _check_depth_forward(depth_mode, out, ref, rz)
    else:
        e_c = (out["img"].cpu().double() - ref["img"]).abs().amax(-1)[keep].max().item()
        e_a = (out["alpha"].cpu().double() - ref["alpha"])[..., 0].abs()[keep].max().item()
        print(f"  max colour error {e_c:.3g}, max alpha error {e_a:.3g}")
        assert e_c <= FWD_ATOL and e_a <= FWD_ATOL, (e_c, e_a)
    for i, nm in enumerate(AR.GEO + tuple(f"colors[{j}]" for j in range(n_leaves))):
        assert torch.isfinite(ref["grads"][i]).all() and torch.isfinite(out["grads"][i]).all(), nm
        r = _rel(out["grads"][i], ref["grads"][i])
        print(f"  v_{nm}: rel err {r:.3g}")
        assert r <= GRAD_RTOL, (nm, r)
    r = _rel(out["absgrad"], ref["absgrad"])
    print(f"  absgrad: rel err {r:.3g}")
    assert r <= GRAD_RTOL, r
    if cam:
        got, want = out["v_viewmats"].cpu().double(), ref["v_viewmats"]
        for c in range(C):
            rc = ((got[c] - want[c]).abs().max() / want[c].abs().max()).item()
            print(f"  v_viewmats[{c}]: rel err {rc:.3g}")
            assert rc <= GRAD_RTOL, (c, rc)


def _parity(name, colors, sh_degree, bg, seed, mode="RGB", cam=False, culling="gsplat", **kw):
    sc, rz = _scene(name)
    D = (3 if sh_degree is not None else np.asarray(colors[0]).shape[-1]) + (0 if mode == "RGB" else 1)
    vc, va = AR.upstream(rz, D, seed)
    out = AR.gpu(sc, colors, sh_degree, bg, vc, va, mode=mode, cam=cam, culling=culling, **kw)
    ref = AR.reference(sc, colors, sh_degree, bg, vc, va, mode=mode, cam=cam)
    assert out["img"].shape == ref["img"].shape
    _check(name, out, ref, rz, len(colors), cam=cam, depth_mode=None if mode == "RGB" else mode)
    return out, ref


# ---- 1. parity ----

def test_sh3_with_backgrounds_over_the_whole_range_of_rho():
    sc, _ = _scene("A")
    _parity("A", [sc["shs"]], 3, sc["backgrounds"], seed=1)


def test_four_feature_channels_on_ragged_tiles_two_cameras_tight_culling():
    sc, _ = _scene("B")
    feats = np.random.default_rng(5).standard_normal((sc["means"].shape[0], 4)).astype(np.float32)
    out, _ = _parity("B", [feats], None, None, seed=2, culling="tight")
    assert out["meta"]["tile_width"] == 3 and out["meta"]["tile_height"] == 2   # (40 x 24: ragged on both axes)


def test_the_sh_pair_with_an_expected_depth_channel():
    sc, _ = _scene("B")
    shs = sc["shs"]
    _parity("B", [np.ascontiguousarray(shs[:, :1]), np.ascontiguousarray(shs[:, 1:])], 2, sc["backgrounds"], seed=3, mode="RGB+ED", culling="tight")


@pytest.mark.parametrize("name", ["A", "B"])
def test_view_matrix_gradients(name):
    """`_camera_grads=True`: SH colours (A, one camera: the direction term too) and three feature channels (B, two cameras)."""
    sc, _ = _scene(name)
    if name == "A":
        _parity("A", [sc["shs"]], 3, sc["backgrounds"], seed=4, cam=True)
    else:
        feats = np.random.default_rng(6).standard_normal((sc["means"].shape[0], 3)).astype(np.float32)
        _parity("B", [feats], None, None, seed=4, cam=True, culling="gsplat_eager")


def test_activations_inside_the_projection():
    sc, _ = _scene("A")
    op = np.clip(sc["opacities"], 1e-4, 1 - 1e-4).astype(np.float32)
    raw = dict(sc, scales=np.log(sc["scales"]).astype(np.float32), opacities=np.log(op / (1 - op)).astype(np.float32))
    act = dict(sc, scales=np.exp(raw["scales"].astype(np.float64)), opacities=1.0 / (1.0 + np.exp(-raw["opacities"].astype(np.float64))))
    rz = AR.razor(act)
    assert rz.mean() <= RAZOR_SHARE
    vc, va = AR.upstream(rz, 3, 7)
    out = AR.gpu(raw, [sc["shs"]], 3, sc["backgrounds"], vc, va, _activations="exp_sigmoid")
    ref = AR.reference(act, [sc["shs"]], 3, sc["backgrounds"], vc, va)
    s64, o64 = torch.from_numpy(act["scales"]), torch.from_numpy(act["opacities"])
    ref["grads"][2], ref["grads"][3] = ref["grads"][2] * s64, ref["grads"][3] * o64 * (1 - o64)
    _check("A", out, ref, rz, 1)


# ---- 2. what the mode leaves alone ----

@pytest.mark.parametrize("name", ["A", "B"])
def test_radii_means2d_conics_and_depths_are_the_classic_calls(name):
    sc, _ = _scene(name)
    deg = sc["sh_degree"]
    a = AR.gpu(sc, [sc["shs"]], deg, sc["backgrounds"], grad=False)
    b = AR.gpu(sc, [sc["shs"]], deg, sc["backgrounds"], grad=False, rasterize_mode="classic")
    for k in ("radii", "means2d", "conics", "depths"):
        assert torch.equal(a["meta"][k], b["meta"][k]), k
    assert int((a["meta"]["radii"] > 0).sum()) >= 200
    assert not torch.equal(a["img"], b["img"])   # (the mode does something)
    assert b["meta"]["opacities"].shape == a["meta"]["opacities"].shape and bool((a["meta"]["opacities"] < b["meta"]["opacities"]).all())


@pytest.mark.parametrize("cam", [False, True])
def test_classic_passed_explicitly_is_bitwise_the_call_without_the_keyword(cam):
    sc, _ = _scene("B")
    g = torch.Generator().manual_seed(8)
    vc, va = torch.randn((2, 24, 40, 3), generator=g), torch.randn((2, 24, 40, 1), generator=g)
    a = AR.gpu(sc, [sc["shs"]], 2, sc["backgrounds"], vc, va, cam=cam, rasterize_mode="classic")
    b = AR.gpu(sc, [sc["shs"]], 2, sc["backgrounds"], vc, va, cam=cam, rasterize_mode=None)
    assert torch.equal(a["img"], b["img"]) and torch.equal(a["alpha"], b["alpha"])
    for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss", "flatten_ids", "isect_offsets"):
        assert torch.equal(a["meta"][k], b["meta"][k]), k
    for x, y in zip(a["grads"] + [a["absgrad"]], b["grads"] + [b["absgrad"]]):
        assert torch.equal(x, y)
    if cam:
        assert torch.equal(a["v_viewmats"], b["v_viewmats"])


# ---- 3. the list arrays ----

def test_gsplat_list_arrays_are_the_references():
    """`_tile_culling="gsplat"`: the 3-sigma lists, which do not know the opacity -- the reference's, bit for bit."""
    sc, _ = _scene("B")
    out = AR.gpu(sc, [sc["shs"]], 2, sc["backgrounds"], grad=False, culling="gsplat")
    with torch.no_grad():
        ref = AR.forward(sc)
    for k in ("tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets"):
        assert torch.equal(out["meta"][k].cpu().to(ref[k].dtype), ref[k]), k
    assert int(ref["flatten_ids"].numel()) > 500


def _pairs(meta_or_ref, C, tiles):
    """The set of (camera * tiles + tile, Gaussian) pairs of a list."""
    off = meta_or_ref["isect_offsets"].reshape(-1).cpu().long()
    fid = meta_or_ref["flatten_ids"].cpu().long()
    counts = torch.diff(off, append=off.new_tensor([fid.numel()]))
    tile = torch.repeat_interleave(torch.arange(C * tiles), counts)
    return set(zip(tile.tolist(), fid.tolist()))


@pytest.mark.parametrize("name", ["A", "B"])
def test_tight_lists_take_op_eff(name):
    """The tight lists hold every (tile, Gaussian) in which the reference finds a pixel with op_eff exp(-sigma) >= 1/255, nothing outside
    the reference's 3-sigma lists, each tile's entries in the reference's depth order, and fewer entries than the classic call's tight
    lists (which the raw opacity makes).  One camera (A): they are bit for bit the tight lists of the CLASSIC call fed with op_eff as
    its opacities -- the list stages see the effective opacity and nothing else of the mode."""
    sc, _ = _scene(name)
    deg = sc["sh_degree"]
    W, H = int(sc["width"]), int(sc["height"])
    out = AR.gpu(sc, [sc["shs"]], deg, sc["backgrounds"], grad=False, culling="tight")
    classic = AR.gpu(sc, [sc["shs"]], deg, sc["backgrounds"], grad=False, culling="tight", rasterize_mode="classic")
    with torch.no_grad():
        ref = AR.forward(sc)
    C, N = ref["radii"].shape
    tw, th = -(-W // 16), -(-H // 16)
    got, full = _pairs(out["meta"], C, tw * th), _pairs(ref, C, tw * th)
    assert got <= full
    # the pairs the reference's blend can take: alpha at the pixel centres, per (camera, Gaussian)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    tile_of = ((ys - 0.5).long() // 16) * tw + (xs - 0.5).long() // 16
    need = set()
    for c in range(C):
        for n in torch.nonzero(ref["radii"][c] > 0).reshape(-1).tolist():
            dx, dy = xs - ref["means2d"][c, n, 0], ys - ref["means2d"][c, n, 1]
            A_, B_, C_ = ref["conics"][c, n]
            alpha = ref["opacities"][c, n] * torch.exp(-(0.5 * (A_ * dx * dx + C_ * dy * dy) + B_ * dx * dy))
            for t in torch.unique(tile_of[alpha >= 1.0 / 255.0]).tolist():
                need.add((c * tw * th + t, c * N + n))
    print(f"{name}: {len(need)} needed <= {len(got)} tight (op_eff) <= {out['meta']['flatten_ids'].numel()}; classic tight {classic['meta']['flatten_ids'].numel()}, 3-sigma {len(full)}")
    assert need <= got and len(need) > 100
    assert len(got) < classic["meta"]["flatten_ids"].numel()
    # depth order inside each tile: the reference's order restricted to the kept entries
    keep = torch.tensor([p in got for p in zip(torch.repeat_interleave(torch.arange(C * tw * th), torch.diff(
        ref["isect_offsets"].reshape(-1).long(), append=torch.tensor([ref["flatten_ids"].numel()]))).tolist(), ref["flatten_ids"].tolist())])
    assert torch.equal(out["meta"]["flatten_ids"].cpu().long(), ref["flatten_ids"].long()[keep])
    if C == 1:
        fed = AR.gpu(dict(sc, opacities=out["meta"]["opacities"][0].cpu().numpy()), [sc["shs"]], deg, sc["backgrounds"], grad=False, culling="tight",
                     rasterize_mode="classic")
        for k in ("tiles_per_gauss", "flatten_ids", "isect_offsets"):
            assert torch.equal(fed["meta"][k], out["meta"][k]), k
        assert torch.equal(fed["img"], out["img"]) and torch.equal(fed["alpha"], out["alpha"])


# ---- 4. degenerate covariances ----

def test_rank_deficient_gaussians_contribute_nothing_and_stay_finite():
    sc, rz = _scene("Z")
    out, ref = _parity("Z", [sc["shs"]], 1, sc["backgrounds"], seed=9, cam=True)
    d = AR.Z_DEGENERATE
    assert bool((ref["rho"][0, :d] == 0).all()) and bool((ref["radii"][0, :d] > 0).all())
    assert bool((out["meta"]["opacities"][0, :d] == 0).all())
    assert bool(torch.isfinite(out["img"]).all()) and bool(torch.isfinite(out["alpha"]).all())
    for g in out["grads"] + [out["v_viewmats"], out["absgrad"]]:
        assert bool(torch.isfinite(g).all())
    for g in out["grads"][:4]:   # (no pixel takes them: no gradient reaches them)
        assert not bool(g[:d].any())
    rest = {k: np.ascontiguousarray(np.asarray(sc[k])[d:]) for k in AR.GEO + ("shs",)}
    without = AR.gpu(dict(sc, **rest), [rest["shs"]], 1, sc["backgrounds"], grad=False)
    assert torch.equal(without["img"], out["img"]) and torch.equal(without["alpha"], out["alpha"])
    tight = AR.gpu(sc, [sc["shs"]], 1, sc["backgrounds"], grad=False, culling="tight")
    assert torch.equal(tight["img"], out["img"]) and not bool(tight["meta"]["tiles_per_gauss"][0, :d].any())


# ---- 5. the captured step ----

def _train_setup():
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
    from test_gpu_train_graph import LRS
    sc = AR.scene("A")
    dev, T, W, H = torch.device("cuda:0"), torch.from_numpy, 64, 48
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"])
    views = [AR._view(3.0, yaw, pitch) for yaw, pitch in ((0.25, -0.15), (-0.3, 0.1), (0.05, 0.3))]

    def make():
        m = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]),
                          sh_0=shs[:, :1].contiguous(), sh_rest=shs[:, 1:].contiguous(),
                          logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3, white_background=True,
                          means_lr_schedule_max_steps=40).to(dev)
        m.rasterize_mode = "antialiased"
        return m, build_optimizers(m, *LRS, fused="hip")

    datas = [{"w2c": T(v).to(dev), "K": T(sc["Ks"][0]).to(dev), "width": W, "height": H} for v in views]
    g = torch.Generator().manual_seed(11)
    gts = [torch.rand((H, W, 3), generator=g).to(dev) for _ in views]
    return dev, make, datas, gts


ORDER = (2, 0, 1, 1, 2, 0)   # six steps, the views shuffled


def test_captured_step_with_the_scale_regulariser_equals_the_eager_loop():
    """Parameters, moments and statistics bit for bit, l1 and 1 - ssim bit for bit, the total to 1e-6 (the eager mean of the
    regulariser sums in another order): the standard of tests/test_gpu_scale_reg.py."""
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    from test_gpu_scale_reg import _close, _eager_step, _state
    dev, make, datas, gts = _train_setup()
    (ma, oa), (mb, ob) = make(), make()
    for m in (ma, mb):
        m.USE_SCALE_REGULARIZATION, m.MAX_SCALE_RATIO = True, 1.2
    lca, lcb = (LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05) for m in (ma, mb))
    runner = TrainStepGraph(mb, ob, lcb, datas[0], gts[0], check_every=2, rasterize_mode="antialiased")
    for it, v in enumerate(ORDER):
        ma.update_learning_rate(it); mb.update_learning_rate(it)
        l_ref, reg_ref = _eager_step(ma, oa, lca, datas[v], gts[v])
        out = runner.step(datas[v], gts[v])
        runner.finish()
        assert torch.equal(out["loss3"][:2], l_ref[:2]), it
        assert _close(out["loss3"][2], l_ref[2]) and _close(out["scale_reg"], reg_ref) and float(reg_ref) > 0.0, it
        sa, sb = _state(ma, oa), _state(mb, ob)
        for k in sa:
            assert torch.equal(sb[k], sa[k]), (it, k, float((sb[k] - sa[k]).abs().max()))
    rep = runner.report()
    assert rep["steps"] == 6 and rep["overflows"] == 0 and rep["graph"] and rep["scale_reg"] and not rep["rounds"]
    assert int((ma.collecting_counts > 0).sum()) > 250


def test_captured_step_equals_the_eager_loop_and_is_not_the_classic_step():
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    from test_gpu_train_graph import _assert_same, _eager_step
    dev, make, datas, gts = _train_setup()
    (ma, oa), (mb, ob), (mc, oc) = make(), make(), make()
    mc.rasterize_mode = "classic"
    lc = LossComputer(0.2, clamp_input=True)
    runner = TrainStepGraph(mb, ob, lc, datas[0], gts[0], check_every=2)   # (the mode: the model's attribute)
    classic = TrainStepGraph(mc, oc, lc, datas[0], gts[0], check_every=2)
    assert runner.antialiased and not classic.antialiased
    for it, v in enumerate(ORDER):
        for m in (ma, mb, mc):
            m.update_learning_rate(it)
        l_ref = _eager_step(ma, oa, lc, datas[v], gts[v])
        out = runner.step(datas[v], gts[v])
        assert torch.equal(out["loss3"], l_ref), it
        runner.finish()
        _assert_same(ma, oa, mb, ob, f"step {it}")
    classic.step(datas[0], gts[0]); classic.finish()
    assert not torch.equal(mc.logit_opacities, mb.logit_opacities)


def test_captured_step_with_exposure_renders_and_loses_as_the_eager_loop():
    """With `exposure=`: per step the render, the exposed image and the loss are the eager autograd loop's bit for bit on the parameters
    the step saw (the standard of tests/test_gpu_exposure.py), and after six steps the captured runner's parameters, moments and table
    are those of the same sequence issued eagerly."""
    from easy_gaussian_splatting_amd.exposure import ExposureTable
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    from test_gpu_exposure import EXP_LR, _assert_same_exposure, _table
    from test_gpu_train_graph import _assert_same
    dev, make, datas, gts = _train_setup()
    (ma, oa), (mb, ob), (me, oe) = make(), make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    kw = dict(check_every=2, exposure_lr=EXP_LR, rasterize_mode="antialiased")
    ra = TrainStepGraph(ma, oa, lc, datas[0], gts[0], use_graph=True, exposure=_table(dev, seed=5), **kw)
    rb = TrainStepGraph(mb, ob, lc, datas[0], gts[0], use_graph=False, exposure=_table(dev, seed=5), **kw)
    eager = ExposureTable(3).to(dev)
    for it, v in enumerate(ORDER):
        for m in (ma, mb):
            m.update_learning_rate(it)
        with torch.no_grad():   # the eager loop's model and table as the step is about to see them
            for k in ma.param_names:
                getattr(me, k).copy_(getattr(ma, k))
            eager.affine.copy_(ra.exposure.affine)
        oa_, ob_ = ra.step(datas[v], gts[v], view_index=v), rb.step(datas[v], gts[v], view_index=v)
        ra.finish(); rb.finish()
        render = me(datas[v], clamp=False)["render_img"]
        exposed = eager(render, v)
        loss = lc.get_loss_dict(exposed, gts[v], None)
        loss["total"].backward()
        assert torch.equal(render.detach(), oa_["render_img"]) and torch.equal(exposed.detach(), oa_["exposed"]), it
        assert torch.equal(loss["total"].detach(), oa_["loss3"][2]), it
        assert torch.equal(eager.affine.grad[v].reshape(-1), oa_["v_affine"]), it
        eager.affine.grad = None
        for k in me.param_names:
            getattr(me, k).grad = None
        assert torch.equal(oa_["loss3"], ob_["loss3"]) and torch.equal(oa_["exposed"], ob_["exposed"]), it
    _assert_same(ma, oa, mb, ob, "captured vs eager form")
    _assert_same_exposure(ra, rb, "captured vs eager form")
    assert ra.report()["graph"] and not rb.report()["graph"] and ra.report()["overflows"] == 0
