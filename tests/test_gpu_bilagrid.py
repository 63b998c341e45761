"""Per-view bilateral grids on the device (csrc/gs_bilagrid.hip, `bilagrid.BilateralGrids`, `TrainStepGraph(bilagrid=...)`; DESIGN.md
"Bilateral grids in the captured step"): the kernels against torch's grid_sample in fp64 and the bounds of tests/bilagrid_ref.py --
frames under one block and ragged, one spatial cell over many blocks, many cells of few pixels --, each twice for equal bits; the
total variation, the dense Adam and the staging record; the module's autograd path against its plain-torch form; and on the scene of
tests/test_gpu_train_graph.py the captured step: off means off bit for bit, captured equals its eager form (autograd function +
tv_loss(fused=True) + the same Adam entry), the step guard covers the grids, the combinations, sixty steps bring the loss down as the
plain torch loop does, and HostFeed forwards the view."""
import functools

import numpy as np
import pytest
import torch

import adam_ref as A
import bilagrid_ref as R
import parity_log
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.bilagrid import BilagridAdamState, BilateralGrids
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.pose import CameraDeltas
from easy_gaussian_splatting_amd.train_graph import HostFeed, TrainStepGraph
from test_gpu_train_graph import _assert_same, _setup

pytestmark = pytest.mark.gpu
BG_LR, BG_BETAS, BG_EPS, BG_TV = 2e-3, (0.9, 0.999), 1e-15, 10.0
N_VIEWS = 3
# (H, W, (Wg, Hg, L)): under one block; ragged with an interior luminance node; ragged with the default depth; ONE spatial cell over
# five blocks (the cross-block order); many cells of few pixels.  Wg != Hg wherever the case is not fixed: a transposed index shows.
CASES = [(11, 13, (5, 3, 2)), (37, 53, (7, 4, 3)), (37, 53, (16, 12, 8)), (72, 130, (2, 2, 2)), (72, 130, (16, 16, 8))]


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- kernel level -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(H, W, shape):
    """Inputs, fp64 references and bounds of one frame, computed once and shared (read-only) by the tests that use the frame."""
    Wg, Hg, L = shape
    rng = np.random.default_rng(1000 * H + W + 7 * Wg)
    grids = R.random_grids(rng, N_VIEWS, Wg, Hg, L)
    img, v = R.random_images(rng, H, W, L)
    view = (H + W + Wg) % N_VIEWS
    assert R.kink_distance(img, L).min() >= R.KINK_MARGIN   # (on the fp64 luminance: no pixel sits on a kink of the guide)
    luma = img.astype(np.float64) @ R.LUMA
    assert (luma < 0).mean() >= 0.05 and (luma > 1).mean() >= 0.05
    ref, b = R.slice64(grids, img, v, view), R.bounds64(grids[view], img, v)
    bounds = {"apply": b["out"], "vjp": b["v_c"], "adjoint": R.slab_bound(b, ref["v_grids"][view])}
    refs = {"apply": ref["out"], "vjp": ref["v_c"], "adjoint": ref["v_grids"][view]}
    for x in (grids, img, v):
        x.setflags(write=False)
    return grids, img, v, view, refs, bounds


def _kernels(H, W, shape, grids, img, v, view, by_record):
    """gs_bilagrid_apply and gs_bilagrid_bwd on one frame; the view through a staged record or by value.  numpy (out, v_c, v_slab)."""
    dev, L = torch.device("cuda:0"), nat.lib()
    Wg, Hg, Lz = shape
    st = _st(dev)
    t, x, g = (torch.from_numpy(np.array(a)).to(dev) for a in (grids, img, v))
    out = torch.full_like(x, float("nan"))
    slab = torch.full((12, Lz, Hg, Wg), float("nan"), dtype=torch.float32, device=dev)
    partials = torch.full((int(L.gs_bilagrid_partials_doubles(H, W, Wg, Hg, Lz)),), float("nan"), dtype=torch.float64, device=dev)
    rec, by_value = None, view
    if by_record:
        rec_t = torch.zeros((nat.GS_BILAGRID_REC_FLOATS,), dtype=torch.float32, device=dev)
        nat.check(L.gs_bilagrid_step_inputs(st, view, N_VIEWS, BG_LR, BG_BETAS[0], BG_BETAS[1], 3, rec_t.data_ptr()), "gs_bilagrid_step_inputs")
        rec, by_value = rec_t.data_ptr(), -7   # (with a record the by-value argument is not looked at)
    nat.check(L.gs_bilagrid_apply(st, H, W, N_VIEWS, Wg, Hg, Lz, rec, by_value, t.data_ptr(), x.data_ptr(), out.data_ptr()), "gs_bilagrid_apply")
    nat.check(L.gs_bilagrid_bwd(st, H, W, N_VIEWS, Wg, Hg, Lz, rec, by_value, t.data_ptr(), x.data_ptr(), g.data_ptr(), partials.data_ptr(),
                                slab.data_ptr()), "gs_bilagrid_bwd")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), g.cpu().numpy(), slab.cpu().numpy()


@pytest.mark.parametrize("H,W,shape", CASES, ids=lambda x: str(x))
def test_kernels_keep_their_bounds_and_their_bits(H, W, shape):
    grids, img, v, view, refs, bounds = _case(H, W, shape)
    got = dict(zip(("apply", "vjp", "adjoint"), _kernels(H, W, shape, grids, img, v, view, by_record=True)))
    ratios = {k: R.worst_ratio(got[k], refs[k], bounds[k]) for k in got}
    print(f"{H}x{W} grid {shape} view {view}: worst |error| / bound {ratios}")
    parity_log.record(**{f"bilagrid_{H}x{W}_{'x'.join(map(str, shape))}": ratios})
    assert all(r < 1.0 for r in ratios.values()), ratios
    again = _kernels(H, W, shape, grids, img, v, view, by_record=True)       # two runs: the same bits, no atomics anywhere
    by_value = _kernels(H, W, shape, grids, img, v, view, by_record=False)   # the view by value: the same result
    for k, a, b in zip(got, again, by_value):
        assert np.array_equal(got[k].view(np.uint32), a.view(np.uint32)), ("second run", k)
        assert np.array_equal(got[k].view(np.uint32), b.view(np.uint32)), ("by value", k)


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("shape", [(16, 16, 8), (5, 3, 2)], ids=lambda x: str(x))
def test_total_variation_value_and_gradient(n_views, shape):
    dev, L = torch.device("cuda:0"), nat.lib()
    Wg, Hg, Lz = shape
    st = _st(dev)
    rng = np.random.default_rng(50 + n_views + Wg)
    grids_np = R.random_grids(rng, n_views, Wg, Hg, Lz)
    slab_np = (1e-3 * rng.standard_normal((12, Lz, Hg, Wg))).astype(np.float32)
    ref, ref_b, grad, grad_b = R.tv64(grids_np, BG_TV)
    grids, slab = torch.from_numpy(grids_np).to(dev), torch.from_numpy(slab_np).to(dev)
    ws = torch.empty((nat.GS_BILAGRID_TV_DOUBLES,), dtype=torch.float64, device=dev)
    view = n_views - 1
    runs = []
    for with_slab in (False, True, True):
        loss3 = torch.tensor([0.25, 0.5, 0.125], dtype=torch.float32, device=dev)
        tv = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        v_grids = torch.full_like(grids, float("nan"))
        nat.check(L.gs_bilagrid_tv(st, n_views, Wg, Hg, Lz, grids.data_ptr(), BG_TV, None, view, slab.data_ptr() if with_slab else None,
                                   loss3.data_ptr(), tv.data_ptr(), v_grids.data_ptr(), ws.data_ptr()), "gs_bilagrid_tv")
        runs.append((tv.cpu().numpy(), v_grids.cpu().numpy(), loss3.cpu().numpy()))
    (tv0, g0, l0), (tv1, g1, l1), (tv2, g2, l2) = runs
    ratios = {"tv": R.worst_ratio(tv0[0], ref, ref_b), "grad": R.worst_ratio(g0, grad, grad_b)}
    print(f"grid {shape} x {n_views}: tv {ref:.6g}, worst |error| / bound {ratios}")
    parity_log.record(**{f"bilagrid_tv_{'x'.join(map(str, shape))}_n{n_views}": ratios})
    assert all(r < 1.0 for r in ratios.values()), ratios
    assert l0[0] == 0.25 and l0[1] == 0.5 and l0[2] == np.float32(0.125) + np.float32(BG_TV) * tv0[0]   # the product rounded on its own
    want = g0.copy()
    want[view] = g0[view] + slab_np   # the slab added to the rounded TV gradient, on the view alone
    assert np.array_equal(g1.view(np.uint32), want.view(np.uint32)) and tv1[0] == tv0[0]
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)) and tv2[0] == tv1[0] and l2[2] == l1[2]   # twice: equal bits


def test_adam_entry_is_dense_adam_on_all_elements():
    dev, L = torch.device("cuda:0"), nat.lib()
    st = _st(dev)
    n = 12 * 683   # (not a multiple of a block, nor of a wave)
    p, g, m, v = A.regime_inputs(n, seed=21)
    t, lr = 5, 3e-3
    P, G, Mo, V = (torch.from_numpy(x).to(dev) for x in (p, g, m, v))
    rec = torch.zeros((nat.GS_BILAGRID_REC_FLOATS,), dtype=torch.float32, device=dev)
    nat.check(L.gs_bilagrid_step_inputs(st, 0, 1, lr, BG_BETAS[0], BG_BETAS[1], t, rec.data_ptr()), "gs_bilagrid_step_inputs")
    nat.check(L.gs_bilagrid_adam(st, n, rec.data_ptr(), P.data_ptr(), Mo.data_ptr(), V.data_ptr(), G.data_ptr(), BG_BETAS[0], BG_BETAS[1], BG_EPS),
              "gs_bilagrid_adam")
    ratios = A.error_ratios((P.cpu().numpy(), Mo.cpu().numpy(), V.cpu().numpy()), p, A.adam_ref(p, g, m, v, lr, t, BG_BETAS[0], BG_BETAS[1], BG_EPS))
    print(f"gs_bilagrid_adam: error / bound {ratios}")
    assert ratios["p"] <= 1.0 and ratios["m"] <= 1.0 and ratios["v"] <= 1.0, ratios
    assert torch.equal(G.cpu(), torch.from_numpy(g))   # (the gradient is read, never written)


def test_record_holds_the_bias_corrections_and_the_view():
    dev, L = torch.device("cuda:0"), nat.lib()
    rec = torch.full((nat.GS_BILAGRID_REC_FLOATS,), -1.0, dtype=torch.float32, device=dev)
    for view, step, lr in ((0, 1, 2e-3), (2, 9, 3e-4)):
        nat.check(L.gs_bilagrid_step_inputs(_st(dev), view, N_VIEWS, lr, BG_BETAS[0], BG_BETAS[1], step, rec.data_ptr()), "gs_bilagrid_step_inputs")
        r = rec.cpu().numpy()
        bc1, bc2 = 1.0 - float(np.float32(0.9)) ** step, 1.0 - float(np.float32(0.999)) ** step
        assert r[0] == np.float32(float(np.float32(lr)) / bc1) and r[1] == np.float32(1.0 / np.sqrt(bc2))
        assert int(r[2:3].view(np.int32)[0]) == view and r[3] == 0.0


@pytest.mark.parametrize("H,W,shape", [CASES[1], CASES[4]], ids=lambda x: str(x))
def test_module_on_the_device_is_the_plain_torch_module_in_fp64(H, W, shape):
    dev = torch.device("cuda:0")
    grids_np, img_np, v_np, view, refs, bounds = _case(H, W, shape)
    cpu, gpu = BilateralGrids(N_VIEWS, *shape).double(), BilateralGrids(N_VIEWS, *shape).to(dev)
    with torch.no_grad():
        cpu.grids.copy_(torch.from_numpy(np.array(grids_np)))
        gpu.grids.copy_(torch.from_numpy(np.array(grids_np)))
    xc = torch.from_numpy(np.array(img_np)).double().requires_grad_(True)
    xg = torch.from_numpy(np.array(img_np)).to(dev).requires_grad_(True)
    oc, og = cpu(xc, view), gpu(xg, view)
    (oc * torch.from_numpy(np.array(v_np)).double()).sum().backward()
    (og * torch.from_numpy(np.array(v_np)).to(dev)).sum().backward()
    assert og.dtype == torch.float32 and gpu.grids.grad.shape == gpu.grids.shape
    ratios = {"apply": R.worst_ratio(og.detach().cpu().numpy(), oc.detach().numpy(), bounds["apply"]),
              "vjp": R.worst_ratio(xg.grad.cpu().numpy(), xc.grad.numpy(), bounds["vjp"]),
              "adjoint": R.worst_ratio(gpu.grids.grad[view].cpu().numpy(), cpu.grids.grad[view].numpy(), bounds["adjoint"])}
    print(f"{H}x{W} grid {shape}: BilateralGrids on the device against the CPU path in fp64, worst |error| / bound {ratios}")
    assert all(r < 1.0 for r in ratios.values()), ratios
    others = [r for r in range(N_VIEWS) if r != view]
    assert not gpu.grids.grad[others].any() and not cpu.grids.grad[others].any()   # dense, exact zeros on every other view
    tv_ref, tv_b, _, _ = R.tv64(grids_np)
    assert abs(float(gpu.tv_loss(fused=True).detach()) - tv_ref) < tv_b and abs(float(gpu.tv_loss().detach()) - tv_ref) < 1e-5 * tv_ref


# ---- runner level ---------------------------------------------------------------------------------------------------------------
def _grids(dev, seed=None, shape=(6, 4, 3), n_views=N_VIEWS):
    """Identity grids, or (seed) every node off the identity by up to 0.05 (gains up to 0.1): nothing is smooth, nothing commutes."""
    g = BilateralGrids(n_views, *shape).to(dev)
    if seed is not None:
        gen = torch.Generator().manual_seed(seed)
        d = 0.05 * (2 * torch.rand(tuple(g.grids.shape), generator=gen) - 1)
        d[:, [0, 5, 10]] *= 2.0
        with torch.no_grad():
            g.grids.add_(d.to(dev))
    return g


def _bg_state(runner):
    s = runner.bilagrid_state
    return runner.bilagrid.grids.detach().clone(), s.exp_avg.clone(), s.exp_avg_sq.clone()


def _assert_same_grids(ra, rb, what=""):
    for x, y, name in zip(_bg_state(ra), _bg_state(rb), ("grids", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), (what, name)
    assert ra.bilagrid_state.step == rb.bilagrid_state.step


# 1. off means off
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_identity_grids_at_zero_rate_and_zero_tv_weight_change_nothing(fuse_adam):
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    grids = _grids(dev, shape=(16, 16, 8))
    identity = grids.grids.detach().clone()
    ra = TrainStepGraph(ma, oa, lc, datas[0], gts[0], check_every=2, fuse_adam=fuse_adam)
    rb = TrainStepGraph(mb, ob, lc, datas[0], gts[0], check_every=2, fuse_adam=fuse_adam, bilagrid=grids, bilagrid_lr=0.0, bilagrid_tv=0.0)
    assert "bilagrid" not in ra.report() and rb.report()["bilagrid"] is True   # (absent, not False: as "poses", "mcmc", "exposure")
    assert not any("bilagrid" in k or k in ("v_grids", "v_slab", "exposed") for k in ra.buf) and not hasattr(ra, "bilagrid_state")
    for it in range(5):
        v = it % 3
        ma.update_learning_rate(it); mb.update_learning_rate(it)
        la = ra.step(datas[v], gts[v])
        out = rb.step(datas[v], gts[v], view_index=v)
        ra.finish(); rb.finish()
        assert torch.equal(la["loss3"], out["loss3"]), it
        assert torch.equal(out["exposed"], la["render_img"]) and torch.equal(out["render_img"], la["render_img"]), it
        assert float(out["bilagrid_tv"]) == 0.0
        _assert_same(ma, oa, mb, ob, f"step {it}")
    assert torch.equal(grids.grids.detach(), identity) and bool(rb.bilagrid_state.exp_avg.any())
    assert rb.bilagrid_state.step == 5 and rb.report()["bilagrid_steps"] == 5


# 2. captured == its eager form: the autograd function + tv_loss(fused=True) + the same Adam entry
@pytest.mark.parametrize("with_mask", [False, True])
def test_captured_step_equals_its_eager_form_bit_for_bit(with_mask):
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    lc, L = LossComputer(0.2, clamp_input=True), nat.lib()
    mask = None
    if with_mask:
        mask = torch.zeros((208, 320), device=dev)
        mask[40:150, 60:260] = 1.0
    captured, eager = _grids(dev, seed=7, shape=(16, 16, 8)), _grids(dev, seed=7, shape=(16, 16, 8))
    state = BilagridAdamState(eager)
    rec = torch.zeros((nat.GS_BILAGRID_REC_FLOATS,), dtype=torch.float32, device=dev)
    runner = TrainStepGraph(mb, ob, lc, datas[0], gts[0], mask, bilagrid=captured, bilagrid_lr=BG_LR, bilagrid_betas=BG_BETAS, bilagrid_eps=BG_EPS,
                            bilagrid_tv=BG_TV)
    assert runner.report()["graph"]
    for t, v in enumerate((1, 2, 0), start=1):
        params = {k: getattr(mb, k).detach().clone() for k in mb.param_names}   # (the model as the step is about to see it)
        out = runner.step(datas[v], gts[v], mask, view_index=v)
        runner.finish()
        with torch.no_grad():
            for k, p in params.items():
                getattr(ma, k).copy_(p)
        render = ma(datas[v], clamp=False)["render_img"]
        exposed = eager(render, v)
        tv = eager.tv_loss(fused=True)
        total = lc.get_loss_dict(exposed, gts[v], mask)["total"] + BG_TV * tv
        total.backward()
        assert torch.equal(render.detach(), out["render_img"]), v
        assert torch.equal(exposed.detach(), out["exposed"]) and not torch.equal(out["exposed"], out["render_img"]), v
        assert torch.equal(tv.detach(), out["bilagrid_tv"][0]) and float(tv.detach()) > 0, v
        assert torch.equal(total.detach(), out["loss3"][2]), v
        g = eager.grids.grad
        assert torch.equal(g, out["v_grids"]) and bool(g.all()), v   # dense: the TV gradient reaches every node of every view
        st = _st(dev)
        nat.check(L.gs_bilagrid_step_inputs(st, v, N_VIEWS, BG_LR, BG_BETAS[0], BG_BETAS[1], t, rec.data_ptr()), "gs_bilagrid_step_inputs")
        nat.check(L.gs_bilagrid_adam(st, g.numel(), rec.data_ptr(), eager.grids.data.data_ptr(), state.exp_avg.data_ptr(),
                                     state.exp_avg_sq.data_ptr(), g.data_ptr(), BG_BETAS[0], BG_BETAS[1], BG_EPS), "gs_bilagrid_adam")
        torch.cuda.synchronize(dev)
        assert torch.equal(eager.grids.detach(), captured.grids.detach()), v
        assert torch.equal(state.exp_avg, runner.bilagrid_state.exp_avg) and torch.equal(state.exp_avg_sq, runner.bilagrid_state.exp_avg_sq), v
        eager.grids.grad = None
        for k in ma.param_names:
            getattr(ma, k).grad = None


# 3. the update through the runner is dense Adam: idle views decay their moments and move under TV
def test_the_update_is_dense_adam_on_all_views():
    dev, make, datas, gts = _setup()
    m, o = make()
    lc = LossComputer(0.2, clamp_input=True)
    runner = TrainStepGraph(m, o, lc, datas[0], gts[0], bilagrid=_grids(dev, seed=9), bilagrid_lr=BG_LR, bilagrid_betas=BG_BETAS, bilagrid_eps=BG_EPS)
    for t, v in enumerate((1, 2, 0, 0), start=1):
        p0, m0, v0 = (x.cpu().numpy().reshape(N_VIEWS, -1) for x in _bg_state(runner))
        out = runner.step(datas[v], gts[v], view_index=v)
        runner.finish()
        g = out["v_grids"].cpu().numpy().reshape(N_VIEWS, -1)
        p1, m1, v1 = (x.cpu().numpy().reshape(N_VIEWS, -1) for x in _bg_state(runner))
        ratios = A.error_ratios((p1, m1, v1), p0, A.adam_ref(p0, g, m0, v0, BG_LR, t, BG_BETAS[0], BG_BETAS[1], BG_EPS))
        print(f"bilagrid step {t} on view {v}: error / bound  p {ratios['p']:.3f}  m {ratios['m']:.3f}  v {ratios['v']:.3f}")
        assert ratios["p"] <= 1.0 and ratios["m"] <= 1.0 and ratios["v"] <= 1.0, ratios
        assert (p1 != p0).mean() > 0.99   # every view moves: the idle ones under the total variation
    assert runner.bilagrid_state.step == 4 and runner.report()["bilagrid_steps"] == 4


# 4. the guard covers the grids
def test_overflow_voids_the_grid_update_and_the_replay_applies_it_once():
    dev, make, datas, gts = _setup(n=30000, n_views=3, dist=4.0)
    far = dict(datas[0])
    w2c = far["w2c"].clone()
    w2c[2, 3] += 14.0   # camera pulled back: splats shrink, few intersections
    far["w2c"] = w2c
    seq = [(far, 0), (datas[1], 1), (datas[2], 2), (far, 0), (datas[0], 0), (datas[1], 1)]
    lc = LossComputer(0.2, clamp_input=True)
    done = []
    for (first, view), margin in (((far, 0), 1.02), ((datas[1], 1), 4.0)):
        m, o = make()
        r = TrainStepGraph(m, o, lc, {**first, "view_index": view}, gts[0], margin=margin, check_every=4, bilagrid=_grids(dev, seed=5),
                           bilagrid_lr=BG_LR)
        for it, (d, v) in enumerate(seq):   # no finish() in between: the host keeps enqueueing behind the overflow
            r.bilagrid_lr = BG_LR * 0.8 ** it   # a schedule: every pending step keeps the rate it was issued with
            r.step(d, gts[it % 3], view_index=v)
        r.finish()
        done.append((m, o, r))
    (mt, ot, rt), (ma, oa, ra) = done
    print(f"[bilagrid step] margin 1.02 overflowed {rt.report()['overflows']} x and replayed {rt.report()['replayed_steps']} steps; "
          f"margin 4 overflowed {ra.report()['overflows']} x")
    assert rt.report()["overflows"] >= 1 and rt.report()["replayed_steps"] >= 1 and rt.report()["steps"] == len(seq)
    assert ra.report()["overflows"] == 0 and ra.report()["steps"] == len(seq)
    _assert_same(mt, ot, ma, oa, "replayed != never overflowed")
    _assert_same_grids(rt, ra, "replayed != never overflowed")


# 5. combinations
@pytest.mark.parametrize("combo", ["poses", "mcmc", "scale_reg", "rounds", "unfused"])
def test_combinations_captured_equals_eager_form(combo):
    dev, make, datas, gts = _setup()
    runs = []
    for use_graph in (True, False):
        m, o = make()
        kw, lc = {}, LossComputer(0.2, clamp_input=True)
        if combo == "poses":
            kw = dict(poses=CameraDeltas(N_VIEWS).to(dev), pose_lr=1e-3)
        elif combo == "mcmc":
            kw = dict(mcmc=M.MCMCStrategy(m, cap_max=m.nbr_gaussians, noise_lr=5e4, refine_start=10 ** 9, refine_stop=10 ** 9, refine_every=1,
                                          generator=torch.Generator(device=dev).manual_seed(5), noise="counter", seed=2 ** 63 + 12345),
                      mcmc_reg=(0.01, 0.01))
        elif combo == "scale_reg":
            m.USE_SCALE_REGULARIZATION, m.MAX_SCALE_RATIO = True, 2.0
            lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05)
        elif combo == "rounds":
            kw = dict(rounds="on")
        else:
            kw = dict(fuse_adam=False)
        r = TrainStepGraph(m, o, lc, datas[0], gts[0], use_graph=use_graph, check_every=2, bilagrid=_grids(dev, seed=5), bilagrid_lr=BG_LR, **kw)
        rep = r.report()
        assert rep["bilagrid"] and rep["graph"] == use_graph and rep.get("poses", False) == (combo == "poses")
        assert rep.get("mcmc", False) == (combo == "mcmc") and rep.get("scale_reg", False) == (combo == "scale_reg")
        assert rep["rounds"] == (combo == "rounds")
        grads = []
        for it in range(4):
            m.update_learning_rate(it)
            out = r.step(datas[it % 3], gts[it % 3], view_index=it % 3)
            r.finish()
            grads.append(torch.cat([out["v_grids"].reshape(-1), out["loss3"]] + ([out["v_delta"]] if combo == "poses" else [])).clone())
        runs.append((m, o, r, grads))
    (ma, oa, ra, sa), (mb, ob, rb, sb) = runs
    _assert_same(ma, oa, mb, ob, combo)
    _assert_same_grids(ra, rb, combo)
    if combo == "poses":
        assert torch.equal(ra.poses.deltas, rb.poses.deltas) and bool(ra.poses.deltas.detach().any())
    for x, y in zip(sa, sb):
        assert torch.equal(x, y) and bool(x.any())


# 6. it brings the loss down
def _smooth_truth(n_views, shape):
    """Known smooth per-view grids [n_views, 12, L, Hg, Wg] (fp64): a gain that falls off towards the corners (vignetting), a tone
    curve along the luminance axis and a colour cast per view, within +-0.15 of the identity."""
    Wg, Hg, L = shape
    x, y, z = torch.linspace(-1, 1, Wg, dtype=torch.float64), torch.linspace(-1, 1, Hg, dtype=torch.float64), torch.linspace(0, 1, L, dtype=torch.float64)
    r2 = (y[:, None] ** 2 + x[None, :] ** 2)[None]                  # [1, Hg, Wg]
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12).double()
    g = eye[None, :, None, None, None].repeat(n_views, 1, L, Hg, Wg)
    for v in range(n_views):
        gain = 1.0 + 0.08 * (v - 1) - 0.05 * r2 + 0.06 * (z[:, None, None] - 0.5)
        for i, cast in enumerate((1.0, 1.0 - 0.04 * v, 1.0 + 0.04 * v)):
            g[v, 5 * i] = gain * cast
            g[v, 4 * i + 3] = 0.03 * (v - 1) * (1.0 - z[:, None, None]) + 0.0 * r2
    return g


def test_sixty_captured_steps_bring_the_loss_down_as_the_plain_torch_loop_does():
    """Targets: the scene's own renders passed through known smooth per-view grids (`_smooth_truth`).  The scene is frozen; only the
    grids learn, from the identity, 20 steps per view.  The reference is the plain-torch module under `torch.optim.Adam` with the
    plain-torch loss on the CPU, run twice: in fp64 and in fp32.  Comparison quantity: the total loss (image loss + 10 tv) of each
    view's LAST step.  Margin: ten times the larger of (a) the difference between the two plain-torch runs -- the loop's own
    sensitivity to rounding -- and (b) 1e-6, the agreement of the fused loss kernel with the plain-torch loss on such frames
    (tests/test_gpu_loss.py, profiles/loss_parity.json), since the captured step's loss comes from that kernel.
    Measured on an MI355X: the loss per view 0.0631 / 0.0186 / 0.0350 at the first steps; the plain-torch loop ends at 0.008246 /
    0.002817 / 0.004695 in fp64 and within 7.5e-6 of that in fp32 (so the margin is 7.5e-5); the captured step ends -3.9e-7 / -8.5e-6
    / +5.7e-6 from the fp64 loop (DESIGN.md "Bilateral grids in the captured step")."""
    dev, make, datas, gts = _setup()
    m, o = make()
    for grp in o.param_groups:   # the scene is frozen
        grp["lr"] = 0.0
    shape = (6, 4, 3)
    lc = LossComputer(0.2, clamp_input=True)
    truth = _smooth_truth(N_VIEWS, shape)
    with torch.no_grad():
        renders = [m(d, clamp=False)["render_img"].detach().clone() for d in datas]
        targets = [R.slice_torch(truth, r.cpu().double(), v).clamp(0.0, 1.0).float().contiguous().to(dev) for v, r in enumerate(renders)]

    finals = {}
    lc_ref = LossComputer(0.2, fused=False, clamp_input=True)
    for dtype in (torch.float64, torch.float32):
        ref = BilateralGrids(N_VIEWS, *shape).to(dtype)
        opt = torch.optim.Adam(ref.parameters(), lr=BG_LR, betas=BG_BETAS, eps=BG_EPS)
        rr, tt = [r.cpu().to(dtype) for r in renders], [t.cpu().to(dtype) for t in targets]
        hist = []
        for it in range(60):
            v = it % 3
            opt.zero_grad()
            total = lc_ref.get_loss_dict(ref(rr[v], v), tt[v], None)["total"] + BG_TV * ref.tv_loss()
            total.backward()
            opt.step()
            hist.append(float(total.detach()))
        finals[dtype] = np.array(hist)
    h64, h32 = finals[torch.float64], finals[torch.float32]

    grids = _grids(dev, shape=shape)
    before = {k: getattr(m, k).detach().clone() for k in m.param_names}
    runner = TrainStepGraph(m, o, lc, datas[0], targets[0], bilagrid=grids, bilagrid_lr=BG_LR, bilagrid_betas=BG_BETAS, bilagrid_eps=BG_EPS,
                            bilagrid_tv=BG_TV)
    for it in range(60):
        runner.step(datas[it % 3], targets[it % 3], view_index=it % 3)
    runner.finish()
    hist = runner.loss_history(60)[:, 2].cpu().numpy().astype(np.float64)
    spread = float(np.abs(h64[-3:] - h32[-3:]).max())
    margin = 10.0 * max(spread, 1e-6)
    dev_ = hist[-3:] - h64[-3:]
    print(f"[bilagrid step] total loss per view: first {h64[:3].tolist()} -> plain torch fp64 {h64[-3:].tolist()}, fp32 {h32[-3:].tolist()} "
          f"(spread {spread:.3e}), captured {hist[-3:].tolist()}; captured - fp64 {dev_.tolist()}; margin {margin:.3e}")
    parity_log.record(bilagrid_sixty_steps={"first": h64[:3].tolist(), "torch_fp64": h64[-3:].tolist(), "torch_fp32": h32[-3:].tolist(),
                                            "captured": hist[-3:].tolist(), "margin": margin})
    assert all(torch.equal(getattr(m, k).detach(), before[k]) for k in m.param_names)
    assert (h64[-3:] < h64[:3]).all(), h64                    # the reference loop itself brings every view's loss down
    assert (hist[-3:] < hist[:3]).all(), hist                 # and so does the captured step
    assert (np.abs(dev_) <= margin).all(), (dev_, margin)     # ... to where the reference loop brings it
    assert runner.report()["steps"] == 60 and runner.report()["graph"] and runner.report()["overflows"] == 0


# 7. HostFeed
def test_host_feed_forwards_the_view_index_with_grids():
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    ra = TrainStepGraph(ma, oa, lc, datas[0], gts[0], bilagrid=_grids(dev, seed=5), bilagrid_lr=BG_LR)
    rb = TrainStepGraph(mb, ob, lc, datas[0], gts[0], bilagrid=_grids(dev, seed=5), bilagrid_lr=BG_LR)
    feed = HostFeed(rb)
    pin = lambda t: t.cpu().pin_memory()   # noqa: E731
    batches = [{"w2c": pin(datas[v]["w2c"]), "K": pin(datas[v]["K"]), "width": 320, "height": 208, "image": pin(gts[v]), "view_index": v}
               for v in range(3)]
    for it in range(4):
        v = (2 * it + 1) % 3
        ra.step(datas[v], gts[v], view_index=v)
        out = feed.step(batches[v])
        assert "v_grids" in out
    ra.finish(); rb.finish()
    _assert_same(ma, oa, mb, ob, "host feed")
    _assert_same_grids(ra, rb, "host feed")
    errors = []
    for call in (lambda: feed.step({k: x for k, x in batches[0].items() if k != "view_index"}), lambda: rb.step(datas[0], gts[0])):
        with pytest.raises(ValueError, match="view_index") as e:
            call()
        errors.append(str(e.value))
    assert errors[0] == errors[1]   # the feed without the index in its batch: the same refusal as step()
    assert rb.bilagrid_state.step == 4 and rb.report()["steps"] == 4
