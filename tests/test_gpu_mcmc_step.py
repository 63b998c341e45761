"""Training under a Gaussian budget inside the captured step, on the GPU:

* the counter-based normals (gs_mcmc_normals) against the Python-integer / numpy-fp64 reference of tests/mcmc_step_ref.py;
* the fused draw-and-apply pass (gs_mcmc_step_inputs + gs_mcmc_noise_step) against gs_mcmc_normals + the existing gs_mcmc_noise;
* the budget regulariser (gs_mcmc_reg) against the fp64 reference, and its fused form against the unfused chain;
* `TrainStepGraph(mcmc=...)` against the eager budget loop across a relocate + grow, and across an overflow replay.
"""
import numpy as np
import pytest
import torch

import mcmc_step_ref as R
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from scenes import make_scene

pytestmark = pytest.mark.gpu
LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4100]   # a thread's group of four, its ragged tail, a block of 1024 Gaussians and its edges
STEPS = [1, 2 ** 32 - 1, 2 ** 32 + 5]
SEEDS = [0, 2 ** 63 + 12345]


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream(dev()).cuda_stream


def host(t):
    return t.detach().cpu().numpy()


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp_distance(a, b):
    """float32 arrays: how many representable values apart (finite inputs)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- the normals ----

_REF = {}


def ref_normals(t, seed):
    """The reference's normals of Gaussians 0 .. max(SIZES), computed once per (step, seed) and shared."""
    if (t, seed) not in _REF:
        z = R.normals(max(SIZES) + 1, t, seed)
        z.setflags(write=False)
        _REF[(t, seed)] = z
    return _REF[(t, seed)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("t", STEPS)
def test_normals_against_the_reference(t, seed):
    ref = ref_normals(t, seed)
    worst = differing = total = 0
    for n in SIZES:
        z = M.counter_normals(n, t, seed, dev())
        assert z.shape == (n, 3) and z.dtype == torch.float32
        again = M.counter_normals(n, t, seed, dev())
        assert torch.equal(z, again)                                   # two calls: the same bits
        d = ulp_distance(host(z), ref[:n])
        worst, differing, total = max(worst, int(d.max())), differing + int((d != 0).sum()), total + d.size
        assert d.max() <= 1, (n, int(d.max()))
    print(f"[mcmc step] normals t={t} seed={seed}: {differing} of {total} values differ from the reference, by at most {worst} ulp")


def test_normals_depend_on_step_gaussian_and_seed():
    n, t, seed = 4100, 2 ** 32 + 5, 2 ** 63 + 12345
    z = host(M.counter_normals(n, t, seed, dev()))
    for other in (host(M.counter_normals(n, t + 1, seed, dev())), host(M.counter_normals(n, 5, seed, dev())),
                  host(M.counter_normals(n, t, 12345, dev())), host(M.counter_normals(n, t, seed + 1, dev()))):
        assert (bits_of(other) != bits_of(z)).mean() > 0.99
    assert (bits_of(z[1:]) != bits_of(z[:-1])).mean() > 0.99          # n offset by one: other values
    assert np.isfinite(z).all() and abs(z.mean()) < 0.05 and abs(z.var() - 1.0) < 0.05
    assert M.counter_normals(0, 1, 0, dev()).shape == (0, 3)


# ---- the noise ----

def noise_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn((n, 3), generator=g)
    ls = torch.rand((n, 3), generator=g) * 3.0 - 4.0
    q = torch.randn((n, 4), generator=g)
    lo = torch.rand((n,), generator=g) * 8.0 - 12.0          # transparent: the gate is open
    lo[::3] = 8.0                                            # opaque: the gate is shut
    return [x.to(dev()).contiguous() for x in (means, ls, q, lo)]


def guard_block(tripped):
    info = torch.zeros((nat.GS_INFO_WORDS,), dtype=torch.int64, device=dev())
    if tripped:
        info[nat.GS_INFO_FLAGS] = nat.GS_FLAG_ISECTS
    return info


@pytest.mark.parametrize("n", SIZES)
def test_noise_step_equals_normals_plus_noise(n):
    L = nat.lib()
    t, seed, strength = 2 ** 32 + 5, 2 ** 63 + 12345, 0.75
    means, ls, q, lo = noise_inputs(n, n)
    keep = [x.clone() for x in (ls, q, lo)]
    a, b = means.clone(), means.clone()
    z = M.counter_normals(n, t, seed, dev())
    nat.check(L.gs_mcmc_noise(stream(), n, strength, ls.data_ptr(), q.data_ptr(), lo.data_ptr(), z.data_ptr(), a.data_ptr()), "gs_mcmc_noise")
    rec = torch.zeros((nat.GS_MCMC_REC_WORDS,), dtype=torch.int64, device=dev())
    nat.check(L.gs_mcmc_step_inputs(stream(), strength, t, seed, rec.data_ptr()), "gs_mcmc_step_inputs")
    nat.check(L.gs_mcmc_noise_step(stream(), n, rec.data_ptr(), ls.data_ptr(), q.data_ptr(), lo.data_ptr(), b.data_ptr()), "gs_mcmc_noise_step")
    r = rec.tolist()
    assert r[1] == t and r[2] == seed - 2 ** 64 and r[3] == 0 and np.array([r[0]], dtype=np.int64).view(np.float64)[0] == strength
    assert torch.equal(a, b)
    for x, k in zip((ls, q, lo), keep):
        assert torch.equal(x, k)                                     # log-scales, quaternions and logits keep their bits
    moved = (b != means).any(1)
    opaque = lo == 8.0
    assert not bool((moved & opaque).any())                          # gate ~ e^-99: an opaque Gaussian does not move
    if n >= 3:
        assert bool(moved[~opaque].all())
    # under a tripped guard nothing moves; under a clear one the same move again
    for tripped in (True, False):
        c, info = means.clone(), guard_block(tripped)
        nat.check(L.gs_guard_set(info.data_ptr(), 1 << 20, 1 << 10), "gs_guard_set")
        try:
            nat.check(L.gs_mcmc_noise_step(stream(), n, rec.data_ptr(), ls.data_ptr(), q.data_ptr(), lo.data_ptr(), c.data_ptr()), "gs_mcmc_noise_step")
        finally:
            L.gs_guard_set(None, 0, 0)
        assert torch.equal(c, means if tripped else b)


# ---- the regulariser ----

def run_reg(lo, ls, a, b, loss3=None, v_lo=None, v_ls=None, ws=None):
    L = nat.lib()
    N = lo.numel()
    if ws is None:
        ws = torch.zeros((int(L.gs_mcmc_reg_workspace_floats(N)),), dtype=torch.float32, device=lo.device)
    p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    nat.check(L.gs_mcmc_reg(stream(), N, lo.data_ptr(), ls.data_ptr(), a, b, p(loss3), ws.data_ptr(), p(v_lo), p(v_ls)), "gs_mcmc_reg")
    return ws


@pytest.mark.parametrize("N", [1, 5, 257, 20000])
def test_budget_regulariser_against_the_reference(N):
    a, b = 0.37, 0.053
    g = torch.Generator().manual_seed(N)
    lo = (torch.rand((N,), generator=g) * 24.0 - 12.0).to(dev())
    ls = (torch.rand((N, 3), generator=g) * 11.0 - 9.0).to(dev())
    val, g_lo, g_ls = R.budget_reg(host(lo), host(ls), a, b)
    zero_lo, zero_ls = torch.zeros_like(lo), torch.zeros_like(ls)
    loss3 = torch.tensor([0.25, 0.5, 0.75], device=dev())
    ws = run_reg(lo, ls, a, b, loss3, zero_lo, zero_ls)
    rel = abs(float(ws[0]) - val) / abs(val)
    e_ls = np.abs(host(zero_ls).astype(np.float64) - g_ls) / np.abs(g_ls)
    e_lo = np.abs(host(zero_lo).astype(np.float64) - g_lo) / float(np.float32(a / N))
    print(f"[mcmc step] reg N={N}: value {rel:.2e} relative, scale gradient {e_ls.max() / 2 ** -24:.2f} x 2^-24 relative, "
          f"logit gradient {e_lo.max() / 2 ** -24:.2f} x 2^-24 fl32(a/N)")
    assert rel <= 1e-6
    assert e_ls.max() <= 4 * 2.0 ** -24
    assert e_lo.max() <= 4 * 2.0 ** -24
    assert float(loss3[0]) == 0.25 and float(loss3[1]) == 0.5 and torch.equal(loss3[2], torch.tensor(0.75, device=dev()) + ws[0])
    # added onto what the arrays hold; the same bits again
    v_lo, v_ls = torch.full_like(lo, 0.5), torch.full_like(ls, -0.25)
    ws2 = run_reg(lo, ls, a, b, None, v_lo, v_ls)
    assert torch.equal(ws2[0], ws[0]) and torch.equal(v_lo, 0.5 + zero_lo) and torch.equal(v_ls, -0.25 + zero_ls)
    # each array on its own; the value-only call leaves them alone
    w_lo, w_ls = torch.full_like(lo, 0.5), torch.full_like(ls, -0.25)
    run_reg(lo, ls, a, b, None, w_lo, None)
    run_reg(lo, ls, a, b, None, None, w_ls)
    assert torch.equal(w_lo, v_lo) and torch.equal(w_ls, v_ls)
    ws3 = run_reg(lo, ls, a, b)
    assert torch.equal(ws3[0], ws[0]) and torch.equal(w_lo, v_lo) and torch.equal(w_ls, v_ls)
    # a tripped guard: no value, no gradient, no loss
    info = guard_block(True)
    sentinel = torch.full_like(ws, 7.0)
    nat.check(nat.lib().gs_guard_set(info.data_ptr(), 1 << 20, 1 << 10), "gs_guard_set")
    try:
        run_reg(lo, ls, a, b, loss3, w_lo, w_ls, ws=sentinel)
    finally:
        nat.lib().gs_guard_set(None, 0, 0)
    assert bool((sentinel == 7.0).all()) and torch.equal(w_lo, v_lo) and torch.equal(w_ls, v_ls)
    assert torch.equal(loss3[2], torch.tensor(0.75, device=dev()) + ws[0])


def test_budget_regulariser_of_nothing_launches_nothing():
    ws, loss3 = torch.full((4,), 7.0, device=dev()), torch.full((3,), 0.5, device=dev())
    e = torch.full((4,), 3.0, device=dev())   # (the pointers must be there, as gs_scale_reg's; nothing reads or writes them)
    assert nat.lib().gs_mcmc_reg(stream(), 0, e.data_ptr(), e.data_ptr(), 0.1, 0.1, loss3.data_ptr(), ws.data_ptr(), e.data_ptr(), e.data_ptr()) == 0
    assert bool((ws == 7.0).all()) and bool((e == 3.0).all()) and bool((loss3 == 0.5).all())


# ---- the captured step ----

def scene(n=20000, W=320, H=208, n_views=3, seed=3, sh_degree=3, dist=4.0, n_dead=600, scale_regularization=False, min_abs_logit=0.0):
    sc = make_scene(n, W, H, sh_degree=sh_degree, n_views=n_views, seed=seed, scale_range=(0.01, 0.08), dist=dist)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-2, 1 - 1e-3)
    logit = np.log(op / (1 - op)).astype(np.float32)
    logit[:n_dead] = -7.0     # opacity 0.0009: dead (min_opacity 0.005), and the only ones the noise gate lets move
    near = np.abs(logit) < min_abs_logit
    logit[near] = np.where(logit[near] < 0, -min_abs_logit, min_abs_logit).astype(np.float32)
    shs = T(sc["shs"])
    ls = torch.log(T(sc["scales"]))
    ratio = torch.exp(ls).amax(1) / torch.exp(ls).amin(1)
    extra = dict(use_scale_regularization=True, max_scale_ratio=float(torch.quantile(ratio.double(), 2.0 / 3.0))) if scale_regularization else {}

    def make():
        m = GaussianModel(means=T(sc["means"]), log_scales=ls.clone(), quats=T(sc["quats"]), sh_0=shs[:, :1].contiguous(),
                          sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(logit.copy()), sh_degree=sh_degree, white_background=True,
                          means_lr_schedule_max_steps=40, **extra).to(dev())
        return m, build_optimizers(m, *LRS, fused="hip")

    datas = [{"w2c": T(sc["viewmats"][v]).to(dev()), "K": T(sc["Ks"][v]).to(dev()), "width": W, "height": H} for v in range(n_views)]
    g = torch.Generator().manual_seed(11)
    gts = [torch.rand((H, W, 3), generator=g).to(dev()) for _ in range(n_views)]
    return make, datas, gts


def strategy(model, cap_max=None, refine=None, seed=2 ** 63 + 12345, noise="counter"):
    start, stop, every = refine or (10 ** 9, 10 ** 9, 1)
    return M.MCMCStrategy(model, cap_max=cap_max or model.nbr_gaussians, noise_lr=5e4, refine_start=start, refine_stop=stop,
                          refine_every=every, generator=torch.Generator(device=dev()).manual_seed(5), noise=noise, seed=seed)


def state(m, o):
    out = {}
    for k in m.param_names:
        out[k] = getattr(m, k).detach().clone()
        mm, vv = o.moments_of(getattr(m, k))
        out["m_" + k], out["v_" + k] = mm.clone(), vv.clone()
    for k in ("max_radii", "grad_norm_accum", "collecting_counts"):
        out[k] = getattr(m, k).clone()
    return out


def assert_same(sa, sb, what):
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), (what, k, float((sa[k] - sb[k]).abs().max()))


def close(a, b, rtol=1e-6):
    return abs(float(a) - float(b)) <= rtol * max(abs(float(b)), 1e-30)


REG = (0.02, 0.015)


def eager_step(model, opt, lc, st, data, gt, step, fused=True):
    out = model(data, clamp=False)
    loss = lc.get_loss_dict(out["render_img"], gt)
    reg = st.regularization(*REG, fused=fused)
    total = loss["total"] + reg
    total.backward()
    model.update_statistics(data, out)
    opt.step()
    opt.zero_grad()
    l3 = torch.stack([loss["l1"].detach(), loss["ssim"].detach(), total.detach()])
    return l3, reg.detach(), st.after_step(step)


@pytest.mark.parametrize("sh_degree", [0, 3])
@pytest.mark.parametrize("both", [False, True])
def test_fused_budget_term_equals_the_unfused_chain(both, sh_degree):
    """One step through gs_project_bwd_adam_mcmc against gs_project_bwd -> [gs_scale_reg ->] gs_mcmc_reg -> gs_update_statistics ->
    gs_adam_step_dev: parameters, moments and statistics bit for bit -- and not what a step without the term gives."""
    make, datas, gts = scene(n=6000, sh_degree=sh_degree, scale_regularization=both)
    states, regs = [], []
    for fuse_adam, with_mcmc in ((True, True), (False, True), (True, False)):
        m, o = make()
        lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05) if both else LossComputer(0.2, clamp_input=True)
        r = TrainStepGraph(m, o, lc, datas[0], gts[0], use_graph=False, fuse_adam=fuse_adam, mcmc=strategy(m) if with_mcmc else None,
                           mcmc_reg=REG)
        assert r.scale_reg == both
        out = r.step(datas[0], gts[0])
        r.finish()
        states.append(state(m, o))
        regs.append((out["loss3"].clone(), out["mcmc_reg"].clone() if with_mcmc else None))
    assert_same(states[0], states[1], "fused != unfused")
    assert torch.equal(regs[0][0], regs[1][0]) and torch.equal(regs[0][1], regs[1][1]) and float(regs[0][1]) > 0.0
    assert close(regs[0][0][2], float(regs[2][0][2]) + float(regs[0][1]))
    assert not torch.equal(states[0]["logit_opacities"], states[2]["logit_opacities"])
    assert not torch.equal(states[0]["log_scales"], states[2]["log_scales"])


@pytest.mark.parametrize("binning", ["tiles", "bins"])
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_captured_budget_step_equals_eager(fuse_adam, binning, monkeypatch):
    """Seven steps with a relocate + grow after step 3 (N 20000 -> 21000 = cap_max) and a pure relocate after step 6: the eager
    budget loop against a hipGraph runner and the same sequence issued eagerly."""
    monkeypatch.setenv("GS_BINNING", binning)
    make, datas, gts = scene()
    (ma, oa), (mb, ob), (mc, oc) = make(), make(), make()
    n0 = ma.nbr_gaussians
    sa, sb, sc_ = (strategy(m, cap_max=int(1.05 * n0), refine=(0, 7, 3)) for m in (ma, mb, mc))
    lc = LossComputer(0.2, clamp_input=True)
    rb = TrainStepGraph(mb, ob, lc, datas[0], gts[0], use_graph=True, check_every=2, fuse_adam=fuse_adam, mcmc=sb, mcmc_reg=REG)
    rc = TrainStepGraph(mc, oc, lc, datas[0], gts[0], use_graph=False, check_every=2, fuse_adam=fuse_adam, mcmc=sc_, mcmc_reg=REG)
    rep = rb.report()
    assert rep["mcmc"] and rep["mcmc_reg"] == REG and rep["mcmc_seed"] == 2 ** 63 + 12345
    for it in range(7):
        step, v = it + 1, it % 3
        for m in (ma, mb, mc):
            m.update_learning_rate(it)
        l_ref, reg_ref, info_a = eager_step(ma, oa, lc, sa, datas[v], gts[v], step)
        outs = [r.step(datas[v], gts[v]) for r in (rb, rc)]
        for r in (rb, rc):
            r.finish()
        for out in outs:
            assert torch.equal(out["loss3"][:2], l_ref[:2]), it
            assert close(out["loss3"][2], l_ref[2]) and close(out["mcmc_reg"], reg_ref), (it, float(out["mcmc_reg"]), float(reg_ref))
            assert out["mcmc_reg"].dim() == 0 and float(reg_ref) > 0.0
        assert torch.equal(outs[0]["loss3"], outs[1]["loss3"]) and torch.equal(outs[0]["mcmc_reg"], outs[1]["mcmc_reg"])
        captures = rb.report()["captures"]
        infos = [s.after_step(step, r) for s, r in ((sb, rb), (sc_, rc))]
        if step in (3, 6):
            n_dead = int(info_a["relocate"]["n_dead"])
            assert n_dead >= (100 if step == 3 else 0)   # (some Gaussians ARE dead at the first refinement)
            for info in infos:
                assert int(info["relocate"]["n_dead"]) == n_dead and info["n_new"] == info_a["n_new"] == (1000 if step == 3 else 0)
        else:
            assert infos == [{}, {}] and info_a == {}
        assert ma.nbr_gaussians == mb.nbr_gaussians == mc.nbr_gaussians == (n0 if step < 3 else n0 + 1000)
        assert rb.report()["captures"] == captures          # (after_step itself never re-captures)
        st_a, st_b, st_c = state(ma, oa), state(mb, ob), state(mc, oc)
        assert_same(st_b, st_c, f"step {step}: graph != no graph")
        assert_same(st_b, st_a, f"step {step}: captured != eager")
    for r in (rb, rc):
        rep = r.report()
        assert rep["steps"] == 7 and rep["rebuilds"] >= 2
    # re-captured once, for the grow; the pure relocate after step 6 kept the graph
    assert rb.report()["captures"] == 2 and rb.report()["rebuilds"] == 2 + rb.report()["overflows"]


def test_fused_regulariser_against_the_torch_expression_after_one_step():
    """One eager step with `regularization(fused=True)` against one with the torch expression: every parameter agrees to 1e-6
    relative, element by element.  The scene keeps every raw logit at least 0.25 from zero: Adam's first step moves a logit by its
    learning rate, 0.05, and each path rounds that move on its own, so a logit the move all but cancels (0.0504 -> 0.0004) would
    carry an absolute difference of the rounding of 0.05 against almost nothing of its own size."""
    make, datas, gts = scene(min_abs_logit=0.25)
    (ma, oa), (mb, ob) = make(), make()
    assert float(mb.logit_opacities.detach().abs().min()) >= 0.25
    lc = LossComputer(0.2, clamp_input=True)
    eager_step(ma, oa, lc, strategy(ma), datas[0], gts[0], 1, fused=True)
    eager_step(mb, ob, lc, strategy(mb), datas[0], gts[0], 1, fused=False)
    for k in ma.param_names:
        a, b = getattr(ma, k).detach().double(), getattr(mb, k).detach().double()
        err = float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())
        print(f"[mcmc step] fused against torch regulariser, {k}: {err:.2e} relative")
        assert err <= 1e-6, k


@pytest.mark.parametrize("binning", ["tiles", "bins"])
def test_overflow_replay_draws_the_same_noise(binning, monkeypatch):
    """Capacity learnt from a pulled-back camera with margin 1.02, then close-up views while the host runs ahead: the skipped steps
    are replayed with their own step counter and learning rates, so they draw what they would have drawn -- the final state is
    that of a runner with ample margin, and that of the eager loop, which has no capacity to outgrow, bit for bit.  (Noise from
    torch.randn could not pass this.)"""
    monkeypatch.setenv("GS_BINNING", binning)
    make, datas, gts = scene(n=30000)
    far = dict(datas[0])
    w2c = far["w2c"].clone()
    w2c[2, 3] += 14.0
    far["w2c"] = w2c
    seq = [far, datas[1], datas[2], far, datas[0], datas[1]]
    lc = LossComputer(0.2, clamp_input=True)
    results = []
    for first, margin in ((far, 1.02), (datas[1], 4.0)):
        m, o = make()
        r = TrainStepGraph(m, o, lc, first, gts[0], margin=margin, check_every=4, mcmc=strategy(m), mcmc_reg=REG)
        before = m.means.detach().clone()
        for it, d in enumerate(seq):   # no finish() in between: the host keeps enqueueing behind the overflow
            m.update_learning_rate(it)
            r.step(d, gts[it % 3])
        r.finish()
        results.append((state(m, o), r.report()))
        assert bool((m.means.detach()[:600] != before[:600]).any(1).all())   # the transparent Gaussians were moved by the noise
    (tight, rep_tight), (ample, rep_ample) = results
    print(f"[mcmc step] replay {binning}: margin 1.02 overflowed {rep_tight['overflows']} x and replayed {rep_tight['replayed_steps']} steps, "
          f"margin 4 overflowed {rep_ample['overflows']} x")
    assert rep_tight["overflows"] >= 1 and rep_tight["replayed_steps"] >= 1 and rep_tight["steps"] == len(seq)
    assert rep_ample["steps"] == len(seq) and rep_tight["binning"] == binning
    assert_same(tight, ample, "replayed != ample margin")
    m, o = make()
    st = strategy(m)
    for it, d in enumerate(seq):
        m.update_learning_rate(it)
        eager_step(m, o, lc, st, d, gts[it % 3], it + 1)
    assert_same(tight, state(m, o), "replayed != eager")


def test_without_a_strategy_nothing_is_added():
    make, datas, gts = scene(n=6000)
    m, o = make()
    r = TrainStepGraph(m, o, LossComputer(0.2, clamp_input=True), datas[0], gts[0])
    out = r.step(datas[0], gts[0])
    r.finish()
    assert set(out) == {"render_img", "loss3", "batch_radii", "absgrad"}
    fixed = {"binning", "probed_isects", "probed_longest_list", "probed_coarse_entries", "capacity_isects", "capacity_tile_list",
             "capacity_work_units", "capacity_rows", "probed_work_units", "probed_rows", "seen_work_units", "seen_rows", "steps", "graph",
             "rounds", "round_fraction", "front_round_alone"}
    assert set(r.report()) == fixed | set(r.stats) and not any("mcmc" in k for k in r.report())
    assert r.mcmc is None and "mcmc_reg" not in r.buf and "mcmc_rec" not in r.buf
