"""Every fused Adam path against the fp64 reference of tests/adam_ref.py, at ragged and edge sizes.

All comparisons are ONE step from the device's own fp32 state: p, m, v and the gradient are read back before the step, `adam_ref`
gives the fp64 result, and the device's new p, m, v must lie within `adam_bounds` -- errors never compound, the bounds hold at
every step.  Each test prints the worst observed error / bound per quantity.

* the streaming kernel (csrc/gs_adam.hip: gs_adam_step, gs_adam_step_stats, gs_adam_step_dev fed by gs_adam_hyper and by
  gs_step_inputs): ragged segments and pads, null-gradient subsets, the statistics rider, the grid-stride wrap, magnitude
  regimes, element isolation, step counts;
* the in-place update of the fused projection backward (csrc/gs_project.hip: adam_sh_tile, adam_geo_tile through
  gs_project_bwd_adam / gs_project_bwd_adam_reg): ragged N, every K / active degree, culled Gaussians, the regulariser, the
  captured path.

The sibling variants of that fused kernel -- the budget, row-sums (poses), depth, ortho / fisheye and antialiased instantiations, each
at every SH degree, and the two-range row walk of depth rounds -- are held to the same standard by tests/test_gpu_fused_variants.py,
which generalises `_fused_case` over the variant matrix of tests/fused_variants.py and imports `_fused_setup`, `_check_step`, `Worst`
and the small helpers from here.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

import adam_ref as AR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.optim import FusedAdam
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from scenes import make_scene

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.9, 0.999, 1e-8
LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
NAMES = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _flat(opt):
    """(p, m, v): host copies of the three flat buffers."""
    torch.cuda.synchronize()
    return tuple(x.detach().cpu().numpy().copy() for x in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq))


def _np(g):
    return None if g is None else g.detach().reshape(-1).cpu().numpy()


class Worst:
    """Worst error / bound per quantity and the share of elements under the fp32-range rule, over everything one test checks."""

    def __init__(self):
        self.r = {"p": 0.0, "m": 0.0, "v": 0.0}
        self.flagged = self.n = 0

    def add(self, ratios, n):
        for k in self.r:
            self.r[k] = max(self.r[k], ratios[k])
        self.flagged += ratios["flagged"] * n
        self.n += n

    def share(self):
        return self.flagged / max(self.n, 1)

    def check(self, what):
        print(f"[adam] {what}: worst error / bound  p {self.r['p']:.3f}  m {self.r['m']:.3f}  v {self.r['v']:.3f}   "
              f"fp32-range rule on {100.0 * self.share():.3f} % of {self.n} elements")
        assert self.n > 0, what
        assert self.r["p"] <= 1.0 and self.r["m"] <= 1.0 and self.r["v"] <= 1.0, (what, self.r)
        assert self.share() <= 0.01, (what, self.share())


def _check_step(opt, before, after, grads, lrs, t, worst, gs=1.0, skip=None):
    """One step of `opt` from `before` to `after` (`_flat` snapshots) on `grads` (one flat fp32 array or None per segment):
    updated segments within the bounds, skipped ones bit-identical, every pad float of the three buffers bit-zero.
    `skip`: {segment: boolean mask of elements left out of the comparison}."""
    for i, (o, n, e) in enumerate(zip(opt._offs, opt._lens, opt._ends)):
        for buf in after:
            assert not _bits(buf[o + n:e]).any(), ("pad floats must stay zero", i)
        sl = slice(o, o + n)
        if grads[i] is None or n == 0:
            for a, b in zip(before, after):
                assert _same_bits(a[sl], b[sl]), ("a segment without gradient must not change", i)
            continue
        assert grads[i].shape == (n,)
        keep = slice(None) if skip is None or i not in skip else ~skip[i]
        old = tuple(b[sl][keep] for b in before)
        ref = AR.adam_ref(old[0], grads[i][keep], old[1], old[2], lrs[i], t, B1, B2, EPS, gs)
        worst.add(AR.error_ratios(tuple(a[sl][keep] for a in after), old[0], ref), old[0].size)


def _make_opt(shapes, dev, seed, lrs=None):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    lrs = [LRS[i % 6] for i in range(len(ps))] if lrs is None else lrs
    return ps, FusedAdam([{"params": [p], "lr": lr, "name": NAMES[i] if len(ps) == 6 else f"t{i}"} for i, (p, lr) in enumerate(zip(ps, lrs))])


def _rand_grads(ps, g, scale=1.0):
    return [torch.randn(p.shape, generator=g).to(p.device) * scale for p in ps]


def _step_and_check(ps, opt, grads, worst, **kw):
    """Sets the gradients (None = none), steps, checks against the reference.  Returns the snapshots."""
    for p, gr in zip(ps, grads):
        p.grad = gr
    before = _flat(opt)
    opt.step(**kw)
    after = _flat(opt)
    only = kw.get("only")
    eff = [None if (gr is None or (only is not None and grp.get("name") not in only)) else _np(gr)
           for gr, (grp, _) in zip(grads, opt._plist)]
    _check_step(opt, before, after, eff, [float(grp["lr"]) for grp, _ in opt._plist], opt._step, worst, gs=kw.get("grad_scale", 1.0))
    opt.zero_grad()
    return before, after


# ------------------------------------------------------------------------------------------------ the streaming kernel
def _model_shapes(n, K):
    return [(n, 3), (n, 3), (n, 4), (n, 1, 3), (n, K - 1, 3), (n,)]


RAGGED = {"n7_K1": _model_shapes(7, 1), "n7_K2": _model_shapes(7, 2), "n7_K16": _model_shapes(7, 16),
          "n1_K16": _model_shapes(1, 16), "plain_1d": [(1,), (2,), (3,), (5,), (0,), (6,)]}


@pytest.mark.parametrize("case", sorted(RAGGED))
def test_ragged_segments_and_pads(case):
    """Element counts of every residue mod 4 in every position (an empty tensor and N = 1 among them), three steps."""
    dev = _dev()
    ps, opt = _make_opt(RAGGED[case], dev, seed=3)
    assert opt._lens == [int(np.prod(s)) for s in RAGGED[case]] and any(n % 4 for n in opt._lens)
    g = torch.Generator().manual_seed(5)
    worst = Worst()
    for it in range(3):
        _step_and_check(ps, opt, _rand_grads(ps, g, 10.0 ** (it - 1)), worst)
    assert opt._step == 3
    worst.check(f"ragged segments {case}")


def test_null_gradient_subsets():
    """Each single group alone, each group left out, all null with a statistics rider; `only=` + `advance=False` in two launches
    gives the bits of one full step."""
    dev = _dev()
    ps, opt = _make_opt(_model_shapes(37, 16), dev, seed=7)
    g = torch.Generator().manual_seed(8)
    worst = Worst()
    _step_and_check(ps, opt, _rand_grads(ps, g), worst)   # (moments off zero)
    subsets = [{k} for k in range(6)] + [set(range(6)) - {k} for k in range(6)]
    for sub in subsets:
        grads = [gr if k in sub else None for k, gr in enumerate(_rand_grads(ps, g))]
        _step_and_check(ps, opt, grads, worst)
    # no Adam work at all: only the rider runs
    src = [torch.randn(301, generator=g).to(dev) for _ in range(2)]
    dst = [torch.randn(301, generator=g).to(dev) for _ in range(2)]
    want = [(d + s).cpu().numpy() for d, s in zip(dst, src)]
    before, after = _step_and_check(ps, opt, [None] * 6, worst, stats=(src[0], src[1], dst[0], dst[1]))
    for a, b in zip(before, after):
        assert _same_bits(a, b)
    for d, w in zip(dst, want):
        assert _same_bits(d.cpu().numpy(), w)
    worst.check("null-gradient subsets")
    # one step in two launches
    (pa, oa), (pb, ob) = _make_opt(_model_shapes(37, 16), dev, seed=9), _make_opt(_model_shapes(37, 16), dev, seed=9)
    for it in range(2):
        grads = _rand_grads(pa, g)
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr, gr.clone()
        oa.step()
        ob.step(only=NAMES[:3])
        ob.step(only=NAMES[3:], advance=False)
        assert oa._step == ob._step == it + 1
        for a, b in zip(_flat(oa), _flat(ob)):
            assert _same_bits(a, b), it


@pytest.mark.parametrize("adam_floats", [8, 300000])
@pytest.mark.parametrize("stat_n", [1, 255, 257, 70001])
def test_statistics_rider(stat_n, adam_floats):
    """dst += src exactly, next to Adam work of fewer (2 quads) and of more (75000 quads) threads than the rider needs."""
    dev = _dev()
    ps, opt = _make_opt([(adam_floats,)], dev, seed=11, lrs=[1e-3])
    g = torch.Generator().manual_seed(stat_n)
    src = [torch.randn(stat_n, generator=g).to(dev) for _ in range(2)]
    dst = [torch.randn(stat_n, generator=g).to(dev) for _ in range(2)]
    want = [(d + s).cpu().numpy() for d, s in zip(dst, src)]
    guard = [torch.cat([d, torch.full((8,), 7.0, device=dev)]) for d in dst]   # (what lies behind the destination must not move)
    dst = [gd[:stat_n] for gd in guard]
    worst = Worst()
    _step_and_check(ps, opt, _rand_grads(ps, g), worst, stats=(src[0], src[1], dst[0], dst[1]))
    for gd, w in zip(guard, want):
        got = gd.cpu().numpy()
        assert _same_bits(got[:stat_n], w)
        assert np.all(got[stat_n:] == 7.0)
    worst.check(f"statistics rider stat_n={stat_n} adam={adam_floats}")


def test_grid_stride_wrap():
    """Two segments of 4 (256 * 16 * 256 + 300) + 3 floats in all: more quads than the capped grid has threads, so the
    grid-stride loop takes a second trip; every element within the bounds, the last 2000 included."""
    dev = _dev()
    total = 4 * (256 * 16 * 256 + 300) + 3
    a = 2_000_001
    ps, opt = _make_opt([(a,), (total - a,)], dev, seed=13, lrs=[1e-3, 5e-3])
    assert opt.flat_param.numel() // 4 > 256 * 16 * 256
    worst = Worst()
    g = torch.Generator().manual_seed(14)
    before, after = _step_and_check(ps, opt, _rand_grads(ps, g), worst)
    o, n = opt._offs[1], opt._lens[1]
    assert np.all(after[0][o + n - 2000:o + n] != before[0][o + n - 2000:o + n])   # the tail was reached
    worst.check("grid-stride wrap")


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, 1.0 / 3.0])
def test_magnitude_regimes(grad_scale):
    """|g| over 32 decades, moments at 10^+-3 of it, exact zeros, three grad_scales; g = m = v = 0 leaves p bit-unchanged."""
    dev = _dev()
    n = 60001
    p0, g0, m0, v0 = AR.regime_inputs(n, seed=23)
    ps, opt = _make_opt([(n,)], dev, seed=1, lrs=[1e-3])
    with torch.no_grad():
        opt.flat_param[:n].copy_(torch.from_numpy(p0)); opt.exp_avg[:n].copy_(torch.from_numpy(m0)); opt.exp_avg_sq[:n].copy_(torch.from_numpy(v0))
    opt._step = 2
    worst = Worst()
    before, after = _step_and_check(ps, opt, [torch.from_numpy(g0).to(dev)], worst, grad_scale=grad_scale)
    assert _same_bits(before[0][:n], p0) and opt._step == 3
    still = (g0 == 0) & (m0 == 0) & (v0 == 0)
    assert still.sum() >= 50
    for a, b in zip(before, after):
        assert _same_bits(a[:n][still], b[:n][still])
    worst.check(f"magnitude regimes grad_scale={grad_scale:.3f}")


def test_nan_and_inf_gradients_stay_in_their_element():
    """A NaN and an Inf gradient, each in one lane of a float4 quad, poison that element's p, m, v only."""
    dev = _dev()
    n = 67
    ps, opt = _make_opt([(n,)], dev, seed=15, lrs=[1e-3])
    g = torch.Generator().manual_seed(16)
    worst = Worst()
    _step_and_check(ps, opt, _rand_grads(ps, g), worst)
    grad = torch.randn(n, generator=g)
    bad = {5: float("nan"), 18: float("inf"), 64: float("-inf")}   # lanes 1, 2 and 0 of quads 1, 4 and 16 (the padded tail quad)
    for k, x in bad.items():
        grad[k] = x
    mask = np.zeros(n, dtype=bool)
    mask[list(bad)] = True
    ps[0].grad = grad.to(dev)
    before = _flat(opt)
    opt.step()
    after = _flat(opt)
    for buf in after:
        assert not np.isfinite(buf[:n][mask]).any()
        assert np.isfinite(buf[:n][~mask]).all()
    gz = grad.numpy().copy()
    _check_step(opt, before, after, [gz], [1e-3], opt._step, worst, skip={0: mask})
    worst.check("element isolation")


def _dev_step(opt, grads, t, applied, hyper, via):
    """gs_adam_step_dev on `opt`'s buffers, its hyper-parameters staged by gs_adam_hyper or by gs_step_inputs at step `t`."""
    L = nat.lib()
    st = torch.cuda.current_stream().cuda_stream
    ns = len(opt._plist)
    lrs = (ct.c_float * ns)(*[float(grp["lr"]) for grp, _ in opt._plist])
    if via == "hyper":
        nat.check(L.gs_adam_hyper(st, ns, lrs, B1, B2, t, hyper.data_ptr()), "gs_adam_hyper")
    else:
        nat.check(L.gs_step_inputs(st, ns, lrs, B1, B2, t, hyper.data_ptr(), None, None, None, None, None, None, None), "gs_step_inputs")
    ends, lens = (ct.c_int64 * ns)(*opt._ends), (ct.c_int64 * ns)(*opt._lens)
    gptr = (ct.c_void_p * ns)(*[gr.data_ptr() for gr in grads])
    nat.check(L.gs_adam_step_dev(st, opt.flat_param.numel(), opt.flat_param.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(),
                                 ns, ends, lens, gptr, B1, B2, EPS, 1.0, hyper.data_ptr(), applied.data_ptr()), "gs_adam_step_dev")


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_step_counts_and_the_device_side_bias_corrections(t):
    """At step t the host-formed bias corrections (gs_adam_step) and the two device-staged forms (gs_adam_hyper, gs_step_inputs
    -> gs_adam_step_dev) give the same bits, all within the bounds of the reference; `applied_dev` advances by one."""
    dev = _dev()
    shapes = _model_shapes(33, 4)
    made = [_make_opt(shapes, dev, seed=19) for _ in range(3)]
    g = torch.Generator().manual_seed(20 + t % 7)
    worst = Worst()
    warm = _rand_grads(made[0][0], g)
    for ps, opt in made:   # (moments off zero, the same in all three)
        for p, gr in zip(ps, warm):
            p.grad = gr.clone()
        opt.step(); opt.zero_grad()
    grads = _rand_grads(made[0][0], g, 0.3)
    (pa, oa), (pb, ob), (pc, oc) = made
    oa._step = t - 1
    _step_and_check(pa, oa, [gr.clone() for gr in grads], worst)
    assert oa._step == t
    for opt, via in ((ob, "hyper"), (oc, "inputs")):
        applied = torch.full((1,), 41, dtype=torch.int64, device=dev)
        hyper = torch.zeros(16, device=dev)
        _dev_step(opt, grads, t, applied, hyper, via)
        torch.cuda.synchronize()
        assert int(applied.item()) == 42
        for a, b in zip(_flat(oa), _flat(opt)):
            assert _same_bits(a, b), (t, via)
    worst.check(f"step count t={t}")


# ------------------------------------------------------------------------- the fused projection backward + Adam
W, H = 64, 48


def _fused_setup(N, max_deg, active_deg, reg=False, seed=31):
    """Two identical models + FusedAdam, a quarter of the Gaussians behind the camera, two Adam steps on random gradients
    behind them (every moment non-zero, those of culled Gaussians and inactive coefficients included)."""
    dev = _dev()
    sc = make_scene(N, W, H, sh_degree=max_deg, n_views=1, seed=seed, scale_range=(0.05, 0.3), dist=4.0)
    rng = np.random.default_rng(seed + 1)
    means = sc["means"].copy()
    behind = np.arange(N) % 4 == 1
    means[behind, 2] = -4.0 - rng.uniform(1.0, 3.0, int(behind.sum())).astype(np.float32)   # (view 0 is [I | (0, 0, 4)])
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"]) * 0.5
    ls = torch.log(T(sc["scales"]))
    extra = {}
    if reg:
        ratio = torch.exp(ls).amax(1) / torch.exp(ls).amin(1)
        extra = dict(use_scale_regularization=True, max_scale_ratio=float(torch.quantile(ratio.double(), 0.5)))

    def make():
        m = GaussianModel(means=T(means), log_scales=ls.clone(), quats=T(sc["quats"]), sh_0=shs[:, :1].contiguous(),
                          sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)),
                          sh_degree=max_deg, white_background=True, **extra).to(dev)
        m.active_sh_degree = active_deg
        o = build_optimizers(m, *LRS, fused="hip")
        g = torch.Generator().manual_seed(seed + 2)
        for it in range(2):
            for name in m.param_names:
                p = getattr(m, name)
                p.grad = (torch.randn(p.shape, generator=g) * 0.02).to(dev)
            o.step(); o.zero_grad()
        return m, o

    data = {"w2c": T(sc["viewmats"][0]).to(dev), "K": T(sc["Ks"][0]).to(dev), "width": W, "height": H}
    gt = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(seed + 3)).to(dev)
    return dev, make, data, gt, behind


def _stats(m):
    return {k: getattr(m, k).detach().cpu().numpy().copy() for k in ("max_radii", "grad_norm_accum", "collecting_counts")}


def _fused_case(N, max_deg, active_deg, reg=False):
    dev, make, data, gt, behind = _fused_setup(N, max_deg, active_deg, reg)
    (mu, ou), (mf, of) = make(), make()
    K = (max_deg + 1) ** 2
    ka = (active_deg + 1) ** 2
    assert mu.sh_rest.shape == (N, K - 1, 3) and ou._step == 2
    lcs = [LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.1) if reg else LossComputer(0.2, clamp_input=True) for m in (mu, mf)]
    ru = TrainStepGraph(mu, ou, lcs[0], data, gt, use_graph=False, fuse_adam=False)
    rf = TrainStepGraph(mf, of, lcs[1], data, gt, use_graph=False, fuse_adam=True)
    assert ru.scale_reg == rf.scale_reg == reg
    before_u, before_f = _flat(ou), _flat(of)
    for a, b in zip(before_u, before_f):
        assert _same_bits(a, b)   # (building a runner leaves the state alone)
    for r in (ru, rf):
        r.step(data, gt)
        r.finish()
    after_u, after_f = _flat(ou), _flat(of)
    t = ou._step
    assert t == of._step == 3 and ru.report()["steps"] == rf.report()["steps"] == 1
    lrs = [float(grp["lr"]) for grp, _ in ou._plist]
    # what the runner staged for this step is what t and the learning rates imply
    hyper = ru.buf["hyper"].cpu().numpy()
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    assert hyper[0] == np.float32(1.0 / np.sqrt(1.0 - b2 ** t))
    assert all(hyper[1 + k] == np.float32(float(np.float32(lrs[k])) / (1.0 - b1 ** t)) for k in range(6))
    # culled Gaussians: at least an eighth, at most seven eighths
    radii = ru.buf["radii"].cpu().numpy().reshape(-1)
    culled = radii <= 0
    assert np.array_equal(culled, rf.buf["radii"].cpu().numpy().reshape(-1) <= 0)
    assert culled[behind].all() and 1.0 / 8.0 <= culled.mean() <= 7.0 / 8.0, culled.mean()
    grads = [_np(ru.grads[name]) if ru.grads[name] is not None else None for name in NAMES]
    # their gradient is a dense zero (log-scales with the regulariser excepted) and so is that of the inactive coefficients:
    # the reference then demands the zero-gradient update torch gives a dense `.grad` of zeros -- moments decay, p coasts
    for k, name in enumerate(NAMES):
        if grads[k] is None:
            assert name == "sh_rest" and K == 1
            continue
        rows = grads[k].reshape(N, -1)
        if not (reg and name == "log_scales"):
            assert not rows[culled].any(), name
        assert rows[~culled].any() or name == "sh_rest", name
    if K > 1:
        g_rest = grads[4].reshape(N, K - 1, 3)
        assert not g_rest[:, ka - 1:].any()
        if ka > 1:
            assert g_rest[~culled, :ka - 1].any()
    wu, wf = Worst(), Worst()
    _check_step(ou, before_u, after_u, grads, lrs, t, wu)
    _check_step(of, before_f, after_f, grads, lrs, t, wf)
    tag = f"N={N} K={K} degree={active_deg}{' reg' if reg else ''}"
    wu.check(f"projection backward then streaming Adam, {tag}")   # (a)
    wf.check(f"fused projection backward + Adam, {tag}")          # (b)
    # a culled Gaussian's and an inactive coefficient's first moment is beta1 m, and it did move
    o, n = ou._offs[0], ou._lens[0]
    m_old, m_new = before_f[1][o:o + n].reshape(N, 3)[culled], after_f[1][o:o + n].reshape(N, 3)[culled]
    assert culled.any() and m_old.all() and np.all(m_old != m_new)
    m_old, m_new = m_old.astype(np.float64), m_new.astype(np.float64)
    assert np.all(np.abs(m_new - b1 * m_old) <= AR.C_M * AR.EPS32 * np.abs(b1 * m_old))
    if K > ka:
        o, n = ou._offs[4], ou._lens[4]
        mo = before_f[1][o:o + n].reshape(N, K - 1, 3)[:, ka - 1:].astype(np.float64)
        mn = after_f[1][o:o + n].reshape(N, K - 1, 3)[:, ka - 1:].astype(np.float64)
        assert mo.all() and np.all(np.abs(mn - b1 * mo) <= AR.C_M * AR.EPS32 * np.abs(b1 * mo))
    # (c) fused == unfused, bit for bit
    for a, b, what in zip(after_u, after_f, ("parameters", "exp_avg", "exp_avg_sq")):
        assert _same_bits(a, b), (tag, what, int((_bits(a) != _bits(b)).sum()))
    su, sf = _stats(mu), _stats(mf)
    for k in su:
        assert _same_bits(su[k], sf[k]), (tag, k)
    assert su["collecting_counts"].sum() == (~culled).sum()


@pytest.mark.parametrize("N", [257, 258, 259, 511, 1001])
def test_fused_adam_at_ragged_n(N):
    """K = 16, degree 3: last blocks of 1, 2, 3, 255 and 233 rows -- scalar tails of every width at residues 1, 2 and 3."""
    _fused_case(N, 3, 3)


@pytest.mark.parametrize("K,deg", [(1, 0), (4, 0), (4, 1), (9, 2), (16, 0), (16, 1), (25, 2), (25, 4)])
def test_fused_adam_at_every_k_and_degree(K, deg):
    """adam_sh_tile<0>, <16> and <25>, with inactive coefficients whose gradient is zero and whose moments still decay."""
    max_deg = {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}[K]
    _fused_case(259, max_deg, deg)


@pytest.mark.parametrize("N", [259, 1001])
def test_fused_adam_with_the_regulariser(N):
    """gs_project_bwd_adam_reg: the unfused runner's log-scale gradient already holds the regulariser's."""
    _fused_case(N, 3, 3, reg=True)


def test_captured_fused_step_equals_the_eager_fused_step():
    """use_graph=True, fuse_adam=True at N = 1001, three steps: the path training takes, bit for bit the eager fused runner."""
    dev, make, data, gt, behind = _fused_setup(1001, 3, 3)
    (ma, oa), (mb, ob) = make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    ra = TrainStepGraph(ma, oa, lc, data, gt, use_graph=False, fuse_adam=True)
    rb = TrainStepGraph(mb, ob, lc, data, gt, use_graph=True, fuse_adam=True)
    for it in range(3):
        for r in (ra, rb):
            r.step(data, gt)
            r.finish()
        for a, b, what in zip(_flat(oa), _flat(ob), ("parameters", "exp_avg", "exp_avg_sq")):
            assert _same_bits(a, b), (it, what)
        sa, sb = _stats(ma), _stats(mb)
        for k in sa:
            assert _same_bits(sa[k], sb[k]), (it, k)
    assert oa._step == ob._step == 5 and rb.report()["captures"] >= 1 and rb.report()["overflows"] == 0
