"""Every variant of the fused projection backward + Adam against its unfused chain and the fp64 reference of tests/adam_ref.py.

csrc/gs_project.hip compiles the fused "row reduction + SH backward + projection backward + Adam" kernel once per (SH degree, variant):
the 18 rows of tests/fused_variants.py (plain / poses / depth x the four regulariser masks; ortho / fisheye / antialiased x {none, scale})
x degrees 0 .. 4 = 90 instantiations, each with a register allocation of its own.  `_case` is `_fused_case` of tests/test_gpu_adam_edges.py
over that axis: ONE step of two eager runners (`use_graph=False`) built from identical state -- 64 x 48 frame, one view, a quarter of the
Gaussians behind the camera, two prior Adam steps on random gradients -- one with `fuse_adam=False`, one with `fuse_adam=True`:

1. fused == unfused bit for bit: parameters, exp_avg, exp_avg_sq, max_radii, grad_norm_accum, collecting_counts (poses: the corrected view
   matrix and the camera gradient v_delta too -- sums on one side, rows on the other, GRAD_RTOL of tests/test_gpu_pose_step.py by
   contract, the same bits in every case here);
2. both against `adam_ref` within `adam_bounds` on the gradients the unfused runner left in `grads` (they hold the regulariser, budget
   and depth terms), through `_check_step` / `Worst.check`: no tolerance of this module's own;
3. culled Gaussians (the same set in both runners, between 1/8 and 7/8 of N) and inactive SH coefficients: a dense-zero gradient except
   where a regulariser reaches (which then IS non-zero there), first moments beta1 m within C_M eps32 elsewhere;
4. the variant ran: the fused runner called the row's entry point and no other, `report()` shows its flags, and for every term of the
   row (scale, budget, depth) the same fused step without that term ends elsewhere.

Sizes: every variant at N = 259 with (K, active degree) = (1,0) (4,1) (9,2) (16,3) (25,4) -- one case per instantiation --, at (16,1) and
(25,2) -- inactive coefficients, adam_sh_tile with a run-time active count --, and at K = 16, degree 3 with N = 257 and 1001 (last blocks
of 1 and 233 rows).  Depth rounds (ProjBwdArgs.rblk, the two-range row walk): plain, budget and poses at N = 1001, degrees 0 and 3.

Each case prints the variant tag with the worst error / bound of p, m, v for both runners."""
import numpy as np
import pytest
import torch

import adam_ref as AR
import camera_model_ref as CM
import fused_variants as FV
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.depth_loss import MODES, DepthSupervision
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.mcmc import MCMCStrategy
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from test_gpu_adam_edges import B1, B2, H, NAMES, W, Worst, _bits, _check_step, _flat, _fused_setup, _np, _same_bits, _stats
from test_gpu_pose_step import GRAD_RTOL, _poses

pytestmark = pytest.mark.gpu
LAMBDA_SCALE = 0.1            # (as `_fused_case`)
BUDGET_REG = (0.02, 0.015)    # (opacity_reg, scale_reg) of the budget regulariser, as tests/test_gpu_mcmc_step.py
LAMBDA_DEPTH = 0.1
CAMERA_PARAM = {"ortho": 2.2, "fisheye": 75.0}   # half width in scene units / half field of view in degrees (camera_model_ref.intrinsics)
DEGREE_SWEEP = [(259, 1, 0), (259, 4, 1), (259, 9, 2), (259, 16, 3), (259, 25, 4)]   # (N, K, active degree): one per instantiation
INACTIVE = [(259, 16, 1), (259, 25, 2)]                                              # K != (degree + 1)^2
RAGGED = [(257, 16, 3), (1001, 16, 3)]                                               # last blocks of 1 and 233 rows
SHAPES = DEGREE_SWEEP + INACTIVE + RAGGED
MAX_DEG = {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}
TAGS = [v.tag for v in FV.VARIANTS]
assert tuple(deg for _, _, deg in DEGREE_SWEEP) == FV.DEGREES and all(K == (deg + 1) ** 2 for _, K, deg in DEGREE_SWEEP)


def _gt_depth(dev, seed=41):
    """A positive target inside the scene's depth range with "no measurement" (zero) pixels."""
    g = torch.Generator().manual_seed(seed)
    t = 2.0 + 4.0 * torch.rand((H, W), generator=g)
    t[torch.rand((H, W), generator=g) < 0.15] = 0.0
    assert 0.05 < float((t == 0).float().mean()) < 0.3
    return t.to(dev)


class _Setup:
    """Identical starting states for every runner of one case (`_fused_setup`, with and without the scale regulariser on the model)."""

    def __init__(self, v, N, max_deg, active_deg, depth_mode):
        self.v, self.N, self.depth_mode = v, N, depth_mode
        self.dev, self._make_reg, data, self.gt, self.behind = _fused_setup(N, max_deg, active_deg, reg=True)
        _, self._make_plain, _, _, _ = _fused_setup(N, max_deg, active_deg, reg=False)
        if v.family in CAMERA_PARAM:
            K = torch.from_numpy(CM.intrinsics(v.family, W, H, 1, CAMERA_PARAM[v.family])[0]).to(self.dev)
            data = dict(data, K=K, camera_model=v.family)
        self.data = data
        self.gt_depth = _gt_depth(self.dev) if v.family == "depth" else None

    def runner(self, fuse_adam, scale, budget, lambda_depth=LAMBDA_DEPTH, rounds="off"):
        """(runner, model, optimizer, the fused entry points it called): this variant's family with the given terms."""
        v = self.v
        m, o = (self._make_reg if scale else self._make_plain)()
        if v.family == "aa":
            m.rasterize_mode = "antialiased"
        lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=LAMBDA_SCALE) if scale else LossComputer(0.2, clamp_input=True)
        kw = {}
        if budget:   # (no noise, no relocation: the buffers after the step are Adam's alone)
            kw.update(mcmc=MCMCStrategy(m, cap_max=self.N, noise="counter", noise_lr=0.0, refine_start=10 ** 9, refine_stop=10 ** 9, seed=7),
                      mcmc_reg=BUDGET_REG)
        if v.family == "poses":
            kw.update(poses=_poses(self.dev, seed=5), pose_lr=1e-3)
        if v.family == "depth":
            kw.update(depth=DepthSupervision(lambda_depth, self.depth_mode), gt_depth=self.gt_depth)
        if v.family in CAMERA_PARAM:
            kw.update(camera_model=v.family)
        r = TrainStepGraph(m, o, lc, self.data, self.gt, use_graph=False, fuse_adam=fuse_adam, rounds=rounds, **kw)
        called, ck = [], r._ck

        def recording_ck(rc, what):
            if what.startswith(FV.ENTRY_PREFIX):
                called.append(what)
            return ck(rc, what)
        r._ck = recording_ck
        return r, m, o, called

    def step(self, r):
        kw = {}
        if self.v.family == "poses":
            kw["view_index"] = 0
        if self.v.family == "depth":
            kw["gt_depth"] = self.gt_depth
        out = r.step(self.data, self.gt, **kw)
        r.finish()
        return {k: out[k].detach().clone() for k in ("viewmat", "v_delta") if self.v.family == "poses"}


def _segment(opt, buf, name):
    k = NAMES.index(name)
    return buf[opt._offs[k]:opt._offs[k] + opt._lens[k]]


def _reached(scale, budget):
    """The tensors whose gradient a regulariser reaches on every Gaussian, culled ones included."""
    return ({"log_scales"} if scale else set()) | ({"log_scales", "logit_opacities"} if budget else set())


def _check_flags(v, r, rounds_on):
    rep = r.report()
    assert rep.get("scale_reg", False) == v.scale and rep.get("mcmc", False) == v.budget, rep
    assert rep.get("poses", False) == (v.family == "poses") and rep.get("depth", False) == (v.family == "depth"), rep
    assert rep["rounds"] == rounds_on and not rep["graph"] and rep["steps"] == 1 and rep["overflows"] == 0, rep
    assert r.camera_model == {"ortho": nat.GS_CAMERA_ORTHO, "fisheye": nat.GS_CAMERA_FISHEYE}.get(v.family, nat.GS_CAMERA_PINHOLE)
    assert r.antialiased == (v.family == "aa")
    if v.budget:
        assert rep["mcmc_reg"] == BUDGET_REG and rep["mcmc_noise_lr"] == 0.0
    if v.family == "depth":
        assert rep["lambda_depth"] == LAMBDA_DEPTH


def _case(tag, N, K, active_deg, rounds=False):
    v = FV.BY_TAG[tag]
    max_deg, ka = MAX_DEG[K], (active_deg + 1) ** 2
    shape = (N, K, active_deg)
    depth_mode = MODES[(TAGS.index(tag) + (SHAPES.index(shape) if shape in SHAPES else 0)) % 2]   # (the two modes alternate across the cases)
    s = _Setup(v, N, max_deg, active_deg, depth_mode)
    what = f"{tag} N={N} K={K} degree={active_deg}" + (f" {depth_mode}" if v.family == "depth" else "") + (" two rounds" if rounds else "")
    # the unfused chain (one round, as everywhere) and the fused kernel; depth rounds: an unfused chain in two rounds as well, whose
    # rows -- the same set, summed in the order of the two ranges -- are the fused kernel's
    ru, mu, ou, called_u = s.runner(False, v.scale, v.budget, rounds="on" if rounds else "off")
    rf, mf, of, called_f = s.runner(True, v.scale, v.budget, rounds="on" if rounds else "off")
    assert mu.sh_rest.shape == (N, K - 1, 3) and ou._step == of._step == 2
    before_u, before_f = _flat(ou), _flat(of)
    for a, b in zip(before_u, before_f):
        assert _same_bits(a, b)   # (building a runner leaves the state alone)
    out_u, out_f = s.step(ru), s.step(rf)
    after_u, after_f = _flat(ou), _flat(of)
    t = ou._step
    assert t == of._step == 3
    # 4a. the variant ran: its entry point and no other, its flags
    assert called_f and set(called_f) == {v.entry}, (what, called_f)
    assert not called_u, (what, called_u)
    _check_flags(v, rf, rounds)
    assert ru.scale_reg == rf.scale_reg == v.scale
    lrs = [float(grp["lr"]) for grp, _ in ou._plist]
    hyper = ru.buf["hyper"].cpu().numpy()
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    assert hyper[0] == np.float32(1.0 / np.sqrt(1.0 - b2 ** t))
    assert all(hyper[1 + k] == np.float32(float(np.float32(lrs[k])) / (1.0 - b1 ** t)) for k in range(6))
    # 3. culled Gaussians: the same set in both runners, at least an eighth, at most seven eighths
    radii = ru.buf["radii"].cpu().numpy().reshape(-1)
    culled = radii <= 0
    assert np.array_equal(culled, rf.buf["radii"].cpu().numpy().reshape(-1) <= 0)
    assert culled[s.behind].all() and 1.0 / 8.0 <= culled.mean() <= 7.0 / 8.0, culled.mean()
    if v.family in CAMERA_PARAM:   # ... and so says the fp64 projection of this camera model, on the CPU
        f64 = lambda x: x.detach().cpu().double()
        ref_radii = CM.project(v.family, f64(mu.means), f64(mu.quats), torch.exp(f64(mu.log_scales)), f64(s.data["w2c"])[None],
                               f64(s.data["K"])[None], W, H)[0][0].numpy()
        assert 1.0 / 8.0 <= (ref_radii <= 0).mean() <= 7.0 / 8.0, (ref_radii <= 0).mean()
    grads = [_np(ru.grads[name]) if ru.grads[name] is not None else None for name in NAMES]
    reached = _reached(v.scale, v.budget)
    for k, name in enumerate(NAMES):
        if grads[k] is None:
            assert name == "sh_rest" and K == 1
            continue
        rows = grads[k].reshape(N, -1)
        if name not in reached:
            assert not rows[culled].any(), (what, name)
        elif v.budget:   # the budget term: on every Gaussian
            assert rows[culled].any(axis=1).all(), (what, name)
        else:            # the scale-ratio term: on those beyond the ratio (the median: half of them)
            assert rows[culled].any(), (what, name)
        assert rows[~culled].any() or name == "sh_rest", (what, name)
    if K > 1:
        g_rest = grads[4].reshape(N, K - 1, 3)
        assert not g_rest[:, ka - 1:].any()
        if ka > 1:
            assert g_rest[~culled, :ka - 1].any()
    # 2. both against the fp64 reference
    wu, wf = Worst(), Worst()
    _check_step(ou, before_u, after_u, grads, lrs, t, wu)
    _check_step(of, before_f, after_f, grads, lrs, t, wf)
    wu.check(f"[{what}] unfused chain")
    wf.check(f"[{what}] fused kernel")
    # a culled Gaussian's and an inactive coefficient's first moment is beta1 m where no regulariser reaches, and it did move
    assert culled.any()
    for k, name in enumerate(NAMES):
        if name in reached or grads[k] is None:
            continue
        m_old = _segment(of, before_f[1], name).reshape(N, -1)[culled]
        m_new = _segment(of, after_f[1], name).reshape(N, -1)[culled]
        assert m_old.all() and np.all(m_old != m_new), (what, name)
        m_old, m_new = m_old.astype(np.float64), m_new.astype(np.float64)
        assert np.all(np.abs(m_new - b1 * m_old) <= AR.C_M * AR.EPS32 * np.abs(b1 * m_old)), (what, name)
    if K > ka:
        mo = _segment(of, before_f[1], "sh_rest").reshape(N, K - 1, 3)[:, ka - 1:].astype(np.float64)
        mn = _segment(of, after_f[1], "sh_rest").reshape(N, K - 1, 3)[:, ka - 1:].astype(np.float64)
        assert mo.all() and np.all(np.abs(mn - b1 * mo) <= AR.C_M * AR.EPS32 * np.abs(b1 * mo))
    # 1. fused == unfused, bit for bit
    for a, b, buf in zip(after_u, after_f, ("parameters", "exp_avg", "exp_avg_sq")):
        assert _same_bits(a, b), (what, buf, int((_bits(a) != _bits(b)).sum()))
    su, sf = _stats(mu), _stats(mf)
    for k in su:
        assert _same_bits(su[k], sf[k]), (what, k)
    assert su["collecting_counts"].sum() == (~culled).sum()
    if v.family == "poses":
        assert torch.equal(out_u["viewmat"], out_f["viewmat"]) and not torch.equal(out_f["viewmat"], s.data["w2c"]), what
        # The camera gradient: from the row sums on the fused side, from the rows on the unfused one.  Nothing in the interface promises
        # bits there (GRAD_RTOL of its largest entry is the contract), but every case of this module gives the same bits -- both sides hand
        # project_cam_kernel the same per-Gaussian sums and cam_sum_kernel adds the block partials in a fixed order in fp64 -- so that is
        # what is asserted.
        du, df = out_u["v_delta"].double(), out_f["v_delta"].double()
        rel = float((du - df).abs().max() / du.abs().max())
        print(f"[{what}] v_delta: fused (row sums) against unfused (rows) {rel:.3g} of its largest entry (contract {GRAD_RTOL:g})")
        assert bool(du.any()) and torch.equal(out_u["v_delta"], out_f["v_delta"]), (what, rel)
    # 4b. every term of the variant moves the result: the same fused step without it ends elsewhere
    ablations = [("scale", dict(scale=False, budget=v.budget), ("log_scales",))] * v.scale + \
                [("budget", dict(scale=v.scale, budget=False), ("logit_opacities", "log_scales"))] * v.budget + \
                [("depth", dict(scale=v.scale, budget=v.budget, lambda_depth=0.0), ("means",))] * (v.family == "depth")
    for term, kw, moved in ablations:
        rw, mw, ow, _ = s.runner(True, rounds="on" if rounds else "off", **kw)
        s.step(rw)
        without = _flat(ow)[0]
        for name in moved:
            a, b = _segment(of, after_f[0], name), _segment(ow, without, name)
            assert a.shape == b.shape and not _same_bits(a, b), (what, f"a step without the {term} term moves {name} as one with it does")
    return s, rf, after_f, grads


@pytest.mark.parametrize("N,K,deg", DEGREE_SWEEP)
@pytest.mark.parametrize("tag", TAGS)
def test_every_variant_at_every_degree(tag, N, K, deg):
    """18 variants x degrees 0 .. 4 with K = (degree + 1)^2: each of the 90 instantiations once."""
    _case(tag, N, K, deg)


@pytest.mark.parametrize("N,K,deg", INACTIVE)
@pytest.mark.parametrize("tag", TAGS)
def test_every_variant_with_inactive_coefficients(tag, N, K, deg):
    """K = 16 at degree 1 and K = 25 at degree 2: coefficients beyond the active degree decay, adam_sh_tile takes its active count at
    run time."""
    _case(tag, N, K, deg)


@pytest.mark.parametrize("N,K,deg", RAGGED)
@pytest.mark.parametrize("tag", TAGS)
def test_every_variant_at_ragged_n(tag, N, K, deg):
    """K = 16, degree 3, last blocks of 1 and 233 rows: adam_geo_tile's 0 - 3 float tails in every variant."""
    _case(tag, N, K, deg)


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("tag", ["plain", "plain+budget", "poses"])
def test_variants_in_two_depth_rounds(tag, deg):
    """`rounds="on"`: the rows of a Gaussian lie in two ranges (ProjBwdArgs.rblk; row_sum_wave's two-range walk, in row_sums_kernel for
    poses), on the 64 x 48 frame, both rounds with work.
    Fused in two rounds against unfused in ONE round is NOT bit for bit, for an ordering reason: the gradient rows are the same set, but
    row_sum_wave adds them in items of 64 rows, and the items cut the two ranges laid end to end elsewhere than they cut the one list --
    another association of the same sums (tests/test_gpu_rounds.py holds the two pipelines' gradients to 2e-5 for that reason; measured
    here: the same bits at degree 0 and with poses, other bits for plain and budget at degree 3).  So: the fused kernel against the unfused chain over the SAME two ranges bit
    for bit (all of `_case`, the fp64 reference on that chain's gradients included); the unfused chain in one round within the same
    `adam_bounds` on its own gradients; and between the two chains every gradient within test_gpu_rounds' 2e-5 of its largest entry."""
    N, K = 1001, (deg + 1) ** 2
    s, rf, after_f, grads_on = _case(tag, N, K, deg, rounds=True)
    blk = rf.buf["rounds"].tolist()
    listed = int(rf.buf["info"][0])
    print(f"[{tag} N={N} K={K} degree={deg} two rounds] front round {blk[nat.GS_ROUND_BASE]} of {listed} listed, "
          f"{blk[nat.GS_ROUND_LIVE]} of {rf.tiles} tiles live behind it")
    assert blk[nat.GS_ROUND_LIVE] > 0 and 0 < blk[nat.GS_ROUND_BASE] < listed, (blk, listed)   # (both rounds had work)
    v = FV.BY_TAG[tag]
    r1, m1, o1, _ = s.runner(False, v.scale, v.budget, rounds="off")
    before_1 = _flat(o1)
    s.step(r1)
    after_1 = _flat(o1)
    assert not r1.report()["rounds"]
    w1 = Worst()   # (the one-round chain within the same bounds on its own gradients: both sides of the comparison are held to the reference)
    _check_step(o1, before_1, after_1, [None if r1.grads[name] is None else _np(r1.grads[name]) for name in NAMES],
                [float(grp["lr"]) for grp, _ in o1._plist], o1._step, w1)
    w1.check(f"[{tag} N={N} K={K} degree={deg}] unfused chain in one round")
    same = all(_same_bits(a, b) for a, b in zip(after_1, after_f))
    print(f"[{tag} N={N} K={K} degree={deg} two rounds] fused in two rounds against unfused in one: {'the same bits' if same else 'other bits'}")
    for name, g_on in zip(NAMES, grads_on):
        if g_on is not None:
            g_off = _np(r1.grads[name]).astype(np.float64)
            err = np.abs(g_on.astype(np.float64) - g_off).max() / max(np.abs(g_off).max(), 1e-30)
            assert err <= 2e-5, (tag, name, err)
