"""`TrainStepGraph(visible_adam=True)` -- gs_project_bwd_selective with `fuse_adam`, gs_adam_step_visible_dev without -- and the eager
`optimizer.step(visible=out["batch_radii"])` on scenes whose visibility is known by construction (tests/visible_scene.py: 64 x 48, two
views; "third": every third Gaussian behind the camera, so 16-byte quads straddle seen and culled rows; "block": [256, 512) behind it,
so a whole block of the fused kernel is culled; "none").  N in {257, 515}, degrees {0, 3, 4}, with and without the scale regulariser.

After one step and after three (per step, on the gradients the unfused selective runner leaves in `grads` -- they hold the
regulariser's term on every Gaussian, culled ones included):
  (i)   culled Gaussians: all six parameters and both moments keep their bits, with the regulariser on as well;
  (ii)  visible Gaussians, fused and unfused: within `adam_bounds` of `adam_ref` (tests/test_gpu_adam_edges.py `_check_step`, as
        tests/test_gpu_fused_variants.py judges the dense variants) -- and fused == unfused bit for bit, which is what lets one set of
        gradients serve both;
  (iii) "none": parameters, moments, statistics and `out` are the dense runner's, bit for bit;
  (iv)  image, loss values, radii and the three statistics buffers of the first step are the dense runner's bit for bit;
  (v)   one more step under the second view changes the culled set; Gaussians culled in every step are still untouched.
Each case asserts its precondition on the step's own radii."""
import numpy as np
import pytest
import torch

import visible_scene as VS
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from test_gpu_adam_edges import LRS, NAMES, Worst, _bits, _check_step, _dev, _flat, _np, _same_bits, _stats

pytestmark = pytest.mark.gpu
LAMBDA_SCALE = 0.1


def _setup(case, N, deg, reg, seed=31):
    dev = _dev()
    sc, behind, both = VS.scene(case, N, deg, seed)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"]) * 0.5
    ls = torch.log(T(sc["scales"]))
    extra = {}
    if reg:
        ratio = torch.exp(ls).amax(1) / torch.exp(ls).amin(1)
        extra = dict(use_scale_regularization=True, max_scale_ratio=float(torch.quantile(ratio.double(), 0.5)))

    def make():
        m = GaussianModel(means=T(sc["means"]), log_scales=ls.clone(), quats=T(sc["quats"]), sh_0=shs[:, :1].contiguous(),
                          sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)),
                          sh_degree=deg, white_background=True, **extra).to(dev)
        m.active_sh_degree = deg
        o = build_optimizers(m, *LRS, fused="hip")
        g = torch.Generator().manual_seed(seed + 2)
        for it in range(2):   # two dense steps on random gradients: every moment non-zero, the culled Gaussians' included
            for name in m.param_names:
                p = getattr(m, name)
                p.grad = (torch.randn(p.shape, generator=g) * 0.02).to(dev)
            o.step(); o.zero_grad()
        return m, o

    datas = [{"w2c": T(sc["viewmats"][v]).to(dev), "K": T(sc["Ks"][v]).to(dev), "width": VS.W, "height": VS.H} for v in range(2)]
    gts = [torch.rand((VS.H, VS.W, 3), generator=torch.Generator().manual_seed(seed + 3 + v)).to(dev) for v in range(2)]
    return make, datas, gts, behind, both


class _Recording(TrainStepGraph):
    """Notes the Adam entries the runner enqueues (the warm-up steps and the capture inside the constructor included)."""

    def _ck(self, rc, what):
        if "adam_step" in what or "project_bwd" in what:
            self.__dict__.setdefault("called", []).append(what)
        return super()._ck(rc, what)


def _runner(make, reg, data, gt, **kw):
    m, o = make()
    lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=LAMBDA_SCALE) if reg else LossComputer(0.2, clamp_input=True)
    r = _Recording(m, o, lc, data, gt, check_every=1, **kw)
    return r, m, o


def _out(r, data, gt):
    out = r.step(data, gt)
    r.finish()
    return {k: v.detach().clone() for k, v in out.items()}


def _element_mask(opt, rows):
    """{segment: mask over its elements} of the Gaussians `rows`."""
    N = rows.size
    return {k: np.repeat(rows, n // N) for k, n in enumerate(opt._lens) if n}


def _rows_unchanged(opt, before, after, rows, what):
    N = rows.size
    for k, (o, n) in enumerate(zip(opt._offs, opt._lens)):
        if n:
            for b, a, buf in zip(before, after, ("p", "m", "v")):
                assert _same_bits(b[o:o + n].reshape(N, -1)[rows], a[o:o + n].reshape(N, -1)[rows]), (what, NAMES[k], buf)


@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("deg", [0, 3, 4])
@pytest.mark.parametrize("N", VS.SIZES)
@pytest.mark.parametrize("case", VS.CASES)
def test_captured_step_updates_what_it_saw(case, N, deg, reg):
    what = f"{case} N={N} degree={deg}" + (" +scale" if reg else "")
    make, datas, gts, behind, both = _setup(case, N, deg, reg)
    rd, md, od = _runner(make, reg, datas[0], gts[0])                               # the dense step
    ru, mu, ou = _runner(make, reg, datas[0], gts[0], visible_adam=True, fuse_adam=False)
    rf, mf, of = _runner(make, reg, datas[0], gts[0], visible_adam=True, fuse_adam=True)
    assert ru.grads is not None and rf.grads is None and ou._step == of._step == od._step == 2
    start = _flat(of)
    for a, b in zip(start, _flat(ou)):
        assert _same_bits(a, b)
    wu, wf = Worst(), Worst()
    seen_ever = np.zeros(N, dtype=bool)
    for it, v in enumerate((0, 0, 0, 1)):   # three steps under view 0, (v) one under view 1
        bu, bf = _flat(ou), _flat(of)
        out_u, out_f = _out(ru, datas[v], gts[v]), _out(rf, datas[v], gts[v])
        au, af = _flat(ou), _flat(of)
        t = ou._step
        assert t == of._step == 3 + it
        radii = out_u["batch_radii"].cpu().numpy().reshape(-1)
        seen = radii > 0
        assert np.array_equal(radii, out_f["batch_radii"].cpu().numpy().reshape(-1))
        # the case's precondition, on the step's own radii
        assert np.array_equal(seen, ~(behind if v == 0 else both)), (what, it)
        if v == 0 and case == "third":
            assert 0.2 <= seen.mean() <= 0.8
        if v == 0 and case == "block":
            assert not seen[256:512].any() and seen[:256].any()
        if v == 0 and case == "none":
            assert seen.all()
        if v == 1 and behind.sum() >= 2:
            assert (seen & behind).any() and (~seen).any()   # the culled set changed, and some stay culled
        seen_ever |= seen
        # (i) culled Gaussians keep their bits -- under the regulariser too, whose term the unfused gradients hold for them
        for opt, b, a, tag in ((ou, bu, au, "unfused"), (of, bf, af, "fused")):
            _rows_unchanged(opt, b, a, ~seen, (what, it, tag))
        grads = [_np(ru.grads[name]) if ru.grads[name] is not None and ru.grads[name].numel() else None for name in NAMES]
        if reg and (~seen).sum() >= 8:   # (the term reaches the half of the Gaussians beyond the median ratio)
            assert grads[1].reshape(N, 3)[~seen].any(), what   # the ignored gradient is not zero: ignoring it is the feature
        # (ii) visible Gaussians within the bounds, on both paths; the same bits on both
        lrs = [float(grp["lr"]) for grp, _ in ou._plist]
        skip = _element_mask(ou, ~seen)
        _check_step(ou, bu, au, grads, lrs, t, wu, skip=skip)
        _check_step(of, bf, af, grads, lrs, t, wf, skip=skip)
        for a, b, buf in zip(au, af, ("parameters", "exp_avg", "exp_avg_sq")):
            assert _same_bits(a, b), (what, it, buf, int((_bits(a) != _bits(b)).sum()))
        su, sf = _stats(mu), _stats(mf)
        for k in su:
            assert _same_bits(su[k], sf[k]), (what, it, k)
        if it == 0 or case == "none":
            # (iv) the forward does not know about the option; (iii) nothing culled: the dense step altogether
            out_d = _out(rd, datas[v], gts[v])
            assert set(out_d) == set(out_f) == set(out_u)
            for k in out_d:
                assert torch.equal(out_d[k], out_f[k]) and torch.equal(out_d[k], out_u[k]), (what, it, k)
            sd = _stats(md)
            for k in sd:
                assert _same_bits(sd[k], sf[k]), (what, it, k)
            if case == "none":
                for a, b, buf in zip(_flat(od), af, ("parameters", "exp_avg", "exp_avg_sq")):
                    assert _same_bits(a, b), (what, it, buf)
            elif it == 0:   # culled Gaussians decay and drift in the dense step: that is what the option removes
                pd = _flat(od)
                assert not _same_bits(pd[0], af[0]) and not _same_bits(pd[1], af[1])
    # (v) what no step saw is where it started
    if (~seen_ever).any():
        _rows_unchanged(of, start, _flat(of), ~seen_ever, (what, "never seen"))
    else:
        assert behind.sum() < 2
    assert set(rf.called) == {"gs_project_bwd_selective"}, rf.called
    assert set(ru.called) == {"gs_project_bwd", "gs_adam_step_visible_dev"}, ru.called
    assert set(rd.called) == {"gs_project_bwd_adam_reg" if reg else "gs_project_bwd_adam"}, rd.called   # the default step is the step as it was
    for r in (ru, rf):
        rep = r.report()
        assert rep["steps"] == 4 and rep["overflows"] == 0, rep
    wu.check(f"[{what}] unfused chain, visible")
    wf.check(f"[{what}] fused kernel, visible")


@pytest.mark.parametrize("case,N,deg,reg", [("third", 257, 3, True), ("block", 515, 3, False), ("none", 257, 0, False), ("third", 515, 4, True)])
def test_eager_loop_equals_the_unfused_captured_step(case, N, deg, reg):
    """model(data), backward, `optimizer.step(visible=out["batch_radii"])`: culled rows untouched, seen rows within the bounds on the
    loop's own gradients -- and within the same bounds on the gradients of the unfused captured step of the same scene."""
    what = f"eager {case} N={N} degree={deg}" + (" +scale" if reg else "")
    make, datas, gts, behind, _ = _setup(case, N, deg, reg)
    m, o = make()
    lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=LAMBDA_SCALE) if reg else LossComputer(0.2, clamp_input=True)
    ru, mu, ou = _runner(make, reg, datas[0], gts[0], visible_adam=True, fuse_adam=False)
    before = _flat(o)
    out = m(datas[0], clamp=False)
    lc.get_loss_dict(out["render_img"], gts[0])["total"].backward()
    grads = [_np(p.grad) if p.grad is not None and p.numel() else None for _, p in o._plist]
    radii = out["batch_radii"]
    assert tuple(radii.shape) == (1, N) and radii.dtype == torch.int32
    o.step(visible=radii)
    after = _flat(o)
    seen = radii.cpu().numpy().reshape(-1) > 0
    assert np.array_equal(seen, ~behind)
    _rows_unchanged(o, before, after, ~seen, what)
    w = Worst()
    lrs = [float(grp["lr"]) for grp, _ in o._plist]
    _check_step(o, before, after, grads, lrs, o._step, w, skip=_element_mask(o, ~seen))
    w.check(f"[{what}] the loop on its own gradients")
    bu = _flat(ou)
    _out(ru, datas[0], gts[0])
    au = _flat(ou)
    for a, b in zip(before, bu):
        assert _same_bits(a, b)
    _rows_unchanged(ou, bu, au, ~seen, what)
    # ... and within the same bounds of the reference on the gradients the unfused captured step left: how (ii) above judges that step
    gu = [_np(ru.grads[name]) if ru.grads[name] is not None and ru.grads[name].numel() else None for name in NAMES]
    wl, wr = Worst(), Worst()
    _check_step(o, before, after, gu, lrs, o._step, wl, skip=_element_mask(o, ~seen))
    _check_step(ou, bu, au, gu, lrs, ou._step, wr, skip=_element_mask(ou, ~seen))
    wl.check(f"[{what}] the loop on the captured step's gradients")
    wr.check(f"[{what}] the unfused captured step")
    same = all(_same_bits(a, b) for a, b in zip(after, au))
    print(f"[{what}] the loop against the unfused captured step: {'the same bits' if same else 'other bits'}")
