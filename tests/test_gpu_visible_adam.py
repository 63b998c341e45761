"""`FusedAdam.step(visible=...)` (gs_adam_step_visible: adam_step_visible_kernel) against the fp64 reference of tests/adam_ref.py.

The reference's six groups at SH degrees 0-4 (widths 3, 3, 4, 3, 3 (K - 1), 1: quads that hold one, two and four Gaussians, an empty
segment at degree 0), N in {1, 3, 255, 256, 257, 1031} (a block's edge, ragged tails, more than one block), non-zero incoming moments,
step counts {1, 2, 1000}, seven masks.  The gradients of culled rows are NaN: a culled row that read its gradient into a result would
show it.

* culled rows: p, m, v keep their bits (`torch.equal` on the old values);
* visible rows: within the derived bounds of tests/adam_ref.py (`error_ratios` <= 1 on p, m, v) -- no tolerance of this module's own;
* all visible, finite gradients: the bits of `step()` without `visible`;
* none visible: the three buffers unchanged, the step count advanced by one;
* every pad float of the three buffers stays bit-zero."""
import numpy as np
import pytest
import torch

import adam_ref as AR
from easy_gaussian_splatting_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.9, 0.999, 1e-8
LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
NAMES = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")
SIZES = (1, 3, 255, 256, 257, 1031)
MASKS = ("all", "none", "alternating", "first", "last", "half", "tenth")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _mask(kind, n, seed):
    i = np.arange(n)
    r = np.random.default_rng(seed)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": i % 2 == 0, "first": i == 0, "last": i == n - 1,
            "half": r.random(n) < 0.5, "tenth": r.random(n) < 0.1}[kind]


def _shapes(n, deg):
    K = (deg + 1) ** 2
    return [(n, 3), (n, 3), (n, 4), (n, 1, 3), (n, K - 1, 3), (n,)]


def _make(n, deg, seed, t0):
    """Parameters + optimizer with non-zero moments, its step count set so that the next step is step t0 + 1."""
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in _shapes(n, deg)]
    opt = FusedAdam([{"params": [p], "lr": lr, "name": name} for p, lr, name in zip(ps, LRS, NAMES)])
    opt.exp_avg.copy_((torch.randn(opt.exp_avg.shape, generator=g) * 0.05).to(dev))
    opt.exp_avg_sq.copy_((torch.rand(opt.exp_avg_sq.shape, generator=g) * 0.01 + 1e-6).to(dev))
    for o, n_el, e in zip(opt._offs, opt._lens, opt._ends):   # the pads hold zeros, as `_build` leaves them
        opt.exp_avg[o + n_el:e] = 0
        opt.exp_avg_sq[o + n_el:e] = 0
    opt._step = t0
    return ps, opt


def _flat(opt):
    torch.cuda.synchronize()
    return tuple(x.detach().clone() for x in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq))


def _grads(ps, seed, poison=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for p in ps:
        gr = torch.randn(p.shape, generator=g) * 0.3
        if poison is not None and p.numel():
            gr[torch.from_numpy(poison)] = float("nan")
        out.append(gr.to(p.device))
    return out


def _check(opt, before, after, grads, seen, worst, only=None, gs=1.0):
    """Culled rows and skipped groups keep their bits; seen rows lie within the bounds; pads stay zero."""
    n = seen.size
    t = opt._step
    for k, ((grp, p), o, n_el, e) in enumerate(zip(opt._plist, opt._offs, opt._lens, opt._ends)):
        for b in after:
            assert not b[o + n_el:e].view(torch.int32).any(), ("pad floats must stay zero", k)
        if n_el == 0:
            continue
        rows = [b[o:o + n_el].view(n, -1) for b in before], [a[o:o + n_el].view(n, -1) for a in after]
        skipped = only is not None and grp["name"] not in only
        keep = torch.from_numpy(np.ones(n, bool) if skipped else ~seen).to(p.device)
        for old, new in zip(*rows):
            assert torch.equal(old[keep].view(torch.int32), new[keep].view(torch.int32)), ("a culled row changed", grp["name"])
        if skipped or not seen.any():
            continue
        s = torch.from_numpy(seen).to(p.device)
        old = [x[s].double().cpu().numpy() for x in rows[0]]
        new = [x[s].cpu().numpy() for x in rows[1]]
        g = grads[k].reshape(n, -1)[s].cpu().numpy()
        assert np.isfinite(g).all()
        ref = AR.adam_ref(old[0], g, old[1], old[2], float(grp["lr"]), t, B1, B2, EPS, gs)
        ratios = AR.error_ratios(tuple(new), old[0], ref)
        for q in "pmv":
            worst[q] = max(worst[q], ratios[q])
        assert ratios["flagged"] == 0.0


def _report(what, worst):
    print(f"[visible adam] {what}: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")
    assert worst["p"] <= 1.0 and worst["m"] <= 1.0 and worst["v"] <= 1.0, (what, worst)


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_masks_steps_and_poisoned_gradients(n, deg):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for j, kind in enumerate(MASKS):
        seen = _mask(kind, n, 100 + j)
        t0 = (0, 1, 999)[j % 3]
        ps, opt = _make(n, deg, 7 + j, t0)
        grads = _grads(ps, 50 + j, poison=~seen)
        for p, g in zip(ps, grads):
            p.grad = g
        before = _flat(opt)
        radii = torch.from_numpy(np.where(seen, 1 + np.arange(n) % 5, -(np.arange(n) % 2)).astype(np.int32)).to(_dev())   # culled: 0 or -1
        opt.step(visible=radii)
        after = _flat(opt)
        assert opt._step == t0 + 1
        _check(opt, before, after, grads, seen, worst)
        if kind == "none":
            for a, b in zip(before, after):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        # a bool mask is the same step
        ps2, opt2 = _make(n, deg, 7 + j, t0)
        for p, g in zip(ps2, grads):
            p.grad = g.clone()
        opt2.step(visible=torch.from_numpy(seen).to(_dev()))
        for a, b in zip(after, _flat(opt2)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kind
    _report(f"N={n} degree={deg}", worst)


@pytest.mark.parametrize("deg", [0, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_all_visible_is_the_dense_step_bit_for_bit(n, deg):
    for t0, gs in ((0, 1.0), (1, 0.5), (999, 1.0)):
        (pa, oa), (pb, ob) = _make(n, deg, 3, t0), _make(n, deg, 3, t0)
        grads = _grads(pa, 11)
        for p, q, g in zip(pa, pb, grads):
            p.grad, q.grad = g, g.clone()
        oa.step(grad_scale=gs)
        ob.step(grad_scale=gs, visible=torch.full((n,), 7, dtype=torch.int32, device=_dev()))
        assert oa._step == ob._step == t0 + 1
        for a, b in zip(_flat(oa), _flat(ob)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (n, deg, t0)


@pytest.mark.parametrize("n", [3, 257, 1031])
def test_only_and_grad_scale_and_camera_rows(n):
    """`only=` still skips its groups, `grad_scale=` still scales, and a [2, N] radii tensor is the call on its row-wise maximum."""
    deg, worst = 3, {"p": 0.0, "m": 0.0, "v": 0.0}
    r = np.random.default_rng(n)
    two = np.where(r.random((2, n)) < 0.4, r.integers(1, 9, (2, n)), 0).astype(np.int32)
    seen = two.max(0) > 0
    only = ("sh_0", "sh_rest", "quats")
    (pa, oa), (pb, ob) = _make(n, deg, 5, 4), _make(n, deg, 5, 4)
    grads = _grads(pa, 13, poison=~seen)
    for p, q, g in zip(pa, pb, grads):
        p.grad, q.grad = g, g.clone()
    before = _flat(oa)
    oa.step(visible=torch.from_numpy(two).to(_dev()), only=only, grad_scale=0.25)
    after = _flat(oa)
    _check(oa, before, after, grads, seen, worst, only=only, gs=0.25)
    ob.step(visible=torch.from_numpy(two.max(0)).to(_dev()), only=only, grad_scale=0.25)
    for a, b in zip(after, _flat(ob)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the second half of a two-launch step: the count does not advance again
    oa.step(visible=torch.from_numpy(two).to(_dev()), only=("means", "log_scales", "logit_opacities"), advance=False)
    assert oa._step == 5
    _report(f"only= / grad_scale= / [2, N] at N={n}", worst)
