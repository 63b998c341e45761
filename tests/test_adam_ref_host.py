"""The fp64 Adam reference and its bounds (tests/adam_ref.py) on the CPU: the reference is torch.optim.Adam in float64, a
correct fp32 `adam1()` stays inside the bounds over the input regimes of tests/test_gpu_adam_edges.py, six wrong ones do not,
and the documented distance to torch's mixed constants is derived."""
import numpy as np
import pytest
import torch

import adam_ref as AR

B1, B2, EPS = 0.9, 0.999, 1e-8
STEPS = (1, 2, 10, 1000, 100000)
SCALES = (1.0, 0.25, 1.0 / 3.0)
N_REGIME = 100_000


def test_reference_is_torch_adam_in_float64():
    """Ten steps with an lr change in between, the double betas 0.9 / 0.999: 1e-12 relative."""
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn(257, generator=g, dtype=torch.float64)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(B1, B2), eps=EPS)
    p, m, v = p0.numpy().copy(), np.zeros(257), np.zeros(257)
    for t in range(1, 11):
        lr = 1e-3 if t <= 6 else 3e-5
        opt.param_groups[0]["lr"] = lr
        grad = torch.randn(257, generator=g, dtype=torch.float64) * 10.0 ** (t % 5 - 2)
        pt.grad = grad.clone()
        opt.step()
        p, m, v, _ = AR.adam_ref(p, grad.numpy(), m, v, lr, t, B1, B2, EPS, promote=False)
        st = opt.state[pt]
        for mine, theirs in ((p, pt.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            theirs = theirs.numpy()
            assert np.abs(mine - theirs).max() <= 1e-12 * np.abs(theirs).max(), t


@pytest.fixture(scope="module")
def regimes():
    return AR.regime_inputs(N_REGIME, seed=17)


def _ratios(regimes, t, gs, wrong=None):
    p, g, m, v = regimes
    ref = AR.adam_ref(p, g, m, v, 1e-3, t, B1, B2, EPS, gs)
    new = AR.adam1_emulated(p, g, m, v, 1e-3, t, B1, B2, EPS, gs, wrong=wrong)
    return AR.error_ratios(new, p, ref)


def test_emulated_adam1_stays_inside_the_bounds(regimes):
    """The bounds are not too tight for a correct kernel: at most 1 everywhere (the maxima sit near one half), and at most 1 %
    of the elements need the fp32-range rule."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "flagged": 0.0}
    for t in STEPS:
        for gs in SCALES:
            r = _ratios(regimes, t, gs)
            for k in worst:
                worst[k] = max(worst[k], r[k])
    print(f"emulated adam1: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}  flagged {worst['flagged']:.4f}")
    assert worst["p"] <= 1.0 and worst["m"] <= 1.0 and worst["v"] <= 1.0, worst
    assert worst["flagged"] <= 0.01, worst
    # ... nor so loose that they mean nothing: a correct kernel uses a fair share of them
    assert worst["p"] >= 0.2 and worst["m"] >= 0.2 and worst["v"] >= 0.2, worst


def test_all_zero_state_leaves_the_parameter_alone():
    p = np.float32([0.75, -3.0, 1e-3])
    z = np.zeros(3, np.float32)
    pn, mn, vn = AR.adam1_emulated(p, z, z, z, 1e-3, 5, B1, B2, EPS)
    assert np.array_equal(pn, p) and not mn.any() and not vn.any()
    p_ref, m_ref, v_ref, _ = AR.adam_ref(p, z, z, z, 1e-3, 5, B1, B2, EPS)
    assert np.array_equal(p_ref, p.astype(np.float64)) and not m_ref.any() and not v_ref.any()


@pytest.mark.parametrize("wrong", ["eps_in_sqrt", "no_bc2", "no_bc1", "beta1_for_v", "scale_after_square", "torch_constants"])
def test_the_bounds_reject_a_wrong_adam(regimes, wrong):
    worst = 0.0
    for t in STEPS:
        for gs in SCALES:
            r = _ratios(regimes, t, gs, wrong=wrong)
            worst = max(worst, r["p"], r["m"], r["v"])
    print(f"{wrong}: worst error / bound {worst:.3g}")
    assert worst > 1.0, (wrong, worst)


def test_distance_between_the_abi_adam_and_torchs_constants():
    """torch's `exp_avg_sq` decays by fl32(0.999) and grows by fl32(0.001) g^2; the ABI's grows by (1 - fl32(0.999)) g^2.  Both
    the first step's v and the stationary v (increment / (1 - decay)) differ by the ratio of the two increments: 1.29e-5."""
    b2 = float(np.float32(0.999))
    assert abs(b2 - 0.99900001287) < 1e-11
    assert float(np.float32(1.0) - np.float32(0.999)) == 1.0 - b2   # 1 - beta2 is exact in fp32
    inc_abi, inc_torch = 1.0 - b2, float(np.float32(0.001))
    rel = inc_torch / inc_abi - 1.0
    print(f"exp_avg_sq: torch's constants vs the ABI's  {rel:.4e} relative = {rel / AR.EPS32:.0f} eps32")
    assert abs(rel - 1.29e-5) < 0.005e-5
    # the same number from the two recurrences, run to their stationary state on a constant gradient
    g2, va, vt = 4.0, 0.0, 0.0
    for _ in range(30000):
        va, vt = b2 * va + inc_abi * g2, b2 * vt + inc_torch * g2
    assert abs(vt / va - 1.0 - rel) < 1e-9
    # it is two hundred times the bound on v: the reference must be the ABI's Adam, torch's constants would not pass
    assert rel > 30 * AR.C_V * AR.EPS32
