"""The device side of refinement -- gs_update_statistics, gs_refine_flags / gs_scan_rows_i32 / gs_refine_apply (csrc/gs_refine.hip)
under model.densify_and_prune, and reset_opacities over FusedAdam -- against the fp64 reference of tests/refine_ref.py, with the
checker and the inputs tests/test_refine_ref_host.py holds the torch path to (model helpers: tests/refine_models.py)."""
import numpy as np
import pytest
import torch

import adam_ref as AR
import refine_ref as RR
from easy_gaussian_splatting_amd import _native as nat
from refine_models import LRS, STEP, build_model, draw_noise, state_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ORDERINGS, assert_margins, check_statistics, statistics_inputs = RR.ORDERINGS, RR.assert_margins, RR.check_statistics, RR.statistics_inputs
OFF = dict(prune_radii=1e9, prune_scale=1e9, min_opacity=0.0)   # nothing is pruned (but split parents)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- gs_update_statistics --------------------------------------------------------------------------------------------------
def _update_statistics(n, max_hw, radii, absgrad, bufs):
    nat.check(nat.lib().gs_update_statistics(_stream(), n, float(max_hw), radii.data_ptr(), absgrad.data_ptr(), bufs[0].data_ptr(),
                                             bufs[1].data_ptr(), bufs[2].data_ptr()), "gs_update_statistics")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_update_statistics_equals_reference(n):
    radii, absgrad, max_hw, mr, acc, cnt = statistics_inputs(n, 300 + n)
    if n > 1:
        assert (radii == 0).any() and (radii < 0).any() and (radii > 0).any() and np.isnan(absgrad[radii <= 0]).all()
        above = mr[radii > 0] > radii[radii > 0] / max_hw
        assert above.any() and (~above).any()
    bufs = [_dev(x.copy()) for x in (mr, acc, cnt)]
    ref, steps = (mr, acc, cnt), []
    for step in range(2):   # the second step: every row's radius and absgrad are its neighbour's
        rad = np.roll(radii, step)
        ag = np.where((rad > 0)[:, None], np.nan_to_num(np.roll(absgrad, step, 0), nan=3e-5), np.nan).astype(np.float32)
        _update_statistics(n, max_hw, _dev(rad), _dev(ag), bufs)
        ref = RR.statistics_ref(rad, ag, max_hw, *ref)
        steps.append(rad)
        err = check_statistics([b.cpu().numpy() for b in bufs], ref, (mr, acc, cnt), steps)
        print(f"[statistics] n={n} step {step + 1}: worst error / bound {err}")


def test_update_statistics_honours_the_step_guard():
    n = 257
    radii, absgrad, max_hw, mr, acc, cnt = statistics_inputs(n, 9)
    absgrad = np.nan_to_num(absgrad, nan=1e-4)
    bufs = [_dev(x.copy()) for x in (mr, acc, cnt)]
    info = torch.zeros(nat.GS_INFO_WORDS, dtype=torch.int64, device=DEV)
    info[nat.GS_INFO_FLAGS] = 1            # a tripped guard: the statistics of a voided step are not taken
    L = nat.lib()
    nat.check(L.gs_guard_set(info.data_ptr(), 1, 1), "gs_guard_set")
    try:
        _update_statistics(n, max_hw, _dev(np.abs(radii) + 1), _dev(absgrad), bufs)
        torch.cuda.synchronize()
    finally:
        L.gs_guard_set(None, 0, 0)
    for b, x in zip(bufs, (mr, acc, cnt)):
        assert np.array_equal(b.cpu().numpy().view(np.uint32), x.view(np.uint32))
    _update_statistics(n, max_hw, _dev(np.abs(radii) + 1), _dev(absgrad), bufs)    # guard cleared: the same call does its work
    assert np.array_equal(bufs[2].cpu().numpy(), cnt + 1)


# ---- gs_refine_flags -------------------------------------------------------------------------------------------------------
def device_flags(inp):
    n, S, th, P = len(inp["counts"]), inp["num_splits"], inp["thresholds"], inp["params"]
    flags = torch.full((3, n), -7, dtype=torch.int32, device=DEV)
    counters = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    acc, cnt, rad, ls, lo = (_dev(x) for x in (inp["grad_norm_accum"], inp["counts"], inp["max_radii"], P["log_scales"], P["logit_opacities"]))
    nat.check(nat.lib().gs_refine_flags(_stream(), n, S, float(th["densify_grad"]), float(th["densify_scale"]), float(th["prune_radii"]),
                                        float(th["prune_scale"]), float(th["min_opacity"]), acc.data_ptr(), cnt.data_ptr(), rad.data_ptr(),
                                        ls.data_ptr(), lo.data_ptr(), flags.data_ptr(), counters.data_ptr()), "gs_refine_flags")
    return flags.cpu().numpy(), counters.cpu().numpy().tolist()


@pytest.mark.parametrize("ordering", list(ORDERINGS))
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 64, 257, 1000])
def test_refine_flags_equal_reference(n, S, ordering):
    """The decisions alone, ties and non-finite rows included (n >= 64): a row with one NaN log-scale has a NaN largest scale,
    as `amax` gives it -- it is cloned, not split, and not pruned by scale, whatever its two finite scales are."""
    inp = RR.make_inputs(n, 1, 77 * n + S, ORDERINGS[ordering], S)
    ref = RR.refine_ref_of(inp)
    assert_margins(inp, ref)
    flags, counters = device_flags(inp)
    RR.compare_decisions(flags, counters, ref)
    if n >= 64:
        assert np.isnan(inp["params"]["log_scales"]).any(-1).sum() == 3 and min(ref["counters"]) > 0


# ---- the whole device path ---------------------------------------------------------------------------------------------------
def _pads_are_zero(opt):
    for o, n, e in zip(opt._offs, opt._lens, opt._ends):
        for buf in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq):
            assert e - (o + n) < 4 and not buf[o + n:e].any(), "a pad between two flat segments is not zero"
    assert opt._ends[-1] == opt.flat_param.numel() == opt.exp_avg.numel() == opt.exp_avg_sq.numel()


def _adam_step_against_reference(m, opt, start, seed):
    """One more Adam step on the device against adam_ref's step from `start` = {name: (p, exp_avg, exp_avg_sq, slack)}, fp64: what
    the reference says the state is now.  `slack`: what the device's parameter may already be off by (the children's means and
    log-scales, the reset logits); it passes through the step unchanged.  Returns the worst error / bound."""
    r = np.random.default_rng(seed)
    grads = {}
    for name in RR.PARAM_NAMES:
        grads[name] = r.standard_normal(tuple(getattr(m, name).shape)).astype(np.float32)
        getattr(m, name).grad = _dev(grads[name])
    opt.step()
    assert opt._step == STEP + 1
    worst = 0.0
    for name, lr in zip(RR.PARAM_NAMES, LRS):
        p0, m0, v0, slack = start[name]
        ok = np.isfinite(p0)                                           # (the non-finite rows stay non-finite: nothing to bound)
        ref = AR.adam_ref(np.where(ok, p0, 0.0), grads[name], m0, v0, lr, STEP + 1, 0.9, 0.999, 1e-8)
        tol_p, tol_m, tol_v, _ = AR.adam_bounds(np.where(ok, p0, 0.0), *ref)
        new = [x.detach().cpu().numpy().astype(np.float64) for x in (getattr(m, name),) + tuple(opt.moments_of(getattr(m, name)))]
        for x, rf, tol, mask in ((new[0], ref[0], tol_p + slack, ok), (new[1], ref[1], tol_m, None), (new[2], ref[2], tol_v, None)):
            err = np.abs(x - rf) if mask is None else np.where(mask, np.abs(x - rf), 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(err == 0, 0.0, err / tol)
            q = np.where(np.isnan(q), np.inf, q)
            worst = max(worst, float(q.max(initial=0.0)))
    return worst


def _start_after_refine(ref):
    start = {}
    cr = ref["child_rows"]
    for name in RR.PARAM_NAMES:
        p0 = ref["params"][name].astype(np.float64)
        slack = np.zeros_like(p0)
        if name == "means":
            p0[cr] = ref["child_means"]
            slack[cr] = RR.C_MU * RR.EPS32 * ref["child_mean_scale"]
        if name == "log_scales":
            p0[cr] = ref["child_log_scales"]
            slack[cr] = RR.C_LS * RR.EPS32 * np.maximum(1.0, np.abs(ref["child_log_scales"]))
        start[name] = (p0, ref["exp_avg"][name].astype(np.float64), ref["exp_avg_sq"][name].astype(np.float64), slack)
    return start


def _run_device_path(inp, seed=9):
    gen = draw_noise(inp, DEV, seed)
    ref = RR.refine_ref_of(inp)
    flags, counters = device_flags(inp)
    m, opt = build_model(inp, DEV, "hip")
    info = m.densify_and_prune(generator=gen)
    ratios = RR.compare_refine(state_of(m, info, flags, counters), ref)
    assert info["n_before"] == len(inp["counts"]) and opt._step == STEP
    _pads_are_zero(opt)
    for buf in (m.grad_norm_accum, m.collecting_counts, m.max_radii):
        assert buf.shape == (ref["n_new"],) and buf.is_cuda and not buf.any()
    return m, opt, ref, ratios


@pytest.mark.parametrize("n,K,S,ordering", [(1, 16, 2, "default"), (64, 1, 1, "default"), (64, 25, 3, "swapped"), (257, 4, 2, "swapped"),
                                            (257, 9, 3, "default"), (1000, 16, 2, "default"), (1000, 25, 1, "default"),
                                            (1000, 1, 3, "swapped"), (1000, 4, 2, "default"), (1000, 9, 1, "swapped")])
def test_device_path_equals_reference(n, K, S, ordering):
    inp = RR.make_inputs(n, K, 31 * n + K + S, ORDERINGS[ordering], S)
    m, opt, ref, ratios = _run_device_path(inp)
    assert_margins(inp, ref)
    worst = _adam_step_against_reference(m, opt, _start_after_refine(ref), n + K)
    print(f"[refine device] n={n} K={K} S={S} {ordering}: {ref['tb_info']}; children off by {ratios} eps32 x scale; "
          f"next Adam step at {worst:.3f} of its bounds")
    assert worst <= 1.0
    if n >= 257:
        assert all(int((ref["kind"] == k).sum()) > 5 for k in ((0, 1, 2) if ordering == "default" else (0, 2)))


def test_device_path_gather_grid_stride_loop():
    """refine_gather_kernel launches at most 65536 x 256 threads per tensor: with K = 25 (72 floats of sh_rest per Gaussian)
    every thread takes a second element once n_new * 72 > 2^24, that is from 233 017 Gaussians on."""
    n, K, S = 250_000, 25, 2
    inp = RR.make_inputs(n, K, 4, dict(RR.DEFAULT_THRESHOLDS, **OFF), S, grad_span=1.003)   # 0.3 % of the rows densified
    m, opt, ref, ratios = _run_device_path(inp)
    assert ref["n_new"] * 3 * (K - 1) > 65536 * 256 and ref["n_new"] >= n
    assert min(ref["tb_info"]["train/densify"].values()) > 50 and len(ref["child_rows"]) > 100
    print(f"[refine device] n={n} K={K}: {ref['tb_info']}; children off by {ratios} eps32 x scale")


@pytest.mark.parametrize("outcome", ["nothing changes", "everything pruned", "every row split", "every row cloned"])
def test_device_path_outcomes_that_empty_a_row_of_work(outcome):
    n, K, S = 300, 4, 2
    th = {"nothing changes": dict(OFF, densify_grad=1e9, densify_scale=0.01),
          "everything pruned": dict(RR.DEFAULT_THRESHOLDS, min_opacity=2.0),
          "every row split": dict(OFF, densify_grad=0.0, densify_scale=0.0),
          "every row cloned": dict(OFF, densify_grad=0.0, densify_scale=1e9)}[outcome]
    inp = RR.make_inputs(n, K, 12, th, S, special=False)
    m, opt, ref, ratios = _run_device_path(inp)
    t = ref["tb_info"]
    want = {"nothing changes": (0, 0, n), "everything pruned": (t["train/densify"]["split"], t["train/densify"]["clone"], 0),
            "every row split": (n, 0, n * S), "every row cloned": (0, n, 2 * n)}[outcome]
    assert (t["train/densify"]["split"], t["train/densify"]["clone"], ref["n_new"]) == want
    assert m.sh_rest.shape == (ref["n_new"], K - 1, 3)
    if outcome == "nothing changes":
        got = state_of(m)
        for what in ("params", "exp_avg", "exp_avg_sq"):
            for k in RR.PARAM_NAMES:
                assert np.array_equal(got[what][k].view(np.uint32), inp[what][k].view(np.uint32)), (what, k)
    if ref["n_new"]:
        assert _adam_step_against_reference(m, opt, _start_after_refine(ref), 3) <= 1.0


# ---- reset_opacities over FusedAdam ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(1, 16), (257, 1), (1000, 25)])
def test_reset_opacities_over_fused_adam(n, K):
    inp = RR.make_inputs(n, K, 50 + n)
    m, opt = build_model(inp, DEV, "hip")
    before = [b.clone() for b in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
    offs, lens = list(opt._offs), list(opt._lens)
    m.reset_opacities()
    assert (list(opt._offs), list(opt._lens)) == (offs, lens) and opt._step == STEP
    _pads_are_zero(opt)
    after = (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)
    for i, (o, ln) in enumerate(zip(offs, lens)):
        for b, a in zip(before, after):
            if i < 5:       # every other segment: bit for bit
                assert torch.equal(b[o:o + ln].view(torch.int32), a[o:o + ln].view(torch.int32)), RR.PARAM_NAMES[i]
    o = offs[5]
    assert not opt.exp_avg[o:o + n].any() and not opt.exp_avg_sq[o:o + n].any()
    ref = RR.reset_opacities_ref(inp["params"]["logit_opacities"], inp["thresholds"]["min_opacity"])
    err = RR.reset_opacities_error(m.logit_opacities.detach().cpu().numpy(), ref)
    start = {k: (inp["params"][k].astype(np.float64), inp["exp_avg"][k].astype(np.float64), inp["exp_avg_sq"][k].astype(np.float64),
                 np.zeros(inp["params"][k].shape)) for k in RR.PARAM_NAMES[:5]}
    with np.errstate(invalid="ignore"):
        start["logit_opacities"] = (ref, np.zeros(n), np.zeros(n), RR.C_OP * RR.EPS32 * np.maximum(1.0, np.abs(ref)))
    worst = _adam_step_against_reference(m, opt, start, n)
    print(f"[reset device] n={n} K={K}: worst error {err:.2f} eps32 max(1, |ref|); next Adam step at {worst:.3f} of its bounds")
    assert err <= RR.C_OP and worst <= 1.0


# ---- gs_scan_rows_i32 ------------------------------------------------------------------------------------------------------
def test_row_scan_carry_loop():
    """One row of more than 1024 chunks of 16384: scan_blocksums_kernel goes round its loop twice and carries the first total."""
    L, n = nat.lib(), 1024 * 16384 + 17
    x = torch.randint(0, 2, (1, n), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    out = torch.empty_like(x)
    ws = torch.empty((int(L.gs_scan_rows_workspace_ints(1, n)),), dtype=torch.int32, device=DEV)
    assert ws.numel() >= 1025
    nat.check(L.gs_scan_rows_i32(_stream(), 1, n, x.data_ptr(), out.data_ptr(), ws.data_ptr()), "gs_scan_rows_i32")
    assert torch.equal(out, torch.cumsum(x, 1, dtype=torch.int32))
