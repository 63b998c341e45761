"""The torch path of model.densify_and_prune / reset_opacities / update_statistics, on the CPU with torch.optim.Adam, against the
fp64 reference of tests/refine_ref.py -- and the reference's own checker against deliberate mistakes.  No GPU."""
import copy

import numpy as np
import pytest
import torch

import refine_ref as RR
from easy_gaussian_splatting_amd.model import GaussianModel
from refine_models import STEP, build_model, draw_noise, state_of

ORDERINGS, SWAPPED = RR.ORDERINGS, RR.SWAPPED_THRESHOLDS
assert_margins = RR.assert_margins


# ---- densify_and_prune -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", list(ORDERINGS))
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("K", [1, 4, 16, 25])
def test_torch_path_equals_reference(K, S, ordering):
    n = 300
    inp = RR.make_inputs(n, K, 1000 * K + 10 * S + len(ordering), ORDERINGS[ordering], S)
    assert len(inp["special_rows"]) == RR.N_SPECIAL            # the ties and the non-finite rows ride along in every case
    gen = draw_noise(inp, "cpu", 7)
    ref = RR.refine_ref_of(inp)
    assert_margins(inp, ref)
    m, opt = build_model(inp)
    info = m.densify_and_prune(generator=gen)
    ratios = RR.compare_refine(state_of(m, info), ref)
    print(f"[refine host] K={K} S={S} {ordering}: {ref['tb_info']}, children off by {ratios} eps32")
    t = ref["tb_info"]
    # every class of row and every counter is populated (so none of the comparisons above was empty)
    assert min(t["train/densify"].values()) > 5 and min(t["train/prune"].values()) > 5
    assert all(int((ref["kind"] == k).sum()) > 5 for k in ((0, 1, 2) if ordering == "default" else (0, 2)))
    assert info["n_before"] == n and m.sh_rest.shape == (ref["n_new"], K - 1, 3)
    for buf in (m.grad_norm_accum, m.collecting_counts, m.max_radii):
        assert buf.shape == (ref["n_new"],) and not buf.any()
    assert all(float(opt.state[getattr(m, k)]["step"]) == STEP for k in RR.PARAM_NAMES)


def test_ties_and_nonfinite_rows_decide_as_the_reference_project_does():
    """What the constructed rows must come to, spelled out (the reference is checked here, not only used)."""
    inp = RR.make_inputs(64, 4, 5)
    ref = RR.refine_ref_of(inp)
    b = 64 - RR.N_SPECIAL
    f0, f1, f2 = (ref["flags"][r][b:] for r in range(3))
    #            r==t r>t  g==t g<t  tie-split 3t/3 never NaNavg NaNbig NaNlow NaNsmall -inf NaNop +inf  s=0  split
    assert f0.tolist() == [1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0]
    assert f1.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]   # (the last split's children go by scale)
    assert f2.tolist() == [0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0]
    # an fp64 average would not densify the tie: accum / (1 + 1e-8) < accum
    i = b + 2
    assert inp["grad_norm_accum"][i] / (inp["counts"][i].astype(np.float64) + 1e-8) < np.float32(inp["thresholds"]["densify_grad"])
    # swapped thresholds: a clone that is itself pruned by scale is counted in large_scale
    inp = RR.make_inputs(400, 4, 6, SWAPPED)
    ref = RR.refine_ref_of(inp)
    cloned_and_dropped = (ref["flags"][2] == 0) & (ref["facts"]["avg"] >= np.float32(2e-4)) & (ref["facts"]["smax"] < 0.01) & \
                         (ref["facts"]["smax"] > SWAPPED["prune_scale"]) & (ref["facts"]["opacity"] >= 0.005)
    assert cloned_and_dropped.sum() > 5


def test_margin_move_keeps_every_row():
    moved = 0
    for S in (1, 2, 3):
        for name, th in ORDERINGS.items():
            inp = RR.make_inputs(3000, 1, 40 + S, th, S)
            moved += inp["moved"]
            assert all(v.shape[0] == 3000 for v in inp["params"].values())
            assert_margins(inp, RR.refine_ref_of(inp))
    assert moved > 0    # the generator does put rows inside the margin; they were moved, not dropped


# ---- the checker has teeth -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teeth_case():
    inp = RR.make_inputs(400, 4, 11, RR.DEFAULT_THRESHOLDS, 2)
    ref = RR.refine_ref_of(inp)
    return inp, ref


def _as_got(r):
    return {k: r[k] for k in ("params", "exp_avg", "exp_avg_sq", "tb_info", "flags", "counters")}


def test_checker_accepts_the_reference_itself(teeth_case):
    inp, ref = teeth_case
    assert RR.compare_refine(_as_got(ref), ref) == {"log_scales": pytest.approx(0, abs=1.0), "means": pytest.approx(0, abs=1.0)}


# Deliberate mistakes, each applied to a COPY of the correct result: what an implementation that made it would hand over.
def _reorder(got, order):
    for what in ("params", "exp_avg", "exp_avg_sq"):
        got[what] = {k: v[order] for k, v in got[what].items()}


def _clones_first(got, inp, ref):
    _reorder(got, np.concatenate([np.nonzero(ref["kind"] == k)[0] for k in (0, 2, 1)]))


def _children_row_major(got, inp, ref):
    cr, order = ref["child_rows"], np.arange(ref["n_new"])
    order[cr] = cr[np.lexsort((ref["copy"][cr], ref["src"][cr]))]       # parent by parent instead of copy by copy
    _reorder(got, order)


def _child_parent_moments(got, inp, ref):
    cr = ref["child_rows"]
    for what in ("exp_avg", "exp_avg_sq"):
        for k in RR.PARAM_NAMES:
            got[what][k][cr] = inp[what][k][ref["src"][cr]]


def _grad_gt_for_ge(got, inp, ref):
    """`>` where the average gradient is compared: the Gaussians AT the threshold are not densified -- their clones are missing."""
    fa = ref["facts"]
    tie = (fa["avg"] == np.float32(inp["thresholds"]["densify_grad"])) & ~(fa["smax"] >= np.float32(inp["thresholds"]["densify_scale"]))
    gone = (ref["kind"] == 2) & tie[ref["src"]]
    assert tie.sum() >= 2 and gone.sum() == tie.sum()
    _reorder(got, np.nonzero(~gone)[0])
    got["tb_info"]["train/densify"]["clone"] -= int(tie.sum()); got["tb_info"]["train/nbr_gaussians"] -= int(gone.sum())
    got["flags"][2][tie] = 0; got["counters"][1] -= int(tie.sum())


def _radii_ge_for_gt(got, inp, ref):
    """`>=` where max_radii is compared: the Gaussians AT the threshold are pruned and counted."""
    tie = (ref["facts"]["max_radii"] == np.float32(inp["thresholds"]["prune_radii"])) & (ref["flags"][0] == 1)
    gone = (ref["kind"] == 0) & tie[ref["src"]]
    assert tie.sum() >= 2 and gone.sum() == tie.sum()
    _reorder(got, np.nonzero(~gone)[0])
    got["tb_info"]["train/prune"]["large_radii"] += int(tie.sum()); got["tb_info"]["train/nbr_gaussians"] -= int(gone.sum())
    got["flags"][0][tie] = 0; got["counters"][3] += int(tie.sum()); got["counters"][4] += int(tie.sum())


def _low_opacity_old_only(got, inp, ref):
    old = int((ref["facts"]["opacity"] < np.float32(inp["thresholds"]["min_opacity"])).sum())
    assert old < ref["counters"][2]
    t = got["tb_info"]["train/prune"]
    t["large_radii"] += t["low_opacity"] - old; t["low_opacity"] = old; got["counters"][2] = old


def _scale_div_08(got, inp, ref):
    got["params"]["log_scales"][ref["child_rows"]] += np.float32(np.log(inp["num_splits"]))     # s / 0.8, not s / (0.8 S)


MISTAKES = {f.__name__[1:]: f for f in (_clones_first, _children_row_major, _child_parent_moments, _grad_gt_for_ge, _radii_ge_for_gt,
                                        _low_opacity_old_only, _scale_div_08)}


@pytest.mark.parametrize("mistake", list(MISTAKES))
@pytest.mark.parametrize("with_flags", [False, True])
def test_checker_rejects(teeth_case, mistake, with_flags):
    inp, ref = teeth_case
    bad = copy.deepcopy(_as_got(ref))
    RR.compare_refine(bad, ref)                       # the copy itself is accepted ...
    MISTAKES[mistake](bad, inp, ref)                  # ... and no longer once the mistake is in it
    if not with_flags:   # what the torch path hands over: no flag rows, no counters
        bad["flags"] = bad["counters"] = None
    with pytest.raises(AssertionError):
        RR.compare_refine(bad, ref)


def test_checker_rejects_errors_beyond_the_bounds(teeth_case):
    inp, ref = teeth_case
    for name, C in (("log_scales", RR.C_LS), ("means", RR.C_MU)):
        got = _as_got(ref)
        got["params"] = dict(got["params"])
        x = got["params"][name].copy()
        i = ref["child_rows"][3]
        scale = max(1.0, abs(ref["child_log_scales"][3, 1])) if name == "log_scales" else ref["child_mean_scale"][3, 1]
        x[i, 1] += np.float32(2 * C * RR.EPS32 * scale)
        got["params"][name] = x
        with pytest.raises(AssertionError, match=name):
            RR.compare_refine(got, ref)
        x = ref["params"][name].copy()          # one ulp on a survivor: not a child, no tolerance
        j = int(np.nonzero(ref["kind"] == 0)[0][5])
        x[j, 0] = np.nextafter(x[j, 0], np.float32(np.inf))
        got["params"][name] = x
        with pytest.raises(AssertionError, match="survivor"):
            RR.compare_refine(got, ref)


# ---- the constants ---------------------------------------------------------------------------------------------------------
def test_constants_cover_float32_with_a_factor_of_four():
    """C_LS, C_MU, C_OP: the same formulas in np.float32 against the fp64 reference, every row taken as a split parent."""
    worst = {"ls": 0.0, "mu": 0.0, "op": 0.0}
    n = 4000
    for S in (1, 2, 3):
        for seed in range(4):
            inp = RR.make_inputs(n, 4, 100 + seed, num_splits=S, special=False)
            inp["grad_norm_accum"][:] = 1.0; inp["counts"][:] = 1.0; inp["max_radii"][:] = 0.0         # every row has a high gradient
            th = dict(inp["thresholds"], densify_scale=0.0, prune_scale=1e30, min_opacity=0.0)           # ... is big, and nothing goes
            ref = RR.refine_ref(inp["params"], inp["exp_avg"], inp["exp_avg_sq"], inp["grad_norm_accum"], inp["counts"],
                                inp["max_radii"], inp["noise"], th, S)
            assert ref["n_new"] == n * S and len(ref["child_rows"]) == n * S
            src, copy = ref["src"], np.repeat(np.arange(S), n)
            mu32, ls32 = RR.children_f32(inp["params"], inp["noise"], src, copy, S)
            q = np.abs(ls32 - ref["child_log_scales"]) / (RR.EPS32 * np.maximum(1.0, np.abs(ref["child_log_scales"])))
            u = np.abs(mu32 - ref["child_means"]) / (RR.EPS32 * ref["child_mean_scale"])
            x = inp["params"]["logit_opacities"]
            o = RR.reset_opacities_error(RR.reset_opacities_f32(x, 0.005), RR.reset_opacities_ref(x, 0.005))
            worst = {"ls": max(worst["ls"], float(q.max())), "mu": max(worst["mu"], float(u.max())), "op": max(worst["op"], o)}
    print(f"[refine constants] np.float32 against fp64, in eps32 x scale: {worst}")
    assert 4 * worst["ls"] <= RR.C_LS <= 16 and 4 * worst["op"] <= RR.C_OP <= 16
    assert 4 * worst["mu"] <= RR.C_MU <= 4 * worst["mu"] + 1     # above 16: refine_ref's docstring says why


# ---- reset_opacities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_opacity", [0.005, 0.05])
def test_reset_opacities_torch_path(min_opacity):
    inp = RR.make_inputs(500, 4, 21, dict(RR.DEFAULT_THRESHOLDS, min_opacity=min_opacity))
    x = inp["params"]["logit_opacities"]
    assert np.isnan(x).any() and np.isinf(x).any() and (RR._sigmoid(x) * 0.5 > 2 * min_opacity).sum() > 50 < (RR._sigmoid(x) * 0.5 < 2 * min_opacity).sum()
    m, opt = build_model(inp)
    m.reset_opacities()
    got = state_of(m)
    err = RR.reset_opacities_error(got["params"]["logit_opacities"], RR.reset_opacities_ref(x, min_opacity))
    print(f"[reset host] min_opacity={min_opacity}: worst error {err:.2f} eps32 max(1, |ref|)")
    assert err <= RR.C_OP
    assert not got["exp_avg"]["logit_opacities"].any() and not got["exp_avg_sq"]["logit_opacities"].any()
    for k in RR.PARAM_NAMES[:-1]:
        for what in ("params", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(got[what][k].view(np.uint32), inp[what][k].view(np.uint32)), (what, k)
    assert float(opt.state[m.logit_opacities]["step"]) == STEP


# ---- update_statistics ---------------------------------------------------------------------------------------------------------
def test_statistics_checker_rejects_nan_and_errors_beyond_the_bounds():
    radii, absgrad, max_hw, mr, acc, cnt = RR.statistics_inputs(200, 3)
    ag = np.nan_to_num(absgrad, nan=0.0)
    ref = RR.statistics_ref(radii, ag, max_hw, mr, acc, cnt)
    good = [x.astype(np.float32) for x in ref]
    err = RR.check_statistics(good, ref, (mr, acc, cnt), [radii])
    assert max(err.values()) <= 0.5
    i = np.nonzero(radii > 0)[0][7]
    nan, four_bounds = np.float32(np.nan), np.float32(1 + 4 * 5 * RR.EPS32)
    for which, value in ((0, nan), (1, nan), (2, nan), (0, good[0][i] * four_bounds), (1, good[1][i] * four_bounds), (2, good[2][i] + 1)):
        bad = [x.copy() for x in good]
        bad[which][i] = value
        with pytest.raises(AssertionError):
            RR.check_statistics(bad, ref, (mr, acc, cnt), [radii])
    one = RR.statistics_errors([np.array([0.1, 0.2]), np.array([np.nan, 2e-3]), np.array([1.0, 1.0])],
                               [np.array([0.1, 0.2]), np.array([1e-3, 2e-3]), np.array([1.0, 1.0])], 1)
    assert one == {"max_radii": 0.0, "grad_norm_accum": np.inf, "counts": 0.0}       # a NaN accumulator is an error of any size
    bad = [x.copy() for x in good]                 # an invisible row that changed at all
    bad[1][np.nonzero(radii <= 0)[0][0]] += np.float32(1e-7)
    with pytest.raises(AssertionError, match="never visible"):
        RR.check_statistics(bad, ref, (mr, acc, cnt), [radii])


def test_update_statistics_torch_branch():
    for n in (1, 65, 1000):
        radii, absgrad, max_hw, mr, acc, cnt = RR.statistics_inputs(n, n)
        m = GaussianModel(torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 4), torch.zeros(n, 1, 3), torch.zeros(n, 0, 3),
                          torch.zeros(n), sh_degree=0)
        m.max_radii, m.grad_norm_accum, m.collecting_counts = (torch.from_numpy(x.copy()) for x in (mr, acc, cnt))
        xys = torch.zeros(1, n, 2)
        ref, steps = (mr, acc, cnt), []
        for step in range(2):
            rad = np.roll(radii, step)
            ag = np.where((rad > 0)[:, None], np.nan_to_num(np.roll(absgrad, step, 0), nan=1e-4), np.nan).astype(np.float32)
            xys.absgrad = torch.from_numpy(ag)[None]
            m.update_statistics({"height": 300, "width": max_hw}, {"batch_radii": torch.from_numpy(rad)[None], "batch_xys": xys})
            ref = RR.statistics_ref(rad, ag, max_hw, *ref)
            steps.append(rad)
            got = [x.numpy() for x in (m.max_radii, m.grad_norm_accum, m.collecting_counts)]
            RR.check_statistics(got, ref, (mr, acc, cnt), steps)
