"""fp64 reference of the refinement stages: update_statistics, densify_and_prune, reset_opacities.

Written from the reference project's model/gaussian.py (`update_statistics`, `_get_split_gaussians`, `_get_clone_gaussians`,
`densify_and_prune`, `reset_opacities`) in numpy, without torch and without anything from the package.  The package has three
implementations of these stages -- the torch path of `model.py`, `gs_update_statistics` (csrc/gs_adam.hip) and the kernels of
csrc/gs_refine.hip -- and `compare_refine` is the one checker all of them are held to.

What the contract is
--------------------
The contract is the reference project RUNNING IN FLOAT32.  A plain fp64 evaluation disagrees with a correct fp32
implementation at a few places, and those are modelled here, not tolerated:

  * every threshold is rounded to float32 first (the C ABI takes `float`; torch compares a float32 tensor with a Python
    scalar in float32);
  * `avg = accum / (counts + 1e-8)` is formed in np.float32: in float32 `1 + 1e-8 == 1`, so `accum == threshold` with
    `counts == 1` IS densified, which an fp64 evaluation gets wrong.  Division is correctly rounded on every side.  A NaN
    average becomes 0;
  * `max_radii` is compared as stored, with strict `>`;
  * the largest scale and the opacity pass through exp / sigmoid and are formed in fp64.  Their last bits differ between libm
    implementations, so a decision is only defined where the value is not AT the threshold: `refine_ref` returns every row's
    relative distance to every threshold it is compared with ("margins"; the children's `smax / (0.8 S)` included), and
    `make_inputs` MOVES rows that come closer than `MARGIN` = 1e-4 (no row is ever left out of a comparison);
  * non-finite rows follow `amax` and IEEE comparisons: a NaN in any log-scale makes the row's largest scale NaN and every
    comparison with it false (such a row is cloned, never split, and never pruned by scale); logit = -inf is low opacity, a
    NaN logit is not.

Row order of the result: [survivors, in their old order | children of split parents, copy-major | clones].  New rows carry
`max_radii = 0`, so the prune-by-radius threshold is assumed non-negative (a negative one is out of scope).

Tolerances (eps32 = 2^-23, the spacing of float32 at 1)
--------------------------
Everything is compared bit for bit -- n_new, flag rows, counters, tb_info, survivors, clones, the children's quats / sh_0 /
sh_rest / logits, every moment, the row order -- except the children's means and log-scales:

    log-scale:  |d|   <= C_LS eps32 max(1, |ref|)
    mean:       |d_i| <= C_MU eps32 (|mu_i| + sum_j |R_ij| s_j |noise_j|)
    statistics: max_radii within 1.5 ulp of r / max_hw (the kernel multiplies by the rounded reciprocal: 2^-24 relative, at most
                1 ulp of the result, plus half an ulp of the product); grad_norm_accum within (3 + steps) eps32 |ref| (square-sum, root,
                product: 3, one addition per step; all terms positive); counts exact
    opacity reset:  |d| <= C_OP eps32 max(1, |ref|)

The constants come from the same formulas evaluated in np.float32 (`children_f32`, `reset_opacities_f32`) against this fp64
reference -- never from the code under test -- on the generator's own inputs (3 x 4 sets of 4000 rows, every row taken as a
split parent, S = 1, 2, 3), times 4 for the difference between libm implementations, rounded up.
tests/test_refine_ref_host.py repeats the measurement and asserts 4 x ratio <= C:

                                   log-scale    mean     opacity reset
    measured np.float32 ratio      2.06         12.44    0.76            (units of eps32 x the bound's scale)
    constant                       C_LS = 9     C_MU = 50    C_OP = 4

C_MU is above 16 because the bound's scale, |mu_i| + sum_j |R_ij| s_j |noise_j|, weighs each term of the offset by the rotation
entry it is multiplied with, while a float32 rotation entry carries an ABSOLUTE error of a few eps32 (q is normalised, then
1 - 2 (y^2 + z^2) and 2 (x y - w z) cancel).  Where a small |R_ij| meets the largest scale of an anisotropic Gaussian -- the rows
spread their scales over a factor of e^3 -- and |mu_i| is small too, the error eps32 s_j |noise_j| is large against
|R_ij| s_j |noise_j|.  The ratio has that heavy tail and a light body: its worst over 144 000 float32 samples is 12.4, over the
few hundred children of one test case 1 to 5.  (tests/test_gpu_refine.py allows 2e-6 x the largest |mean| of the whole tensor, about
17 eps32 of a scale that is usually far larger than one row's.)  A wrong rotation convention, a wrong noise row or a missing
scale are errors of order 1, millions of eps32.

Worst device error on an MI355X, tests/test_gpu_refine_ref.py (gfx950, in units of each bound):

    children's log-scales   1.91 eps32 max(1, |ref|)                    bound C_LS = 9
    children's means        5.00 eps32 (|mu_i| + sum_j ...)             bound C_MU = 50   (n = 250 000; 4.69 at n = 1000)
    opacity reset           1.23 eps32 max(1, |ref|)                    bound C_OP = 4
    max_radii               0.63 of 1.5 ulp
    grad_norm_accum         0.27 of (3 + steps) eps32 |ref|
    counts                  exact
    next Adam step          0.991 of tests/adam_ref.py's bounds (the half ulp of p itself, as that module explains)

The torch path on the CPU (tests/test_refine_ref_host.py): log-scales 0.74, means 14.5 (one child in 24 cases; 1 to 2 otherwise),
opacity reset 0.65.
"""
import numpy as np

EPS32 = 2.0 ** -23   # np.finfo(np.float32).eps: one ulp of 1.0 (tests/adam_ref.py counts in half of it)
MARGIN = 1e-4
C_LS, C_MU, C_OP = 9.0, 50.0, 4.0
PARAM_NAMES = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")
FLAG_NAMES = ("old row survives", "split children survive", "clone survives")
COUNTER_NAMES = ("split", "clone", "low_opacity", "low_opacity | large_radii", "low_opacity | large_radii | large_scale")
DEFAULT_THRESHOLDS = dict(densify_grad=0.0002, densify_scale=0.01, prune_radii=0.15, prune_scale=0.1, min_opacity=0.005)
# prune-by-scale BELOW the split threshold: clones pruned by scale, and of the children only those of the smallest parents stay
SWAPPED_THRESHOLDS = dict(DEFAULT_THRESHOLDS, prune_scale=0.008)
ORDERINGS = {"default": DEFAULT_THRESHOLDS, "swapped": SWAPPED_THRESHOLDS}


def _f32(x) -> float:
    """The double a float32 implementation sees for a Python scalar."""
    return float(np.float32(x))


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


# ---- update_statistics -----------------------------------------------------------------------------------------------------
def statistics_ref(radii_i32, absgrad, max_hw, max_radii, grad_norm_accum, counts):
    """One `update_statistics` step in fp64: for rows with radius > 0, max_radii = max(max_radii, r / max_hw),
    grad_norm_accum += |absgrad|_2 max_hw, counts += 1.  Every other row is returned unchanged, whatever its absgrad holds."""
    r = np.asarray(radii_i32).astype(np.int64)
    g = np.asarray(absgrad, dtype=np.float64).reshape(-1, 2)
    mh = _f32(max_hw)
    mr, acc, cnt = (np.asarray(x, dtype=np.float64) for x in (max_radii, grad_norm_accum, counts))
    vis = r > 0
    with np.errstate(invalid="ignore", over="ignore"):
        new_mr = np.where(vis, np.maximum(mr, r / mh), mr)
        new_acc = np.where(vis, acc + np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2) * mh, acc)
        new_cnt = np.where(vis, cnt + 1.0, cnt)
    return new_mr, new_acc, new_cnt


def statistics_errors(got, ref, steps):
    """Worst errors of (max_radii, grad_norm_accum, counts) `got` after `steps` consecutive steps, each in units of its bound:
    visible rows against the tolerances of the module docstring; rows never visible must be checked bit for bit by the caller."""
    out = {}
    mr, acc, cnt = (np.asarray(x, dtype=np.float64) for x in got)
    with np.errstate(invalid="ignore", divide="ignore"):
        ulp = np.spacing(np.abs(ref[0]).astype(np.float32)).astype(np.float64)
        for name, e, tol in (("max_radii", np.abs(mr - ref[0]), 1.5 * ulp),
                             ("grad_norm_accum", np.abs(acc - ref[1]), (3 + steps) * EPS32 * np.abs(ref[1]))):
            q = np.where(e == 0, 0.0, e / tol)
            q = np.where(np.isnan(q), np.inf, q)          # a NaN where the reference has a number is an error of any size
            out[name] = float(q.max(initial=0.0))
    out["counts"] = 0.0 if np.array_equal(cnt, ref[2]) else np.inf
    return out


def statistics_inputs(n, seed):
    """radii (zero, negative, positive), absgrad (NaN where invisible), existing statistics above and below the step's value."""
    r = np.random.default_rng(seed)
    radii = r.integers(1, 400, n).astype(np.int32)
    kind = r.random(n)
    radii[kind < 0.2] = 0
    radii[(kind >= 0.2) & (kind < 0.3)] = -r.integers(1, 50, n)[(kind >= 0.2) & (kind < 0.3)].astype(np.int32)
    absgrad = (10.0 ** r.uniform(-8, -2, (n, 2))).astype(np.float32)
    absgrad[radii <= 0] = np.nan
    max_hw = 517
    max_radii = (r.integers(1, 400, n) / max_hw * r.choice([0.5, 1.0, 2.0], n)).astype(np.float32)
    accum = (r.uniform(0, 3, n) * 2e-4).astype(np.float32)
    counts = r.integers(0, 5, n).astype(np.float32)
    return radii, absgrad, max_hw, max_radii, accum, counts


def check_statistics(got, ref, old, radii_steps):
    """`got` (float32 arrays) after len(radii_steps) steps from `old` against `ref`: the bounds on rows that were visible in a
    step, the bits of `old` on the others.  Returns the worst error / bound of each statistic."""
    seen = np.zeros(len(old[0]), dtype=bool)
    for r in radii_steps:
        seen |= np.asarray(r) > 0
    for g, o in zip(got, old):
        assert np.array_equal(g[~seen].view(np.uint32), o[~seen].view(np.uint32)), "a row that was never visible changed"
    err = statistics_errors([g[seen] for g in got], [x[seen] for x in ref], len(radii_steps))
    for name, e in err.items():
        assert e <= 1.0, f"{name}: {e} of its bound"       # (each on its own: false for a NaN, whatever its place)
    return err


# ---- densify_and_prune -----------------------------------------------------------------------------------------------------
def _rotmat(q):
    """wxyz quaternions [M, 4] (normalised here, F.normalize's eps of 1e-12) -> [M, 3, 3]."""
    q = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y ** 2 + z ** 2), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x ** 2 + z ** 2), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x ** 2 + y ** 2)], axis=-1)
    return R.reshape(-1, 3, 3)


def _rel(x, thr):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(x / thr - 1.0)
    return np.where(np.isnan(d), np.inf, d)   # a NaN is compared false whatever the threshold: it has no razor


def margins(log_scales, logit_opacities, thresholds, num_splits):
    """Relative distance of every row from every transcendental threshold it is compared with."""
    th = {k: _f32(v) for k, v in thresholds.items()}
    with np.errstate(invalid="ignore", over="ignore"):
        smax = np.exp(np.asarray(log_scales, dtype=np.float64)).max(-1) if len(log_scales) else np.zeros(0)
    return {"densify_scale": _rel(smax, th["densify_scale"]), "prune_scale": _rel(smax, th["prune_scale"]),
            "child_prune_scale": _rel(smax / (0.8 * num_splits), th["prune_scale"]),
            "min_opacity": _rel(_sigmoid(logit_opacities), th["min_opacity"])}


def refine_ref(params, exp_avg, exp_avg_sq, grad_norm_accum, counts, max_radii, noise, thresholds, num_splits):
    """`densify_and_prune` of the reference project.  `params`, `exp_avg`, `exp_avg_sq`: dicts of float32 arrays keyed by
    PARAM_NAMES; `noise` [S, N, 3]: the standard-normal samples, child j of Gaussian i takes noise[j, i].
    Returns a dict: "n_new"; "params" / "exp_avg" / "exp_avg_sq" (float32: copies are exact; the children's means and log-scales
    there are the rounded fp64 values); "kind" (0 survivor, 1 child, 2 clone), "src" (old row) and "copy" (which child) per new row; "child_rows",
    "child_means", "child_log_scales" (fp64), "child_mean_scale" (|mu_i| + sum_j |R_ij| s_j |noise_j|); "flags" [3, N] as
    gs_refine_flags defines them; "counters" [5]; "tb_info"; "margins"; and "facts": per old row what the decisions saw."""
    S, f = int(num_splits), np.float32
    th = {k: _f32(v) for k, v in thresholds.items()}
    N = params["means"].shape[0]
    with np.errstate(all="ignore"):
        avg = np.asarray(grad_norm_accum, dtype=f) / (np.asarray(counts, dtype=f) + f(1e-8))          # float32, on purpose
        avg = np.where(np.isnan(avg), f(0), avg)
        high = avg >= f(th["densify_grad"])
        scales = np.exp(params["log_scales"].astype(np.float64))
        smax = scales.max(-1) if N else np.zeros(0)                                                     # (np.max propagates NaN, as amax)
        big = smax >= th["densify_scale"]
        split, clone = big & high, ~big & high
        sidx, cidx = np.nonzero(split)[0], np.nonzero(clone)[0]
        ns, nc = len(sidx), len(cidx)
        rep, copy = np.tile(sidx, S), np.repeat(np.arange(S), ns)      # .repeat(NUM_SPLITS, 1): [parents..., parents...]
        nz = np.asarray(noise, dtype=np.float64)[copy, rep] if ns else np.zeros((0, 3))
        R = _rotmat(params["quats"][rep].astype(np.float64))
        sn = scales[rep] * nz
        mu = params["means"][rep].astype(np.float64)
        child_means = mu + np.einsum("mij,mj->mi", R, sn)
        child_mean_scale = np.abs(mu) + np.einsum("mij,mj->mi", np.abs(R), np.abs(sn))
        child_ls = np.log(scales[rep] / (0.8 * S))
        # [old | children | clones]
        parts = [(np.arange(N), 0, np.full(N, -1)), (rep, 1, copy), (cidx, 2, np.full(nc, -1))]
        src = np.concatenate([p[0] for p in parts]).astype(np.int64)
        kind = np.concatenate([np.full(len(p[0]), p[1]) for p in parts])
        cpy = np.concatenate([p[2] for p in parts])
        is_child = kind == 1
        ls_cat = params["log_scales"][src].astype(np.float64)
        ls_cat[is_child] = child_ls
        mu_cat = params["means"][src].astype(np.float64)
        mu_cat[is_child] = child_means
        mscale_cat = np.zeros_like(mu_cat)
        mscale_cat[is_child] = child_mean_scale
        max_radii_cat = np.where(kind == 0, np.asarray(max_radii, dtype=f)[src], f(0))                  # new rows: zeros
        was_split = np.where(kind == 0, split[src], False)
        low = _sigmoid(params["logit_opacities"][src]) < th["min_opacity"]
        big_r = max_radii_cat > f(th["prune_radii"])
        big_s = (np.exp(ls_cat).max(-1) if len(src) else np.zeros(0)) > th["prune_scale"]
        c0, c1, c2 = int(low.sum()), int((low | big_r).sum()), int((low | big_r | big_s).sum())
        keep = ~(low | big_r | big_s | was_split)
    src_o, kind_o = src[keep], kind[keep]
    n_new = int(keep.sum())
    out_p, out_m, out_v = {}, {}, {}
    for name in PARAM_NAMES:
        out_p[name] = params[name][src_o].copy()
        sel = (kind_o == 0).reshape((-1,) + (1,) * (params[name].ndim - 1))
        out_m[name] = np.where(sel, exp_avg[name][src_o], f(0))
        out_v[name] = np.where(sel, exp_avg_sq[name][src_o], f(0))
    child_rows = np.nonzero(kind_o == 1)[0]
    out_p["means"][child_rows] = mu_cat[keep][child_rows].astype(f)
    out_p["log_scales"][child_rows] = ls_cat[keep][child_rows].astype(f)
    flags = np.zeros((3, N), dtype=np.int32)
    flags[0] = keep[:N]
    first = is_child & (cpy == 0)
    flags[1, src[first]] = keep[first]
    for j in range(1, S):   # the copies of one parent share opacity and scales: one decision
        assert np.array_equal(keep[is_child & (cpy == j)][np.argsort(src[is_child & (cpy == j)], kind="stable")],
                              keep[first][np.argsort(src[first], kind="stable")])
    flags[2, src[kind == 2]] = keep[kind == 2]
    tb_info = {"train/densify": {"split": ns, "clone": nc},
               "train/prune": {"low_opacity": c0, "large_radii": c1 - c0, "large_scale": c2 - c1},
               "train/nbr_gaussians": n_new}
    return {"n_new": n_new, "params": out_p, "exp_avg": out_m, "exp_avg_sq": out_v, "kind": kind_o, "src": src_o, "copy": cpy[keep],
            "child_rows": child_rows, "child_means": mu_cat[keep][child_rows], "child_log_scales": ls_cat[keep][child_rows],
            "child_mean_scale": mscale_cat[keep][child_rows], "flags": flags, "counters": [ns, nc, c0, c1, c2], "tb_info": tb_info,
            "margins": margins(params["log_scales"], params["logit_opacities"], thresholds, S),
            "facts": {"avg": avg, "smax": smax, "opacity": _sigmoid(params["logit_opacities"]), "max_radii": np.asarray(max_radii)}}


def _bits_differ(a, b):
    """Indices (flat, first axis) where two float32 arrays differ in their bits (two NaNs count as equal)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    return np.nonzero(bad.reshape(len(a), -1).any(-1))[0] if a.ndim else np.nonzero(bad)[0]


def _row_facts(ref, i):
    fa = ref["facts"]
    return f"avg grad {fa['avg'][i]!r}, largest scale {fa['smax'][i]!r}, opacity {fa['opacity'][i]!r}, max_radii {fa['max_radii'][i]!r}"


def compare_decisions(flags, counters, ref):
    """The three 0/1 flag rows and the five counters of gs_refine_flags against the reference, bit for bit (None: not given).
    The message names the first row that differs, the decision, and what the decision saw."""
    if flags is not None:
        gf = np.asarray(flags).reshape(3, -1)
        assert gf.shape == ref["flags"].shape, f"flag rows {gf.shape}, reference {ref['flags'].shape}"
        for r in range(3):
            bad = np.nonzero(gf[r] != ref["flags"][r])[0]
            assert bad.size == 0, (f"row {bad[0]}: decision '{FLAG_NAMES[r]}' is {int(gf[r][bad[0]])}, the reference decides "
                                   f"{int(ref['flags'][r][bad[0]])} ({_row_facts(ref, bad[0])}); {bad.size} rows differ")
    if counters is not None:
        for k, (g, r) in enumerate(zip(counters, ref["counters"])):
            assert int(g) == r, f"counter '{COUNTER_NAMES[k]}': {int(g)}, reference {r}"


def compare_refine(got, ref, tol=None):
    """The one checker.  `got`: {"params", "exp_avg", "exp_avg_sq": dicts of float32 arrays; "tb_info"; optionally "flags"
    [3, N] and "counters" [5], where the implementation has them}.  Everything must equal `ref` bit for bit, except the
    children's means and log-scales, which must keep the bounds of the module docstring with `tol` = {"C_LS", "C_MU"}.
    Raises AssertionError naming the first row that differs; returns the worst error ratios {"log_scales", "means"} in units of
    eps32 x scale (so <= C_LS, C_MU)."""
    tol = {"C_LS": C_LS, "C_MU": C_MU} if tol is None else tol
    n_new, kinds = ref["n_new"], ("survivor", "split child", "clone")
    compare_decisions(got.get("flags"), got.get("counters"), ref)
    for key, val in ref["tb_info"].items():
        assert got["tb_info"].get(key) == val, f"tb_info[{key!r}]: {got['tb_info'].get(key)}, reference {val}"
    for name in PARAM_NAMES:
        for what in ("params", "exp_avg", "exp_avg_sq"):
            g, r = np.asarray(got[what][name]), ref[what][name]
            assert g.dtype == np.float32 and g.shape == r.shape, f"{what}[{name}]: {g.dtype} {g.shape}, reference {r.shape} (n_new {n_new})"
    ratios = {"log_scales": 0.0, "means": 0.0}
    child = np.zeros(n_new, dtype=bool)
    child[ref["child_rows"]] = True
    for name in PARAM_NAMES:
        for what in ("exp_avg", "exp_avg_sq", "params"):
            g, r = np.asarray(got[what][name]), ref[what][name]
            rows = np.arange(n_new)
            if what == "params" and name in ("means", "log_scales"):
                rows = np.nonzero(~child)[0]
            bad = _bits_differ(g[rows], r[rows])
            if bad.size:
                i = rows[bad[0]]
                raise AssertionError(f"{what}[{name}] row {i} ({kinds[ref['kind'][i]]} of old row {ref['src'][i]}): "
                                     f"{g[i].ravel()[:4]} is not the reference's {r[i].ravel()[:4]}; {bad.size} rows differ")
    cr = ref["child_rows"]
    if cr.size:
        with np.errstate(invalid="ignore"):
            d = np.abs(np.asarray(got["params"]["log_scales"], dtype=np.float64)[cr] - ref["child_log_scales"])
            q = d / (EPS32 * np.maximum(1.0, np.abs(ref["child_log_scales"])))
            q = np.where(np.isnan(q), np.inf, q)
            d = np.abs(np.asarray(got["params"]["means"], dtype=np.float64)[cr] - ref["child_means"])
            u = np.where(d == 0, 0.0, d / (EPS32 * ref["child_mean_scale"]))
            u = np.where(np.isnan(u), np.inf, u)
        ratios = {"log_scales": float(q.max()), "means": float(u.max())}
        i = np.unravel_index(q.argmax(), q.shape)[0]
        assert ratios["log_scales"] <= tol["C_LS"], (f"log_scales row {cr[i]} (split child of old row {ref['src'][cr[i]]}): off by "
                                                     f"{ratios['log_scales']:.2f} eps32 max(1, |ref|), bound {tol['C_LS']}")
        i = np.unravel_index(u.argmax(), u.shape)[0]
        assert ratios["means"] <= tol["C_MU"], (f"means row {cr[i]} (split child of old row {ref['src'][cr[i]]}): off by "
                                                f"{ratios['means']:.2f} eps32 (|mu| + |R| s |noise|), bound {tol['C_MU']}")
    return ratios


# ---- reset_opacities -------------------------------------------------------------------------------------------------------
def reset_opacities_ref(logit_opacities, min_opacity):
    """logit(min(sigmoid(x) / 2, 2 min_opacity)) in fp64 (the cap as the float32 tensor the reference fills with it)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.minimum(_sigmoid(logit_opacities) * 0.5, 2.0 * _f32(min_opacity))
        return np.log(t / (1.0 - t))


def reset_opacities_error(got, ref):
    """Worst |got - ref| / (eps32 max(1, |ref|)); where the reference is not finite the value must be the same."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if not same[~fin].all():
        return np.inf
    q = np.abs(got[fin] - ref[fin]) / (EPS32 * np.maximum(1.0, np.abs(ref[fin])))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


# ---- the same formulas in np.float32: what the constants are measured with -----------------------------------------------------
def children_f32(params, noise, src, copy, num_splits):
    """Means and log-scales of the split children (old row `src`, copy `copy`) with one float32 rounding per operation."""
    f = np.float32
    q = params["quats"][src].astype(f)
    q = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True, dtype=f)), f(1e-12))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f(1), f(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1).reshape(-1, 3, 3)
    s = np.exp(params["log_scales"][src].astype(f))
    sn = s * np.asarray(noise, dtype=f)[copy, src]
    off = (R[:, :, 0] * sn[:, None, 0] + R[:, :, 1] * sn[:, None, 1]) + R[:, :, 2] * sn[:, None, 2]
    means = params["means"][src].astype(f) + off
    log_scales = np.log(s / f(0.8 * num_splits))
    assert means.dtype == f and log_scales.dtype == f
    return means, log_scales


def reset_opacities_f32(logit_opacities, min_opacity):
    f = np.float32
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        sig = f(1) / (f(1) + np.exp(-np.asarray(logit_opacities, dtype=f)))
        t = np.minimum(sig * f(0.5), f(2.0 * min_opacity))
        out = np.log(t / (f(1) - t))
    assert out.dtype == f
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
N_SPECIAL = 16


def _special_rows(inp, thresholds, num_splits):
    """The constructed rows, written over the last N_SPECIAL rows: exact ties at the non-transcendental comparisons and the
    non-finite rows.  Each starts from a plain row -- scale 0.3 x the smaller scale threshold, opacity 0.5, never densified,
    no radius -- and changes what its line says."""
    f = np.float32
    n = len(inp["counts"])
    th = {k: f(v) for k, v in thresholds.items()}
    lo = 0.3 * min(float(th["densify_scale"]), float(th["prune_scale"]))
    hi = 5.0 * max(float(th["densify_scale"]), float(th["prune_scale"]))   # above both scale thresholds, children included
    tg, tr = th["densify_grad"], th["prune_radii"]
    nan, inf = f(np.nan), f(np.inf)
    b = n - N_SPECIAL
    P = inp["params"]
    P["log_scales"][b:] = f(np.log(lo))
    P["logit_opacities"][b:] = 0
    inp["grad_norm_accum"][b:] = 0
    inp["counts"][b:] = 1
    inp["max_radii"][b:] = 0
    rows = iter(range(b, n))
    inp["max_radii"][next(rows)] = tr                                       # == threshold: not pruned
    inp["max_radii"][next(rows)] = np.nextafter(tr, inf)                    # one ulp above: pruned
    inp["grad_norm_accum"][next(rows)] = tg                                 # avg == threshold (1 + 1e-8 == 1 in fp32): cloned
    inp["grad_norm_accum"][next(rows)] = np.nextafter(tg, f(0))             # one ulp below: not densified
    i = next(rows); inp["grad_norm_accum"][i] = tg; P["log_scales"][i] = f(np.log(2.0 * float(th["densify_scale"])))   # tie, split
    i = next(rows); inp["grad_norm_accum"][i] = tg * f(3); inp["counts"][i] = 3; inp["max_radii"][i] = tr               # 3t / 3 >= t
    i = next(rows); inp["grad_norm_accum"][i] = f(2e-8) * tg; inp["counts"][i] = 0     # never counted: accum / 1e-8 -> high
    i = next(rows); inp["grad_norm_accum"][i] = nan                                    # NaN average -> 0
    # one NaN log-scale, two finite ones above every scale threshold, high gradient: amax says clone and keep both
    i = next(rows); inp["grad_norm_accum"][i] = tg * f(4); P["log_scales"][i] = [nan, f(np.log(hi)), f(np.log(hi))]
    # ... low gradient: not pruned by scale
    i = next(rows); P["log_scales"][i] = [f(np.log(hi)), nan, f(np.log(lo))]
    # ... small finite ones, high gradient: cloned on every reading
    i = next(rows); inp["grad_norm_accum"][i] = tg * f(4); P["log_scales"][i, 2] = nan
    i = next(rows); P["logit_opacities"][i] = -inf; inp["grad_norm_accum"][i] = tg * f(4)   # low opacity, and so is its clone
    i = next(rows); P["logit_opacities"][i] = nan                                           # not low opacity
    i = next(rows); P["logit_opacities"][i] = inf                                           # opacity 1
    i = next(rows); P["log_scales"][i] = -inf                                               # scale 0
    i = next(rows); inp["grad_norm_accum"][i] = tg * f(4); P["log_scales"][i] = f(np.log(hi))   # plain split whose children go by scale
    return np.arange(b, n)


def move_off_thresholds(inp, thresholds, num_splits):
    """Moves (never drops) every row that lies within MARGIN of a transcendental threshold: its log-scales or its logit go up
    by 5 MARGIN.  Returns how many rows were moved."""
    moved = 0
    for _ in range(8):
        m = margins(inp["params"]["log_scales"], inp["params"]["logit_opacities"], thresholds, num_splits)
        near_s = (m["densify_scale"] < 2 * MARGIN) | (m["prune_scale"] < 2 * MARGIN) | (m["child_prune_scale"] < 2 * MARGIN)
        near_o = m["min_opacity"] < 2 * MARGIN
        if not (near_s.any() or near_o.any()):
            break
        moved += int(near_s.sum() + near_o.sum())
        inp["params"]["log_scales"][near_s] += np.float32(5 * MARGIN)
        inp["params"]["logit_opacities"][near_o] += np.float32(5 * MARGIN)
    return moved


def make_inputs(n, K, seed, thresholds=None, num_splits=2, special=True, grad_span=3.0):
    """Everything one refinement reads, as float32 arrays: log-scales in [-9, 1] (the largest of a row uniform there; a tenth of
    the rows within 2 % of a scale threshold or of a threshold x 0.8 S), logits in [-12, 12] (a twentieth within 2 % of the
    opacity threshold), 10 % of the rows never seen, average gradients uniform in [0, grad_span] x their threshold, radii on both
    sides of theirs, random moments with exp_avg_sq > 0, noise [S, n, 3].  With `special` and n >= 2 N_SPECIAL the last
    N_SPECIAL rows are the ties and the non-finite rows of `_special_rows`.  Rows closer than MARGIN to a transcendental
    threshold are moved off it."""
    th = dict(DEFAULT_THRESHOLDS if thresholds is None else thresholds)
    S, f = int(num_splits), np.float32
    r = np.random.default_rng(seed)
    top = r.uniform(-9.0, 1.0, n)
    ls = np.maximum(top[:, None] - r.uniform(0.0, 3.0, (n, 3)), -9.0)
    ls[np.arange(n), r.integers(0, 3, n)] = top
    razor = [v for v in (th["densify_scale"], th["prune_scale"], th["prune_scale"] * 0.8 * S, th["densify_scale"] * 0.8 * S)
             if np.exp(-9.0) < v < np.exp(1.0)]           # (a threshold switched off -- 0, 1e9 -- has no neighbourhood to visit)
    near, pick, jitter = r.random(n) < 0.10, r.integers(0, 4, n), 1.0 + r.uniform(-0.02, 0.02, n)
    if razor:
        shift = np.log(np.array(razor)[pick % len(razor)] * jitter) - top
        ls[near] += shift[near, None]
    logit = r.uniform(-12.0, 12.0, n)
    near, jitter = r.random(n) < 0.05, 1.0 + r.uniform(-0.02, 0.02, n)
    if 0.0 < th["min_opacity"] < 0.5:
        t = th["min_opacity"] * jitter
        logit[near] = np.log(t / (1.0 - t))[near]
    counts = np.where(r.random(n) < 0.10, 0.0, r.integers(1, 6, n)).astype(f)
    # (a threshold switched off -- 0, 1e9 -- does not set the size of the data: gradients and radii keep their usual range)
    g0 = th["densify_grad"] if 0.0 < th["densify_grad"] < 1.0 else DEFAULT_THRESHOLDS["densify_grad"]
    r0 = th["prune_radii"] if 0.0 < th["prune_radii"] < 1.0 else DEFAULT_THRESHOLDS["prune_radii"]
    accum = (r.uniform(0.0, grad_span, n) * g0).astype(f) * counts
    params = {"means": r.standard_normal((n, 3), dtype=f), "log_scales": ls.astype(f), "quats": r.standard_normal((n, 4), dtype=f),
              "sh_0": r.standard_normal((n, 1, 3), dtype=f), "sh_rest": r.standard_normal((n, K - 1, 3), dtype=f) * f(0.1),
              "logit_opacities": logit.astype(f)}
    m = {k: r.standard_normal(v.shape, dtype=f) * f(1e-3) for k, v in params.items()}
    v = {k: r.random(p.shape, dtype=f) * f(1e-6) + f(1e-12) for k, p in params.items()}
    inp = {"params": params, "exp_avg": m, "exp_avg_sq": v, "grad_norm_accum": accum, "counts": counts,
           "max_radii": (r.uniform(0.0, 2.0, n) * r0).astype(f), "noise": r.standard_normal((S, n, 3), dtype=f),
           "thresholds": th, "num_splits": S, "K": K, "special_rows": np.zeros(0, dtype=np.int64)}
    if special and n >= 2 * N_SPECIAL:
        inp["special_rows"] = _special_rows(inp, th, S)
    inp["moved"] = move_off_thresholds(inp, th, S)
    return inp


def refine_ref_of(inp):
    return refine_ref(inp["params"], inp["exp_avg"], inp["exp_avg_sq"], inp["grad_norm_accum"], inp["counts"], inp["max_radii"],
                      inp["noise"], inp["thresholds"], inp["num_splits"])


def assert_margins(inp, ref):
    """No decision of this input hangs on the last bits of exp / sigmoid -- with every row in, none excluded."""
    for name, d in ref["margins"].items():
        assert d.shape == inp["counts"].shape and float(d.min(initial=np.inf)) >= MARGIN, (name, float(d.min(initial=np.inf)))
