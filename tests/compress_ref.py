"""numpy float64 restatements for the compact-file tests (tests/test_compress_host.py, tests/test_gpu_compress.py): the quantiser's
formula, the error in the quantised domain, and a way to undo the file's order that does not ask the code under test."""
import numpy as np


def T(v, log):
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.log1p(np.abs(v)) if log else v


def steps(lo, hi, bits, log):
    """[C] the step of every channel in the quantised domain"""
    return (T(hi, log) - T(lo, log)) / (2 ** bits - 1)


def quant_formula(v, lo, hi, bits, log):
    """q = clamp(rint((T(v) - T(lo)) / (T(hi) - T(lo)) (2^b - 1)), 0, 2^b - 1); hi == lo gives 0"""
    levels = 2 ** bits - 1
    span = T(hi, log) - T(lo, log)
    x = np.where(span > 0, (T(v, log) - T(lo, log)[None, :]) / np.where(span > 0, span, 1.0)[None, :] * levels, 0.0)
    return np.clip(np.rint(x), 0, levels).astype(np.int64)


def domain_error(want, got, lo, hi, bits, log):
    """(|T(want) - T(got)| [N, C], step [C])"""
    return np.abs(T(want, log) - T(got, log)), steps(lo, hi, bits, log)


def float32_store_fits(v, step, log):
    """Does the rounding of a dequantised value to float32, at most 2^-24 |v| (2^-24 |v| / (1 + |v|) in the log domain), lie
    inside the 2^-11 step of slack the bound leaves, in every channel?  (channels of zero step round-trip exactly)"""
    a = np.abs(np.asarray(v, np.float64))
    cost = 2.0 ** -24 * (a / (1.0 + a) if log else a)
    return bool(((cost <= 2.0 ** -11 * step[None, :]) | (step[None, :] == 0)).all())


def canonical(model, name):
    """[N, C] float64: what the file quantises -- the stored parameter; the float32 nearest the unit quaternion, with w >= 0"""
    v = getattr(model, name).detach().cpu().numpy().astype(np.float64)
    v = v.reshape(v.shape[0], -1)
    if name == "quats":
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        v = np.where(v[:, :1] < 0, -v, v)
    return v


def match_rows(original, loaded):
    """perm [N]: loaded[i] is original[perm[i]] -- each loaded mean's nearest original, which must be a permutation (the means of
    the test models are much further apart than a quantisation step)."""
    o, l = np.asarray(original, np.float64), np.asarray(loaded, np.float64)
    d = (l * l).sum(1)[:, None] - 2.0 * (l @ o.T) + (o * o).sum(1)[None, :]
    perm = d.argmin(1)
    assert np.array_equal(np.sort(perm), np.arange(len(o))), "the loaded means do not match the originals one to one"
    return perm
