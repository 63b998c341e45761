"""fp64 reference of the depth loss (csrc/gs_depth_loss.h) and the bounds a correct fp32 kernel keeps -- shared by
tests/test_depth_loss_host.py (the header built with the host compiler, the plain-torch path) and tests/test_gpu_depth_loss.py (the
device).

For a frame of P pixels, a prediction d, a target t and a mask m (all fp32; None = no mask):

    valid = t > 0 and t finite,   w = valid (1 - m),   e = d - t  ("depth")  or  disp(d) - 1 / t  ("disparity"), disp(d) = d > 0 ? 1 / d : 0
    value = sum(w |e|) / sum(w)  (0 when sum(w) == 0),   d value / d d = w sign(e) / sum(w) * {depth: 1; disparity: d > 0 ? -1 / d^2 : 0}

The reference evaluates this in fp64 on the fp32 inputs.  With eps32 = 2^-24, the unit round-off of fp32, the kernel's own roundings:

  w      fl(1 - m): one rounding, |error| <= eps32 w (exact for m in {0, 1}).
  e      depth: fl(d - t), one rounding: E_e = eps32 |e|.  Disparity: fl(1 / d), fl(1 / t) and the difference, three roundings:
         E_e = eps32 (disp(d) + 1 / t + |e|).
  value  the products w |e| are exact in fp64 and the sums are fp64, so the numerator errs by sum(w E_e + eps32 w |e|), the
         denominator by eps32 sum(w); the quotient is rounded to fp32 ONCE: one fp32 ulp of the value.  Plus 1e-12 (relative) for the
         fp64 accumulation and the second-order terms (a chain of n additions errs by at most n 2^-53: 2.3e-10 at 2 M pixels in
         pixel order, far less through the kernels' trees -- and exposure_ref's figure for the same scheme).
  grad   fl(1 / sum(w)) carries the denominator's eps32 and its own rounding; times the upstream gradient, times w (with w's own
         rounding): 5 eps32 |g| in depth mode; the two divisions by d of the disparity mode add 2: 7 eps32 |g|.  One of slack each: 6
         and 8.  Where |e| <= E_e the kernel's sign(e) may legitimately differ from the reference's: there the bound is 2 |g| (an
         exact e == 0 is computed exactly -- d and t equal, or 1 / d and 1 / t equal -- and gives 0 on both sides).
  join   v_acc = g / max(alpha, 1e-10): one more rounding; v_alpha = -(g ((acc / a) / a)) where alpha >= 1e-10, else 0: three more.
"""
import numpy as np

from exposure_ref import BIG_FRAME, FRAMES, worst_ratio  # noqa: F401  (the frames of the streaming image kernels)

EPS32 = 2.0 ** -24
HOST_FRAMES = FRAMES[:3]
MODES = ("depth", "disparity")
ED_FLOOR = np.float32(1e-10)


def make_case(rng, H, W, mask=True, d=None):
    """(d, t, m): a depth-like prediction in [0.5, 8] with a few zeros and negatives (or the map `d` as it is), a target near it with
    holes -- zeros, negatives, NaN, +-inf --, pixels where t == d exactly, and a soft mask in [0, 1] with hard 0 / 1 regions (or
    None).  fp32 [H, W]."""
    given = d is not None
    d = np.array(d, dtype=np.float32) if given else rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    t = (np.where(d > 0, d, 2.0) * (1.0 + 0.1 * rng.standard_normal((H, W)))).astype(np.float32)
    u = rng.random((H, W))
    t[u < 0.10] = 0.0
    t[(u >= 0.10) & (u < 0.13)] = -1.5
    t[(u >= 0.13) & (u < 0.15)] = np.nan
    t[(u >= 0.15) & (u < 0.16)] = np.inf
    t[(u >= 0.16) & (u < 0.17)] = -np.inf
    same = (u >= 0.17) & (u < 0.22)
    t[same] = d[same]
    u2 = rng.random((H, W))
    if not given:
        d[u2 < 0.03] = 0.0
        d[(u2 >= 0.03) & (u2 < 0.05)] = -0.25
    m = None
    if mask:
        m = rng.random((H, W)).astype(np.float32)
        u3 = rng.random((H, W))
        m[u3 < 0.3] = 0.0
        m[u3 > 0.8] = 1.0
    return d, t, m


def blend_like(rng, H, W):
    """(colors4 [H,W,4], alphas [H,W]) as a 4-channel blend leaves them: colours in [-0.1, 1.1], alpha in [0, 1] with exact zeros
    (nothing hit) and values under the expected depth's floor, the accumulated depth = alpha times a depth in [0.5, 8]."""
    alpha = rng.random((H, W)).astype(np.float32)
    u = rng.random((H, W))
    alpha[u < 0.05] = 0.0
    alpha[(u >= 0.05) & (u < 0.07)] = 3e-11
    z = rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    c = rng.uniform(-0.1, 1.1, (H, W, 4)).astype(np.float32)
    c[..., 3] = alpha * z
    return c, alpha


def expected_depth32(acc, alpha):
    """acc / max(alpha, 1e-10) in fp32: an IEEE division, the same bits on every side."""
    return (acc.astype(np.float32) / np.maximum(alpha.astype(np.float32), ED_FLOOR)).astype(np.float32)


def _terms(d, t, m, mode):
    d64, t64 = np.asarray(d, dtype=np.float64), np.asarray(t, dtype=np.float64)
    valid = np.isfinite(t64) & (t64 > 0)
    w = valid.astype(np.float64) * (1.0 if m is None else 1.0 - np.asarray(m, dtype=np.float64))
    ts = np.where(valid, t64, 1.0)
    pos = d64 > 0
    ds = np.where(pos, d64, 1.0)
    if mode == "depth":
        e, fac = d64 - ts, np.ones_like(d64)
        E_e = EPS32 * np.abs(e)
    else:
        disp = np.where(pos, 1.0 / ds, 0.0)
        e = disp - 1.0 / ts
        E_e = EPS32 * (disp + 1.0 / ts + np.abs(e))
        fac = np.where(pos, -1.0 / (ds * ds), 0.0)
    e, E_e = np.where(w > 0, e, 0.0), np.where(w > 0, E_e, 0.0)
    return w, e, E_e, fac


def value64(d, t, m, mode):
    """(value, bound) in fp64."""
    w, e, E_e, _ = _terms(d, t, m, mode)
    den = w.sum()
    if den == 0.0:
        return 0.0, 0.0
    num = (w * np.abs(e)).sum()
    value = num / den
    num_err, den_err = (w * (E_e + EPS32 * np.abs(e))).sum(), EPS32 * den
    bound = (num_err + value * den_err) / den + float(np.spacing(np.float32(value))) + 1e-12 * value
    return float(value), float(bound)


def grad64(d, t, m, mode, upstream=1.0):
    """(upstream * d value / d d, bound): fp64 [H, W] each."""
    w, e, E_e, fac = _terms(d, t, m, mode)
    den = w.sum()
    if den == 0.0:
        return np.zeros_like(w), np.zeros_like(w)
    g = float(upstream) * w * np.sign(e) / den * fac
    mag = np.abs(float(upstream)) * w / den * np.abs(fac)
    k = 6.0 if mode == "depth" else 8.0
    razor = (np.abs(e) <= E_e) & (e != 0.0)
    return g, np.where(razor, 2.0 * mag, k * EPS32 * mag)


def join64(acc, alpha, d, t, m, mode, lam):
    """(v_acc, v_alpha, bound_acc, bound_alpha): the depth term's gradient lam * value through d = acc / max(alpha, 1e-10)."""
    g, gb = grad64(d, t, m, mode, lam)
    acc64, al64 = np.asarray(acc, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    a = np.maximum(al64, float(ED_FLOOR))
    v_acc = g / a
    passes = np.asarray(alpha, dtype=np.float32) >= ED_FLOOR
    v_alpha = np.where(passes, -g * acc64 / (a * a), 0.0)
    b_acc = gb / a + 2.0 * EPS32 * np.abs(v_acc)
    b_alpha = np.where(passes, gb * np.abs(acc64) / (a * a) + 4.0 * EPS32 * np.abs(v_alpha), 0.0)
    return v_acc, v_alpha, b_acc, b_alpha
