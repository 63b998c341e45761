"""fp64 reference of the fused Adam kernels (`adam1()` in csrc/gs_common.h) and the bounds a correct fp32 kernel keeps.

Which Adam
----------
The C ABI takes `beta1`, `beta2`, `eps`, `grad_scale` and the learning rates as `float`.  The kernel forms `1.f - beta` in fp32,
which is EXACT for beta in [0.5, 1] (Sterbenz), and the host forms the bias corrections from `(double)beta`.  So the kernels are a
self-consistent Adam at the fp32 values the ABI receives -- beta2' = fl32(0.999) = 0.99900001287 -- and that is the reference
here: `adam_ref` promotes every hyper-parameter from `np.float32`, exactly as `adam_launch` does, and then works in float64:

    g' = grad_scale * g
    m' = b1 m + (1 - b1) g'
    v' = b2 v + (1 - b2) g'^2
    denom = sqrt(v') / sqrt(1 - b2^t) + eps
    p' = p - lr / (1 - b1^t) * m' / denom

torch.optim.Adam mixes three roundings of beta2 (fl32(0.999) for the decay, fl32(0.001) for the increment, the double 0.999
for the bias correction); its `exp_avg_sq` therefore lies at a relative 1.29e-5 from this reference
(tests/test_adam_ref_host.py derives the number).  That is a property of the float ABI, not of the arithmetic.

The bounds (eps32 = 2^-24, the unit round-off of fp32)
------------------------------------------------------
`adam1()` is, per element:   m = fma(b1, m, (1-b1)*g);  v = fma(b2, v, ((1-b2)*g)*g);  denom = fma(sqrt(v), isbc2, eps);
p = fma(-ss, m/denom, p)  with  g = grad_scale * g_in,  isbc2 = fl32(1/sqrt(1-b2^t)),  ss = fl32(lr/(1-b1^t)).
Counting one relative error of at most eps32 per rounding (1-b is exact and counts nothing):

  m:  the product (1-b1)*g', the rounding of g' = grad_scale*g itself and the fma's final rounding.  The first two scale with
      |(1-b1) g'|, the last with |m'| <= A := |b1 m| + |(1-b1) g'|:  error <= 3 eps32 A.  The CPU emulation measured 1.9.
      Bound: 4 eps32 A.
  v:  two products and twice the rounding of g' on the increment, the fma's rounding on the sum; all terms are positive, so
      everything scales with v':  error <= 5 eps32 v'.  Measured 2.9.  Bound: 6 eps32 v_ref.
  p:  the final rounding is eps32 |p'| <= eps32 max(|p|, |p_ref|) (half an ulp: reached just above a power of two, so the
      observed ratio of p comes close to 1 wherever the update is small against p -- that is the format, not the kernel).
      The update ss * m'/denom carries: ss (1), isbc2 (1), the square root (1, plus half of v's 5 = 2.5), the fma that forms
      denom (1), the division (1) -- 7.5 eps32 relative to the update, which is at most U := ss A / denom -- plus m's own
      3 eps32 A pushed through ss / denom = 3 eps32 U (this term does NOT shrink when b1 m and (1-b1) g' cancel, which is why
      the bound is written in U and not in the update).  The rounding of g' is ONE error that enters m' and sqrt(v') with the
      same sign and cancels in their quotient, so of its 1 + 1 only 1 can count: 9.5 in all.  The emulation measured 4.9.
      Bound: eps32 max(|p|, |p_ref|) + 10 eps32 U.

These are conditions, not measurements: a square root or a division that is not correctly rounded, a bias correction formed in
fp32, an increment constant taken from another rounding of beta2 all show as a ratio above 1.

fp32 range
----------
A relative bound means nothing where fp32 itself has no relative precision.  An element is FLAGGED when one of the positive
quantities that pass through a register on the way to v' -- b2 v, (1-b2) g'^2, v' -- is non-zero and below `TINY`, or when a
reference result exceeds the largest fp32 number.  Flagged elements get, on top of the relative bound, the absolute floor
`V_FLOOR` = 2^-125 on v: two quantities (the incoming b2 v and the increment) may each be flushed or lose their low bits below
the smallest normal number 2^-126.  p and m need no floor: denom >= eps dwarfs sqrt(2^-125), and m is linear in g.  An exact zero
is exact and is not flagged.  Where the reference overflows, the device value may also be +-inf.
`TINY` is 1e-36, a hundred times the smallest normal fp32 number (1.18e-38): below 2^-126 lies the only range in which fp32
products lose relative precision, and the margin covers the rounded intermediates.  (A threshold of 1e-30 would flag 8 % of
gradients drawn log-uniformly from [1e-16, 1e16] -- (1-b2) g^2 < 1e-30 for |g| < 3.2e-14 -- and give every one of them a
weaker check for no reason in the number format; with 1e-36 the flagged share of that distribution stays below the 1 % the
tests assert.)
"""
import numpy as np

EPS32 = 2.0 ** -24
TINY = 1e-36
V_FLOOR = 2.0 ** -125
FLT_MAX = float(np.finfo(np.float32).max)
C_M, C_V, C_P = 4.0, 6.0, 10.0   # the constants of the three bounds, in units of eps32


def _f32(x) -> float:
    """The double the C ABI sees for a `float` argument."""
    return float(np.float32(x))


def adam_ref(p, g, m, v, lr, t, beta1, beta2, eps, grad_scale=1.0, promote=True):
    """One Adam step in float64 on fp32 inputs.  Returns (p_ref, m_ref, v_ref, scales); `scales` holds what `adam_bounds` needs:
    A = |b1 m| + |(1-b1) g'|, U = ss A / denom, and the three positive quantities the flag rule looks at.
    `promote=False` keeps the hyper-parameters as the doubles they were given (torch.optim.Adam in float64)."""
    cv = _f32 if promote else float
    b1, b2, e, gs, lr = cv(beta1), cv(beta2), cv(eps), cv(grad_scale), cv(lr)
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    t = int(t)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    g = gs * g
    with np.errstate(over="ignore", invalid="ignore"):
        m_ref = b1 * m + (1.0 - b1) * g
        inc = (1.0 - b2) * g * g
        v_ref = b2 * v + inc
        denom = np.sqrt(v_ref) / np.sqrt(bc2) + e
        ss = lr / bc1
        p_ref = p - ss * m_ref / denom
        A = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
        U = ss * A / denom
    return p_ref, m_ref, v_ref, {"A": A, "U": U, "decayed": b2 * v, "inc": inc}


def flagged(p_ref, m_ref, v_ref, scales):
    """The elements fp32 cannot hold to a relative bound (module docstring, "fp32 range")."""
    tiny = np.zeros(v_ref.shape, dtype=bool)
    for x in (v_ref, scales["inc"], scales["decayed"]):
        tiny |= (x > 0.0) & (x < TINY)
    over = (np.abs(p_ref) > FLT_MAX) | (np.abs(m_ref) > FLT_MAX) | (np.abs(v_ref) > FLT_MAX)
    return tiny, over


def adam_bounds(p, p_ref, m_ref, v_ref, scales):
    """Per-element tolerances (tol_p, tol_m, tol_v) and the flag mask."""
    p = np.asarray(p, dtype=np.float64)
    tiny, over = flagged(p_ref, m_ref, v_ref, scales)
    with np.errstate(over="ignore", invalid="ignore"):
        tol_m = C_M * EPS32 * scales["A"]
        tol_v = C_V * EPS32 * v_ref + np.where(tiny | over, V_FLOOR, 0.0)
        tol_p = EPS32 * np.maximum(np.abs(p), np.abs(p_ref)) + C_P * EPS32 * scales["U"]
    return tol_p, tol_m, tol_v, tiny | over


def error_ratios(new, old_p, ref, grad_ok=None):
    """new = (p, m, v) after the step, ref = adam_ref(...)'s tuple.  Returns {"p", "m", "v"}: the worst |error| / tolerance over
    the elements (0/0 counts as 0: an exact result against a zero tolerance), and "flagged": the share of flagged elements.
    Where the reference overflows fp32 an infinite device value of the right sign passes."""
    p_ref, m_ref, v_ref, scales = ref
    tol_p, tol_m, tol_v, flag = adam_bounds(old_p, p_ref, m_ref, v_ref, scales)
    out = {"flagged": float(flag.mean()) if flag.size else 0.0}
    for name, x, r, tol in (("p", new[0], p_ref, tol_p), ("m", new[1], m_ref, tol_m), ("v", new[2], v_ref, tol_v)):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            err = np.abs(x - r)
            ovf = np.abs(r) > FLT_MAX
            err = np.where(ovf & np.isinf(x) & (np.sign(x) == np.sign(r)), 0.0, err)
            ratio = np.where(err == 0.0, 0.0, err / tol)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)   # a NaN where the reference is finite is an error of any size
        out[name] = float(ratio.max()) if ratio.size else 0.0
    return out


# ---- an fp32 emulation of adam1() as the library's build compiles it (-ffp-contract=fast) ----------------------------------
def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 a, b, c: the product of two fp32 numbers is exact in float64; the sum is rounded to 53 bits and
    then to 24 (a double rounding that differs from a true fma in about one case in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam1_emulated(p, g, m, v, lr, t, beta1, beta2, eps, grad_scale=1.0, wrong=None):
    """adam1() with one fp32 rounding per operation, multiply-adds fused where the compiler fuses them, and the host side of
    `adam_launch` (bias corrections in double, `step_size` and `inv_sqrt_bc2` rounded to fp32).
    `wrong` names one deliberate mistake (tests/test_adam_ref_host.py: the bounds must reject each):
    "eps_in_sqrt", "no_bc2", "no_bc1", "beta1_for_v", "scale_after_square", "torch_constants"."""
    f = np.float32
    b1, b2, e, gs = f(beta1), f(beta2), f(eps), f(grad_scale)
    bc1 = 1.0 - float(b1) ** int(t)
    bc2 = 1.0 - float(b2) ** int(t)
    if wrong == "no_bc1":
        bc1 = 1.0
    if wrong == "no_bc2":
        bc2 = 1.0
    ss = f(float(f(lr)) / bc1)
    isbc2 = f(1.0 / np.sqrt(bc2))
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    full = lambda s: np.full(p.shape, s, dtype=f)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        gu = g          # the gradient as it came
        g = g * gs
        m = _fma32(full(b1), m, (f(1) - b1) * g)
        b2v = b1 if wrong == "beta1_for_v" else b2
        one_m = f(0.001) if wrong == "torch_constants" else f(1) - b2v
        inc = ((one_m * gu) * gu) * gs if wrong == "scale_after_square" else (one_m * g) * g
        v = _fma32(full(b2v), v, inc)
        if wrong == "eps_in_sqrt":
            denom = np.sqrt(v + e).astype(f) * isbc2
        else:
            denom = _fma32(np.sqrt(v).astype(f), full(isbc2), full(e))
        q = (m / denom).astype(f)
        p = _fma32(full(-ss), q, p)
    return p, m, v


# ---- the input regimes shared by the host and the GPU tests -------------------------------------------------------------
def regime_inputs(n, seed):
    """p, g, m, v [n] fp32: |g| log-uniform in [1e-16, 1e16] with random sign, exact zeros on 5 % of g and on 5 % of (m, v)
    jointly, moments at 10^+-3 relative to g (m = +-|g| 10^u, v = (|g| 10^w)^2 with u, w uniform in [-3, 3]), |p| log-uniform in
    [1e-3, 1e2] with random sign."""
    r = np.random.default_rng(seed)
    mag = 10.0 ** r.uniform(-16.0, 16.0, n)
    sign = lambda: np.where(r.random(n) < 0.5, -1.0, 1.0)
    g = sign() * mag
    m = sign() * mag * 10.0 ** r.uniform(-3.0, 3.0, n)
    v = (mag * 10.0 ** r.uniform(-3.0, 3.0, n)) ** 2
    p = sign() * 10.0 ** r.uniform(-3.0, 2.0, n)
    zg = r.random(n) < 0.05
    zm = r.random(n) < 0.05
    g[zg] = 0.0
    m[zm] = 0.0
    v[zm] = 0.0
    return tuple(x.astype(np.float32) for x in (p, g, m, v))
