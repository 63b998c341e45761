"""An independent statement of the MCMC densification (easy_gaussian_splatting_amd/mcmc.py, csrc/gs_mcmc.hip) in numpy float64
and Python integers: no torch kernels, no native calls.  Shared by tests/test_mcmc_host.py and tests/test_gpu_mcmc.py.

Integer stages (weights given, CDF, draws, counts) have one right answer and are compared exactly.  Floating-point stages are
evaluated here in float64 from the float32 inputs and rounded once to float32; the device does the same, so the two differ by
the last bit of libm's exp / log / pow at the most."""
import math

import numpy as np

MAX_RATIO = 51
O_MAX = 1.0 - 2.0 ** -23
WIDTHS = lambda K: [3, 3, 4, 3, 3 * (K - 1), 1]   # means, log_scales, quats, sh_0, sh_rest, logit_opacities


def sigmoid(l):
    return 1.0 / (1.0 + np.exp(-np.asarray(l, dtype=np.float64)))


def weights(logits, min_opacity, grow=False):
    """(w uint64-valued int64 array, dead bool array, o float64)"""
    o = sigmoid(logits)
    dead = np.zeros(o.shape, dtype=bool) if grow else (o <= min_opacity)
    w = np.where(dead, 0, np.maximum(1, np.floor(o * 2.0 ** 24))).astype(np.int64)
    return w, dead, o


def cdf(w):
    """Inclusive prefix sum with Python integers."""
    out, run = [], 0
    for x in np.asarray(w).tolist():
        run += int(x)
        out.append(run)
    return out


def mulhi64(b, total):
    return ((int(b) & (2 ** 64 - 1)) * int(total)) >> 64


def upper_bound(c, t):
    """min{i : c[i] > t} for a non-decreasing list c with c[-1] > t"""
    lo, hi = 0, len(c) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if c[mid] > t:
            hi = mid
        else:
            lo = mid + 1
    return lo


def draws(w, bits, n_draws):
    """(src list, counts array): draw j of the first n_draws words of `bits` (int64 read as uint64); none if sum(w) == 0"""
    c = cdf(w)
    total = c[-1] if c else 0
    counts = np.zeros(len(c), dtype=np.int64)
    src = []
    if total == 0:
        return src, counts
    for b in np.asarray(bits).tolist()[:n_draws]:
        i = upper_bound(c, mulhi64(b, total))
        src.append(i)
        counts[i] += 1
    return src, counts


def relocation_values(o, s, ratio):
    """(o', s') in float64 for one Gaussian: o scalar, s [3]; R = clamp(ratio, 1, 51);
    D = sum_{i=1..R} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1), the double sum as it is written.
    o' = 1 - (1 - o)^(1/R) through log1p / expm1 (the same number; the power loses o' to cancellation for small o)."""
    R = min(max(int(ratio), 1), MAX_RATIO)
    o = float(o)
    on = -math.expm1(math.log1p(-o) / R) if o < 1.0 else 1.0
    D = 0.0
    for i in range(1, R + 1):
        for k in range(i):
            D += math.comb(i - 1, k) * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1)
    return on, np.asarray(s, dtype=np.float64) * (o / D)


def relocation_values_plain(o, s, ratio):
    """The same with o' = 1 - (1 - o)^(1/R) as written (for the host tests of this file)."""
    R = min(max(int(ratio), 1), MAX_RATIO)
    on = 1.0 - (1.0 - float(o)) ** (1.0 / R)
    D = sum(math.comb(i - 1, k) * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1) for i in range(1, R + 1) for k in range(i))
    return on, np.asarray(s, dtype=np.float64) * (float(o) / D)


def split_flat(flat, n_rows, K, offsets):
    """views of the six tensors [n_rows, width] of a flat buffer"""
    return [flat[o:o + n_rows * w].reshape(n_rows, w) for o, w in zip(offsets, WIDTHS(K))]


def apply(params, exp_avg, exp_avg_sq, n, n_rows, K, offsets, src, dst, counts, min_opacity):
    """New (params, exp_avg, exp_avg_sq) flat float32 arrays: values of the drawn Gaussians first, then the copies src -> dst,
    moments of every rewritten row zero.  Also returns the set of rewritten rows."""
    p, m, v = (np.array(x, dtype=np.float32, copy=True) for x in (params, exp_avg, exp_avg_sq))
    P, M, V = (split_flat(x, n_rows, K, offsets) for x in (p, m, v))
    touched = set()
    for i in np.nonzero(np.asarray(counts)[:n] > 0)[0].tolist():
        o = float(sigmoid(P[5][i, 0]))
        s = np.exp(P[1][i].astype(np.float64))
        on, sn = relocation_values(o, s, int(counts[i]) + 1)
        on = min(max(on, min_opacity), O_MAX)
        P[5][i, 0] = np.float32(math.log(on / (1.0 - on)))
        P[1][i] = np.log(sn).astype(np.float32)
        touched.add(i)
    for s_, d_ in zip(src, dst):
        for t in range(6):
            P[t][d_] = P[t][s_]
        touched.add(int(d_))
    for i in touched:
        for t in range(6):
            M[t][i] = 0.0
            V[t][i] = 0.0
    return p, m, v, touched


def rotmat(q):
    """[n, 4] wxyz (normalised here) -> [n, 3, 3]"""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.maximum(np.sqrt((q * q).sum(axis=1, keepdims=True)), 1e-12)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def noise(means, log_scales, quats, logits, z, strength):
    """means + strength g(o) R diag(s^2) R^T z in float64, [n, 3]"""
    means, z = np.asarray(means, dtype=np.float64), np.asarray(z, dtype=np.float64)
    s2 = np.exp(np.asarray(log_scales, dtype=np.float64)) ** 2
    o = sigmoid(logits)
    gate = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))
    R = rotmat(quats)
    y = s2 * np.einsum("nji,nj->ni", R, z)               # diag(s^2) R^T z
    return means + (strength * gate)[:, None] * np.einsum("nij,nj->ni", R, y)


def ulp_distance(a, b):
    """float32 arrays -> distance in units in the last place (ordered-integer distance)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
