"""Reference of the captured budget step's device arithmetic, in Python integers and numpy float64 (no kernel, no torch):

* `philox4x32_10`  one Philox4x32-10 block (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", 2011);
* `counter_key`    how Gaussian n, optimizer step t and the 64-bit seed are packed into the counter and the key;
* `normals`        the three float32 standard normals of every Gaussian (Box-Muller in fp64, one rounding);
* `budget_reg`     value and gradients of a mean(sigmoid(logit)) + b mean(exp(log_scale)).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(x) & MASK for x in counter)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def counter_key(n, t, seed):
    n, t, seed = int(n), int(t), int(seed) & 0xFFFFFFFFFFFFFFFF
    return (n & MASK, n >> 32, t & MASK, t >> 32), (seed & MASK, seed >> 32)


def words(n_first, count, t, seed):
    """uint32 [count, 4]: the Philox block of Gaussians n_first .. n_first + count - 1 at step t."""
    out = np.empty((count, 4), dtype=np.uint32)
    for i in range(count):
        out[i] = philox4x32_10(*counter_key(n_first + i, t, seed))
    return out


def normals_of_words(x):
    """float32 [count, 3] from uint32 [count, 4]: u = (x + 0.5) 2^-32, Box-Muller in fp64, each z rounded to float32 once."""
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    r01, r23 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a01, a23 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r01 * np.cos(a01), r01 * np.sin(a01), r23 * np.cos(a23)], 1)
    return z.astype(np.float32)


def normals(count, t, seed, n_first=0):
    return normals_of_words(words(n_first, count, t, seed))


def budget_reg(logits, log_scales, a, b):
    """(value, d/d logit [N], d/d log_scale [N, 3]) in fp64; the upstream factors are the float32 values the kernels use."""
    l, ls = np.asarray(logits, np.float64), np.asarray(log_scales, np.float64)
    N = l.shape[0]
    o, s = 1.0 / (1.0 + np.exp(-l)), np.exp(ls)
    ga, gb = np.float64(np.float32(a / N)), np.float64(np.float32(b / (3 * N)))
    return a * o.mean() + b * s.mean(), ga * o * (1.0 - o), gb * s
