"""References for the k-means tests (tests/test_kmeans_host.py, tests/test_gpu_kmeans.py), none of them the code under test:

  * `lloyd_step`: one Lloyd step in float64 numpy -- assign (smallest index among the nearest), mean, an empty cluster kept;
  * `margin`: how far the chosen centroid is from the nearest one in float64, next to the bound a float32 chain may cost;
  * `int_labels`: the brute-force argmin on small-integer data in int64, the lowest index on ties (every operation exact);
  * `host_lib`: tests/hostmath/kmeans.cpp -- csrc/gs_kmeans.h, the device's own text -- built with the host compiler;
  * the data of the cases both files share.
"""
import ctypes as ct
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24   # the unit roundoff of float32


def host_lib(directory):
    so = os.path.join(str(directory), "libkmeans_host.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "kmeans.cpp")], check=True)
    L = ct.CDLL(so)
    L.km_assign.argtypes, L.km_assign.restype = [ct.c_int64, ct.c_int64, ct.c_int] + [ct.c_void_p] * 4, None
    L.km_update.argtypes, L.km_update.restype = [ct.c_int64, ct.c_int64, ct.c_int] + [ct.c_void_p] * 4, None
    return L


def host_assign(L, x, c):
    """(labels int32 [N], dist2 float32 [N]) of the host build of gs_kmeans.h"""
    x, c = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)
    labels, dist2 = np.full(len(x) + 1, -7, np.int32), np.full(len(x) + 1, -7.0, np.float32)   # (a canary behind each)
    L.km_assign(len(x), len(c), x.shape[1], x.ctypes.data, c.ctypes.data, labels.ctypes.data, dist2.ctypes.data)
    assert labels[-1] == -7 and dist2[-1] == -7.0
    return labels[:-1], dist2[:-1]


def host_update(L, x, labels, c):
    """(centroids float32 [K, D], counts int32 [K]) of the host restatement of gs_kmeans_update; `c` is left alone"""
    x, out = np.ascontiguousarray(x, np.float32), np.array(c, np.float32, order="C", copy=True)
    labels, counts = np.ascontiguousarray(labels, np.int32), np.full(len(c), -7, np.int32)
    L.km_update(len(x), len(c), x.shape[1], x.ctypes.data, labels.ctypes.data, out.ctypes.data, counts.ctypes.data)
    return out, counts


def d64(x, c):
    """[N, K] squared distances in float64: |x|^2 - 2 x.c + |c|^2 on the float32 values.  Its own rounding, a few 2^-53 of
    (|x| + |c|)^2, is eight orders of magnitude below the float32 bound of `margin`."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.maximum((x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None, :], 0.0)


def margin(x, c, labels):
    """(gap [N], bound [N]): gap = d64(x, c_label) - min_c d64(x, c); bound = 2 (D + 2) 2^-24 (|x| + max_c |c|)^2 -- twice the
    worst-case error of a (D + 2)-term float32 chain (D products of the dot or the norm, the -2 and the final fma), once for the
    chosen centroid and once for the best."""
    d = d64(x, c)
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    gap = d[np.arange(len(d)), np.asarray(labels, np.int64)] - d.min(1)
    bound = 2.0 * (x64.shape[1] + 2) * U * (np.sqrt((x64 * x64).sum(1)) + np.sqrt((c64 * c64).sum(1)).max()) ** 2
    return gap, bound


def lloyd_step(x, c):
    """One Lloyd step in float64: (labels int64 [N], new centroids float64 [K, D], counts int64 [K]); ties to the smallest index, an
    empty cluster keeps its centroid."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    labels = d64(x, c).argmin(1)   # (numpy's argmin returns the first of equal minima)
    counts = np.bincount(labels, minlength=len(c64))
    sums = np.zeros_like(c64)
    np.add.at(sums, labels, x64)
    new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], c64)
    return labels, new, counts


def mean_bound(x, labels, K):
    """[K, D]: how far a float32 mean formed from a sequential float64 sum may lie from the float64 mean: half a float32 ulp of the
    result (2^-24 |mean|) plus the sum's own error, n 2^-53 sum|x| / n."""
    x64 = np.abs(np.asarray(x, np.float64))
    sabs = np.zeros((K, x64.shape[1]))
    np.add.at(sabs, np.asarray(labels, np.int64), x64)
    counts = np.bincount(labels, minlength=K)
    return U * sabs / np.maximum(counts, 1)[:, None] + 2.0 ** -53 * sabs * 2 + 1e-300


def int_labels(x, c):
    """The argmin of |x - c|^2 on integer-valued data in int64, the lowest index on ties."""
    xi, ci = np.asarray(x).astype(np.int64), np.asarray(c).astype(np.int64)
    assert np.array_equal(xi, x) and np.array_equal(ci, c)
    d = (xi * xi).sum(1)[:, None] - 2 * (xi @ ci.T) + (ci * ci).sum(1)[None, :]
    return d.argmin(1).astype(np.int32)


# ---- data ----

def gauss(n, k, d, seed, offset=0.0, spread=1.0):
    """(x [n, d], c [k, d]) float32: offset + spread * N(0, 1).  A large offset with a small spread is where the expansion
    |c|^2 - 2 x.c cancels: the scores of all centroids agree in their leading digits."""
    rng = np.random.default_rng(seed)
    x = (offset + spread * rng.standard_normal((n, d))).astype(np.float32)
    c = (offset + spread * rng.standard_normal((k, d))).astype(np.float32)
    return x, c


def int_ties(n, k, d, seed, dup_stride=(32, 128, 160)):
    """(x, c) of integers in -3..3 (every product and sum exact in float32) with duplicated centroids: centroid j reappears at
    j + s for every stride s that fits -- in another 32-column tile of the same LDS tile, in the next LDS tile, and in both."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-3, 4, (k, d)).astype(np.float32)
    for s in dup_stride:
        for j in range(0, k - s, 7):
            c[j + s] = c[j]
    x = rng.integers(-3, 4, (n, d)).astype(np.float32)
    x[: min(n, k)] = c[rng.permutation(k)[: min(n, k)]]   # points ON centroids: score ties of exactly equal copies
    return x, c
