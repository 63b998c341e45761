"""The k-means definition (csrc/gs_kmeans.h) built with the host compiler -- the device's own text -- and held to float64: no GPU.

The bound (kmeans_ref.margin): with d64 the squared distance in float64,
    d64(x, c_label) - min_c d64(x, c) <= 2 (D + 2) 2^-24 (|x| + max_c |c|)^2,
twice the worst-case error of a (D + 2)-term float32 chain, once for the chosen centroid and once for the best.  On zero-mean data
the labels ARE the float64 argmin; at offset 3.0 with spread 0.02 the expansion |c|^2 - 2 x.c cancels and some labels differ, inside
the bound.  On small-integer data every operation is exact and the labels are the brute-force argmin, the lowest index on ties."""
import numpy as np
import pytest
import torch

import kmeans_ref as KR

N, K = 1500, 4096


@pytest.fixture(scope="module")
def km(tmp_path_factory):
    return KR.host_lib(tmp_path_factory.mktemp("kmeans"))


@pytest.mark.parametrize("d", (9, 45, 72))
def test_zero_mean_labels_are_the_fp64_argmin(km, d):
    x, c = KR.gauss(N, K, d, seed=100 + d)
    labels, dist2 = KR.host_assign(km, x, c)
    gap, bound = KR.margin(x, c, labels)
    print(f"[kmeans host] D = {d}: labels off the fp64 argmin = {int((gap > 0).sum())}, worst gap / bound = {float((gap / bound).max()):.3g}")
    assert (gap <= bound).all()
    assert np.array_equal(labels, KR.d64(x, c).argmin(1))
    ref = KR.d64(x, c)[np.arange(N), labels]
    assert (np.abs(dist2 - ref) <= 2 * (d + 1) * KR.U * ref).all()   # a chain of D squares of differences rounded once each


def test_offset_data_stays_inside_the_bound(km):
    """Offset 3.0, spread 0.02: the scores agree in their leading digits.  Labels may differ from the fp64 argmin -- by centroids that
    are as near as float32 can tell."""
    x, c = KR.gauss(N, K, 45, seed=7, offset=3.0, spread=0.02)
    labels, _ = KR.host_assign(km, x, c)
    gap, bound = KR.margin(x, c, labels)
    print(f"[kmeans host] offset: labels off the fp64 argmin = {int((gap > 0).sum())}, worst gap / bound = {float((gap / bound).max()):.3g}")
    assert (gap <= bound).all()
    assert (labels >= 0).all() and (labels < K).all()


@pytest.mark.parametrize("n,k,d", [(257, 300, 3), (200, 129, 9), (64, 2, 1), (300, 300, 45)])
def test_integer_data_lowest_index_on_ties(km, n, k, d):
    x, c = KR.int_ties(n, k, d, seed=n + k + d)
    want = KR.int_labels(x, c)
    labels, dist2 = KR.host_assign(km, x, c)
    assert np.array_equal(labels, want)
    assert np.array_equal(dist2.astype(np.int64), ((x - c[want]).astype(np.int64) ** 2).sum(1))


def test_a_duplicate_at_a_higher_index_is_never_chosen(km):
    x, c = KR.gauss(400, 200, 24, seed=3)
    c2 = np.concatenate([c, c[::-1]])          # centroid j again at 399 - j
    labels, _ = KR.host_assign(km, x, c2)
    first, _ = KR.host_assign(km, x, c)
    assert labels.max() < 200 and np.array_equal(labels, first)


def test_a_nan_score_never_wins(km):
    x, c = KR.gauss(50, 20, 9, seed=4)
    c[0, 3] = np.nan
    c[7] = np.inf                               # norm +inf, dot +-inf: inf - inf = NaN
    labels, _ = KR.host_assign(km, x, c)
    ok = np.delete(np.arange(20), [0, 7])
    assert np.array_equal(labels, ok[KR.d64(x, c[ok]).argmin(1)])
    allnan = np.full((3, 9), np.nan, np.float32)
    labels, dist2 = KR.host_assign(km, x, allnan)
    assert (labels == 0).all() and np.isnan(dist2).all()   # nobody wins: label 0


def test_update_is_the_fp64_lloyd_step(km):
    x, c = KR.gauss(1000, 37, 45, seed=5)
    labels = KR.lloyd_step(x, c)[0]
    labels[labels == 11] = 12                   # an empty cluster
    new64, counts64 = _mean64(x, labels, c)
    got, counts = KR.host_update(km, x, labels.astype(np.int32), c)
    assert np.array_equal(counts, counts64) and counts[11] == 0
    assert np.array_equal(got[11].view(np.int32), c[11].view(np.int32))   # kept, bit for bit
    assert (np.abs(got - new64) <= KR.mean_bound(x, labels, len(c))).all()


def _mean64(x, labels, c):
    counts = np.bincount(labels, minlength=len(c))
    sums = np.zeros((len(c), x.shape[1]))
    np.add.at(sums, labels, x.astype(np.float64))
    return np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], c.astype(np.float64)), counts


def test_lloyd_step_reference_on_a_case_done_by_hand():
    x = np.array([[0.0], [1.0], [10.0], [11.0], [5.5]], np.float32)
    c = np.array([[0.0], [11.0], [100.0]], np.float32)
    labels, new, counts = KR.lloyd_step(x, c)
    assert labels.tolist() == [0, 0, 1, 1, 0] and counts.tolist() == [3, 2, 0]   # 5.5: a tie, the smaller index
    assert new[:, 0].tolist() == [6.5 / 3, 10.5, 100.0]


# ---- the front end and the C ABI, as far as they go without a device ----

def test_kmeans_front_end_without_a_device():
    from easy_gaussian_splatting_amd import kmeans as KM
    x = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    cent, labels, inertia = KM.kmeans(x, 4)
    assert torch.equal(cent, x) and cent is not x and labels.tolist() == [0, 1, 2, 3] and labels.dtype == torch.int32 and inertia == []
    cent, labels, _ = KM.kmeans(x, 65536)
    assert torch.equal(cent, x) and labels.tolist() == [0, 1, 2, 3]
    with pytest.raises(NotImplementedError):
        KM.kmeans(x, 2)
    for bad in (x.double(), x.t(), x[0], "x"):
        with pytest.raises(ValueError):
            KM.kmeans(bad, 2)
    for k in (0, -1, 2.0, True, KM.MAX_K + 1):
        with pytest.raises(ValueError):
            KM.kmeans(x, k)
    with pytest.raises(ValueError):
        KM.kmeans(x, 2, iters=-1)
    with pytest.raises(ValueError):
        KM.kmeans(x, 2, init=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        KM.kmeans(torch.zeros(4, KM.MAX_D + 1), 2)
    with pytest.raises(NotImplementedError):
        KM.assign(x, x[:2].contiguous())


def test_bad_arguments_are_refused_before_a_launch():
    from easy_gaussian_splatting_amd import _native as nat
    L = nat.lib()
    assert (nat.GS_KMEANS_MAX_D, nat.GS_KMEANS_MAX_K, nat.GS_KMEANS_MAX_N) == (128, 2 ** 24, 2 ** 30)
    assert L.gs_kmeans_workspace_bytes(1000, 300, 45) >= 4 * (46 * 384 + 384)
    assert L.gs_kmeans_workspace_bytes(1000, 300, 45) % 256 == 0
    for n, k, d in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 129), (2 ** 30 + 1, 1, 1), (1, 2 ** 24 + 1, 1)):
        assert L.gs_kmeans_workspace_bytes(n, k, d) == 0
        assert L.gs_kmeans_assign(None, n, k, d, 256, 256, 256, 256, 256) == nat.GS_ERR_ARG
        assert L.gs_kmeans_update(None, n, k, d, 256, 256, 256, 256, 256) == nat.GS_ERR_ARG
    assert L.gs_kmeans_assign(None, 10, 2, 3, None, 256, 256, 256, 256) == nat.GS_ERR_ARG
    assert L.gs_kmeans_assign(None, 10, 2, 3, 256, 256, 256, 256, 260) == nat.GS_ERR_ARG and b"aligned" in L.gs_last_error()
    assert L.gs_kmeans_update(None, 10, 2, 3, 256, 256, None, 256, 256) == nat.GS_ERR_ARG
