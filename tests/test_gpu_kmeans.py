"""The device k-means (csrc/gs_kmeans.hip through easy_gaussian_splatting_amd/kmeans.py) against two independent things:

  * tests/hostmath/kmeans.cpp, the host build of csrc/gs_kmeans.h -- the device's own text.  Labels, dist2, centroids and counts must
    match it BIT FOR BIT: the kernel's tiling, its MFMA and its reductions may not change a single rounding or tie;
  * float64 (tests/kmeans_ref.py): the chosen centroid is within 2 (D + 2) 2^-24 (|x| + max |c|)^2 of the nearest one.

The sizes are the smallest that straddle every edge of the kernel: N around the wave's 32 rows and the block's 128 points, K around
the 32-column accumulator tile and the 128-centroid LDS tile, D odd (the zero-padded k-step of 2), 1, and the maximum 128.  Every
value of N, K and D meets every value of the other two: 8 K x 8 D pairs cannot be met by fewer than 64 cases, a Latin square over N
gives exactly 64, all tiny.  Every native call here writes into buffers with a canary row behind them."""
import numpy as np
import pytest
import torch

import kmeans_ref as KR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import kmeans as KM

pytestmark = pytest.mark.gpu

NS = (1, 31, 33, 127, 129, 257, 1000)
KS = (1, 2, 31, 32, 33, 127, 129, 300)
DS = (1, 2, 3, 9, 24, 45, 72, 128)
CANARY = 64


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def km(tmp_path_factory):
    return KR.host_lib(tmp_path_factory.mktemp("kmeans"))


def _assign_raw(x, c):
    """gs_kmeans_assign through the C ABI into buffers with a canary row behind them -> (labels, dist2) numpy"""
    dev, L = _dev(), nat.lib()
    n, d, k = x.shape[0], x.shape[1], c.shape[0]
    xd, cd = torch.from_numpy(x).to(dev).contiguous(), torch.from_numpy(c).to(dev).contiguous()
    labels = torch.full((n + CANARY,), -7, dtype=torch.int32, device=dev)
    dist2 = torch.full((n + CANARY,), -7.0, dtype=torch.float32, device=dev)
    ws = torch.empty((int(L.gs_kmeans_workspace_bytes(n, k, d)),), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.check(L.gs_kmeans_assign(st, n, k, d, xd.data_ptr(), cd.data_ptr(), labels.data_ptr(), dist2.data_ptr(), ws.data_ptr()), "gs_kmeans_assign")
    torch.cuda.synchronize()
    labels, dist2 = labels.cpu().numpy(), dist2.cpu().numpy()
    assert (labels[n:] == -7).all() and (dist2[n:] == -7.0).all(), "a write behind the last point"
    assert np.array_equal(cd.cpu().numpy().view(np.int32), c.view(np.int32)) and np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32))
    return labels[:n], dist2[:n]


def _same_bits(got_labels, got_dist2, want_labels, want_dist2, what):
    bad = np.flatnonzero(got_labels != want_labels)
    assert bad.size == 0, f"{what}: {bad.size} labels differ from the host build, first at point {bad[0]}: {got_labels[bad[0]]} vs {want_labels[bad[0]]}"
    bad = np.flatnonzero(got_dist2.view(np.int32) != want_dist2.view(np.int32))
    assert bad.size == 0, f"{what}: {bad.size} dist2 differ in their bits, first at point {bad[0]}: {got_dist2[bad[0]]!r} vs {want_dist2[bad[0]]!r}"


@pytest.mark.parametrize("ki", range(len(KS)))
def test_assign_is_the_host_build_bit_for_bit(km, ki):
    k = KS[ki]
    for di, d in enumerate(DS):
        n = NS[(ki + di) % len(NS)]
        # centroids drawn near the points, so that the nearest ones compete; an offset on every second case (cancellation)
        x, c = KR.gauss(n, k, d, seed=1000 * ki + di, offset=1.5 * ((ki + di) & 1), spread=0.5)
        got = _assign_raw(x, c)
        _same_bits(*got, *KR.host_assign(km, x, c), f"N = {n}, K = {k}, D = {d}")


@pytest.mark.parametrize("n,k,d", [(257, 300, 3), (129, 300, 45), (1000, 129, 2), (33, 33, 1)])
def test_integer_ties_across_lanes_and_tiles(km, n, k, d):
    """Exactly equal scores: duplicated centroids 32, 128 and 160 columns apart -- another accumulator tile, another LDS tile, both --
    and points ON centroids.  A reduction that forgets the index picks a copy at a higher one."""
    x, c = KR.int_ties(n, k, d, seed=n + k + d)
    labels, dist2 = _assign_raw(x, c)
    want = KR.int_labels(x, c)
    assert np.array_equal(labels, want), f"{int((labels != want).sum())} labels are not the lowest index among the nearest"
    _same_bits(labels, dist2, *KR.host_assign(km, x, c), "integer ties")
    # the operand maps: with asymmetric integer data a swapped row / column or a wrong k would move labels; dist2 is exact too
    assert np.array_equal(dist2.astype(np.int64), ((x - c[want]).astype(np.int64) ** 2).sum(1))


def test_the_last_of_65536_centroids_is_reached(km):
    """N = 512, K = 65 536, D = 45 at the scale of a trained sh_rest; one point planted on the last centroid.  The whole result is
    held to the float64 margin; a slice of it -- the planted point among them -- to the host build bit for bit (the host walk of
    all 512 x 65 536 pairs would take longer than the rest of this file)."""
    n, k, d = 512, 65536, 45
    x, c = KR.gauss(n, k, d, seed=11, spread=0.05)
    x[n - 1] = c[k - 1]
    labels, dist2 = _assign_raw(x, c)
    assert labels[n - 1] == k - 1 and dist2[n - 1] == 0.0
    assert labels.min() >= 0 and labels.max() <= k - 1
    as_u16 = labels.astype(np.uint16)
    assert np.array_equal(as_u16.astype(np.int32), labels) and as_u16[n - 1] == 65535   # the compact file's uint16 store is exact
    gap, bound = KR.margin(x, c, labels)
    assert (gap <= bound).all(), f"worst gap / bound = {float((gap / bound).max()):.3g}"
    rows = np.r_[0:24, 250:262, n - 12:n]
    want = KR.host_assign(km, x[rows], c)
    _same_bits(labels[rows], dist2[rows], *want, "K = 65536")


@pytest.mark.parametrize("d,offset,spread", [(9, 0.0, 1.0), (45, 0.0, 1.0), (72, 0.0, 1.0), (45, 3.0, 0.02)])
def test_assign_against_fp64(d, offset, spread):
    """The host file's margin, on the kernel's own labels: N = 1500, K = 4096; the offset case is where cancellation bites."""
    x, c = KR.gauss(1500, 4096, d, seed=100 + d if offset == 0.0 else 7, offset=offset, spread=spread)
    labels, dist2 = _assign_raw(x, c)
    gap, bound = KR.margin(x, c, labels)
    print(f"[kmeans] D = {d}, offset {offset}: labels off the fp64 argmin = {int((gap > 0).sum())}, worst gap / bound = {float((gap / bound).max()):.3g}")
    assert (gap <= bound).all()
    ref = KR.d64(x, c)[np.arange(len(x)), labels]
    if offset == 0.0:
        assert np.array_equal(labels, KR.d64(x, c).argmin(1))
        assert (np.abs(dist2 - ref) <= 2 * (d + 1) * KR.U * ref).all()


def _update_raw(x, labels, c):
    dev, L = _dev(), nat.lib()
    n, d, k = x.shape[0], x.shape[1], c.shape[0]
    xd, ld = torch.from_numpy(x).to(dev).contiguous(), torch.from_numpy(labels.astype(np.int32)).to(dev)
    cent = torch.full((k + 1, d), -7.0, dtype=torch.float32, device=dev)
    cent[:k] = torch.from_numpy(c).to(dev)
    counts = torch.full((k + CANARY,), -7, dtype=torch.int32, device=dev)
    order = torch.sort(ld, stable=True).indices.to(torch.int32)
    seg = torch.zeros((k + 1,), dtype=torch.int32, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(ld, minlength=k), 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.check(L.gs_kmeans_update(st, n, k, d, xd.data_ptr(), order.data_ptr(), seg.data_ptr(), cent.data_ptr(), counts.data_ptr()), "gs_kmeans_update")
    torch.cuda.synchronize()
    cent, counts = cent.cpu().numpy(), counts.cpu().numpy()
    assert (cent[k] == -7.0).all() and (counts[k:] == -7).all(), "a write behind the last cluster"
    return cent[:k], counts[:k]


@pytest.mark.parametrize("case", ["random", "empty", "one_cluster", "k_above_n", "d1", "d128"])
def test_update_is_the_host_restatement_bit_for_bit(km, case):
    n, k, d = {"random": (1000, 37, 45), "empty": (1000, 300, 72), "one_cluster": (1000, 5, 45), "k_above_n": (31, 129, 9),
               "d1": (257, 3, 1), "d128": (129, 33, 128)}[case]
    rng = np.random.default_rng(len(case))
    x, c = KR.gauss(n, k, d, seed=20 + len(case), offset=0.7)
    labels = rng.integers(0, k, n).astype(np.int32)
    if case == "empty":
        labels[labels % 3 == 1] += 1              # every third cluster is empty
    if case == "one_cluster":
        labels[:] = 3                             # more members than one 64-wide batch, many times over
    want, want_counts = KR.host_update(km, x, labels, c)
    got, counts = _update_raw(x, labels, c)
    assert np.array_equal(counts, want_counts) and np.array_equal(counts, np.bincount(labels, minlength=k))
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, f"{len(bad)} centroid coordinates differ in their bits, first at {bad[0]}"
    empty = counts == 0
    assert np.array_equal(got[empty].view(np.int32), c[empty].view(np.int32))   # an empty cluster keeps its bits
    if case in ("empty", "k_above_n"):
        assert empty.any()
    # and the host restatement itself is the float64 mean
    new64 = np.zeros((k, d))
    np.add.at(new64, labels, x.astype(np.float64))
    new64 = np.where(~empty[:, None], new64 / np.maximum(counts, 1)[:, None], c.astype(np.float64))
    assert (np.abs(got - new64) <= KR.mean_bound(x, labels, k)).all()


def test_kmeans_recovers_eight_blobs():
    """Eight blobs 10 apart with spread 0.3, init = one point of each: the labels are the blob membership after two iterations and
    the inertia never increases (Lloyd's steps cannot raise it; relative slack 1e-6 for the float32 distances)."""
    dev = _dev()
    rng = np.random.default_rng(8)
    centres = (10.0 * rng.standard_normal((8, 24))).astype(np.float32)
    member = np.arange(2000) % 8
    x = (centres[member] + 0.3 * rng.standard_normal((2000, 24))).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    init = xd[:8].clone()                         # point i belongs to blob i
    cent, labels, inertia = KM.kmeans(xd, 8, iters=2, init=init)
    assert torch.equal(init, xd[:8]) and cent.shape == (8, 24) and labels.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), member)
    assert len(inertia) == 3 and all(t.dim() == 0 and t.dtype == torch.float64 and t.device.type == "cuda" for t in inertia)
    vals = [float(t) for t in inertia]
    assert all(b <= a * (1 + 1e-6) for a, b in zip(vals, vals[1:])), vals
    mean64 = np.stack([x[member == b].astype(np.float64).mean(0) for b in range(8)])
    assert (np.abs(cent.cpu().numpy() - mean64) <= KR.mean_bound(x, member, 8)).all()
    # a seeded run is reproducible, bit for bit, and needs no init
    a = KM.kmeans(xd, 8, iters=3, generator=torch.Generator().manual_seed(5))
    b = KM.kmeans(xd, 8, iters=3, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    v = [float(t) for t in a[2]]
    assert all(q <= p * (1 + 1e-6) for p, q in zip(v, v[1:])), v
