"""Host half of the device k-NN initialisation (easy_gaussian_splatting_amd/knn.py, GaussianModel.from_pointcloud(knn=...)):
the brute-force reference of tests/knn_ref.py against sklearn, the argument errors -- all raised before any native call --
and the untouched host path.  No GPU."""
import numpy as np
import pytest
import torch

import knn_ref as KR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import scene as S
from easy_gaussian_splatting_amd.knn import LEAF, MAX_K, knn_distances
from easy_gaussian_splatting_amd.model import GaussianModel


def _cloud_with_coincident_groups(n=300, seed=3):
    """n uniform points, among them groups of 2, 4 and 5 coincident ones (scattered over the rows)."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    for rows in ([7, 150], [20, 21, 199, 260], [3, 90, 91, 170, 299]):
        p[rows] = p[rows[0]]
    return p


def test_reference_equals_sklearn_with_coincident_points():
    nn = pytest.importorskip("sklearn.neighbors")
    p = _cloud_with_coincident_groups()
    for k in (1, 3, 8):
        ref = KR.knn_ref_numpy(p, k)
        sk = nn.NearestNeighbors(n_neighbors=k + 1, metric="euclidean").fit(p).kneighbors(p)[0][:, 1:]
        assert ref.shape == sk.shape == (300, k) and np.all(np.diff(ref, axis=1) >= 0)
        assert np.allclose(ref, sk, rtol=1e-12, atol=0.0)
        assert np.array_equal(ref == 0.0, sk == 0.0)
        tr = KR.knn_ref_torch(torch.from_numpy(p), k, chunk=64).numpy()
        assert np.allclose(tr, ref, rtol=1e-14, atol=0.0) and np.array_equal(tr == 0.0, ref == 0.0)
    # the group of 5 has 4 coincident neighbours, the group of 4 has 3, the pair 1
    r3 = KR.knn_ref_numpy(p, 3)
    assert np.all(r3[[3, 90, 91, 170, 299]] == 0.0) and np.all(r3[[20, 21, 199, 260]] == 0.0)
    assert np.all(r3[[7, 150], 0] == 0.0) and np.all(r3[[7, 150], 1] > 0.0)


def test_reference_on_the_line_example():
    """Exclusion is by index, not by distance: 0, 0, 1, 2, 5 on a line."""
    p = np.zeros((5, 3))
    p[:, 0] = [0, 0, 1, 2, 5]
    want = np.array([[0, 1, 2], [0, 1, 2], [1, 1, 1], [1, 2, 2], [3, 4, 5]], dtype=np.float64)
    assert np.array_equal(KR.knn_ref_numpy(p, 3), want)
    assert np.array_equal(KR.knn_ref_torch(torch.from_numpy(p), 3).numpy(), want)
    nn = pytest.importorskip("sklearn.neighbors")
    assert np.array_equal(nn.NearestNeighbors(n_neighbors=4).fit(p).kneighbors(p)[0][:, 1:], want)


def test_constants_come_from_the_header():
    assert (LEAF, MAX_K) == (nat.DEFINES["GS_KNN_LEAF"], nat.DEFINES["GS_KNN_MAX_K"]) == (64, 8)
    assert nat.DEFINES["GS_KNN_MAX_N"] == 2 ** 30
    assert nat.PARAMS["gs_knn_dists"] == ["stream", "N", "k", "points", "order", "dists", "workspace"]


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the native library fails the test: the errors below are raised before it is looked at."""
    def boom():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(nat, "lib", boom)


def test_knn_distances_argument_errors(no_native):
    good = torch.rand((10, 3))
    for bad in (torch.rand((10, 2)), torch.rand((10, 3, 1)), torch.rand((30,))):
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            knn_distances(bad)
    with pytest.raises(ValueError, match="float32"):
        knn_distances(good.double())
    with pytest.raises(ValueError, match="float32"):
        knn_distances(torch.zeros((10, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        knn_distances(torch.rand((3, 10)).t())
    for k in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            knn_distances(good, k=k)
    with pytest.raises(ValueError, match="at least 4 points"):
        knn_distances(torch.rand((3, 3)), k=3)
    with pytest.raises(ValueError, match="at least 9 points"):
        knn_distances(torch.rand((8, 3)), k=8)
    for v in (float("nan"), float("inf"), -float("inf")):
        bad = good.clone()
        bad[4, 1] = v
        with pytest.raises(ValueError, match="NaN or infinity"):
            knn_distances(bad)
        with pytest.raises(NotImplementedError, match="runs on the GPU only"):   # (not looked at without the check)
            knn_distances(bad, check_finite=False)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        knn_distances(good)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        knn_distances(torch.rand((4, 3)), k=3)   # the smallest legal cloud


def test_native_entries_refuse_bad_sizes_without_launching():
    """The C entry points' own range checks (status code + message), on host pointers that are never dereferenced."""
    import ctypes as ct
    L = nat.lib()
    buf = (ct.c_char * 1024)()
    p = (ct.addressof(buf) + 255) & ~255
    assert L.gs_knn_dists(None, 3, 3, p, p, p, p) == -1 and b"k + 1" in L.gs_last_error()
    assert L.gs_knn_dists(None, 100, 0, p, p, p, p) == -1 and b"GS_KNN_MAX_K" in L.gs_last_error()
    assert L.gs_knn_dists(None, 100, 9, p, p, p, p) == -1
    assert L.gs_knn_dists(None, 2 ** 30 + 1, 3, p, p, p, p) == -1 and b"GS_KNN_MAX_N" in L.gs_last_error()
    assert L.gs_knn_dists(None, 100, 3, p, None, p, p) == -1 and b"null" in L.gs_last_error()
    assert L.gs_knn_dists(None, 100, 3, p, p, p, p + 16) == -1 and b"aligned" in L.gs_last_error()
    assert L.gs_knn_codes(None, 1, p, p, p) == -1 and L.gs_knn_codes(None, 2 ** 30 + 1, p, p, p) == -1
    assert L.gs_knn_codes(None, 100, p, None, p) == -1
    assert L.gs_knn_workspace_bytes(0) == 0 and L.gs_knn_workspace_bytes(2 ** 30 + 1) == 0
    # 32 KB of partial boxes + the box, then 16 B per padded point, 32 B per leaf and per node, each part 256-byte aligned
    assert L.gs_knn_workspace_bytes(65) == 32768 + 256 + 2 * 64 * 16 + 256 + 256
    assert L.gs_knn_workspace_bytes(10 ** 6) == 32768 + 256 + 15625 * 64 * 16 + 500224 + 7936   # (15625 x 32 B = 500000 -> 500224; 245 nodes x 32 B = 7840 -> 7936)


def _pc(n=60, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return S.Pointcloud(rng.random((n, 3)).astype(dtype), rng.integers(0, 256, (n, 3), dtype=np.uint8))


def test_from_pointcloud_argument_errors(no_native):
    pc = _pc()
    for bad in ("gpu", "cuda", "", None, True):
        with pytest.raises(ValueError, match="knn"):
            GaussianModel.from_pointcloud(pc, 1, knn=bad)
    with pytest.raises(ValueError, match="device"):
        GaussianModel.from_pointcloud(pc, 1, knn="host", device="cuda:0")
    with pytest.raises(TypeError):
        GaussianModel.from_pointcloud(pc, 1, 0, "device")   # keyword-only
    with pytest.raises(NotImplementedError, match="GPU only"):
        GaussianModel.from_pointcloud(pc, 1, knn="device", device="cpu")
    with pytest.raises(ValueError, match="N >= 4"):
        GaussianModel.from_pointcloud(S.Pointcloud(pc.xyzs[:3], pc.rgbs[:3]), 1, knn="device", device="cpu")
    bad = pc.xyzs.copy()
    bad[5, 0] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        GaussianModel.from_pointcloud(S.Pointcloud(bad, pc.rgbs), 1, knn="device", device="cpu")


def test_default_is_the_host_path_bit_for_bit():
    pytest.importorskip("sklearn")
    for dtype in (np.float64, np.float32):
        pc = _pc(200, 1, dtype)
        a = GaussianModel.from_pointcloud(pc, sh_degree=2, sh_degree_interval=1000, white_background=True)
        b = GaussianModel.from_pointcloud(pc, sh_degree=2, sh_degree_interval=1000, knn="host", white_background=True)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and len(sa) >= 7
        for name in sa:
            assert sa[name].device.type == "cpu" and sa[name].dtype == sb[name].dtype
            assert torch.equal(sa[name].view(torch.int32), sb[name].view(torch.int32)), name
        assert a.active_sh_degree == b.active_sh_degree == 0 and a.MAX_SH_DEGREE == b.MAX_SH_DEGREE == 2
        # today's values: the scales are half the mean of sklearn's three distances, formed in float32
        from sklearn.neighbors import NearestNeighbors
        d = NearestNeighbors(n_neighbors=4, metric="euclidean").fit(pc.xyzs).kneighbors(pc.xyzs)[0][:, 1:].astype(np.float32)
        want = torch.log(torch.tensor(np.repeat(d.mean(axis=1, keepdims=True), 3, axis=1), dtype=torch.float32) / 2.0)
        assert torch.equal(a.log_scales.detach(), want)
