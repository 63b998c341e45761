"""The device k-NN search (csrc/gs_knn.hip through easy_gaussian_splatting_amd/knn.py) and `GaussianModel.from_pointcloud(knn="device")`.

Reference: tests/knn_ref.py, brute force in float64 on the SAME float32 coordinates, on the device.
Tolerance: with the same float32 inputs sqrt(fl(dx^2 + dy^2 + dz^2)) carries at most about 3.5 u (u = 2^-24) of relative error -- each
difference 1 u, so each square 2 u and the sum of non-negative terms no more, two roundings of the sum, half of all that through the
root, the root's own u -- and a leaf passed over on a rounded lower bound could add a few more (the kernel's bound is the same rounded
expression, so it adds none).  Required: |d - d_ref| <= 2^-20 d_ref (16 u), and a reference distance of exactly 0 comes out as
exactly 0.0.  All inputs keep their non-zero distances far above 1e-12 (nothing underflows when squared); no NaN or infinity ever
reaches a kernel here."""
import numpy as np
import pytest
import torch

import knn_ref as KR
from easy_gaussian_splatting_amd import scene as S
from easy_gaussian_splatting_amd.knn import LEAF, knn_distances
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers

pytestmark = pytest.mark.gpu
RTOL = 2.0 ** -20
N_DIST = 4099


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _check(d, ref, what=""):
    """d [N, k] float32 from the code under test, ref [N, k] float64 (same device)."""
    assert d.dtype == torch.float32 and d.shape == ref.shape and d.device == ref.device, what
    d64 = d.double()
    assert bool(torch.isfinite(d64).all()), what
    assert bool((d64[:, 1:] >= d64[:, :-1]).all()), f"{what}: rows not ascending"
    zero = ref == 0.0
    assert bool((d64[zero] == 0.0).all()), f"{what}: a reference distance of 0 came out as {float(d64[zero].abs().max())}"
    assert float(ref[~zero].min()) > 1e-12 if bool((~zero).any()) else True, what
    err = (d64 - ref).abs()
    worst = float((err / ref.clamp_min(1e-300))[~zero].max()) if bool((~zero).any()) else 0.0
    print(f"[knn] {what}: N = {d.shape[0]}, k = {d.shape[1]}, zeros = {int(zero.sum())}, worst relative error = {worst / 2.0 ** -24:.2f} u")
    assert bool((err <= RTOL * ref).all()), f"{what}: worst relative error {worst:.3e} > 2^-20"


def _uniform(n, seed):
    return torch.rand((n, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _clustered(n, seed, n_centres=40, lo=-5.0, hi=-1.0):
    """Cluster spreads over 10^lo .. 10^hi (a 1e4 ratio by default) around centres in the unit cube."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand((n_centres, 3), generator=g, dtype=torch.float64)
    spread = 10.0 ** (lo + (hi - lo) * torch.arange(n_centres, dtype=torch.float64) / (n_centres - 1))
    which = torch.randint(0, n_centres, (n,), generator=g)
    return (centres[which] + spread[which, None] * torch.randn((n, 3), generator=g, dtype=torch.float64)).float()


def _with_groups(n, seed):
    p = _uniform(n, seed)
    for rows in ([5, 3000], [17, 18, 2047, 4098], [0, 63, 64, 1000, 4000]):   # groups of 2, 4 and 5, across leaves
        p[rows] = p[rows[0]].clone()
    return p


def _lattice():
    a = torch.arange(16, dtype=torch.float32) / 16.0
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def _distribution(name):
    n = N_DIST
    if name == "uniform":
        return _uniform(n, 11)
    if name == "clustered":
        return _clustered(n, 12)
    if name == "line":            # two axes of zero extent
        p = torch.full((n, 3), 0.25)
        p[:, 1] = _uniform(n, 13)[:, 0] * 3.0 - 1.0
        return p
    if name == "plane":
        p = _uniform(n, 14)
        p[:, 0] = -0.75
        return p
    if name == "identical":
        return torch.tensor([[0.3, -1.2, 2.5]]).repeat(n, 1)
    if name == "groups":
        return _with_groups(n, 15)
    if name == "lattice":
        return _lattice()
    if name == "outlier":         # the Morton grid collapses: the whole unit cloud falls into a few cells
        p = _uniform(n, 16)
        p[1234] = torch.tensor([1e6, -1e6, 1e6])
        return p
    if name == "offset":          # float32 granularity 6e-5 at 1e3: the reference sees the same float32 values
        return _uniform(n, 17) + torch.tensor([1e3, -1e3, 1e3])
    raise KeyError(name)


_CACHE = {}


def _case(key, make, k):
    """(points on the device, float64 reference): built once per (cloud, k), shared, never written."""
    if (key, k) not in _CACHE:
        if key not in _CACHE:
            _CACHE[key] = make().to(_dev()).contiguous()
        _CACHE[(key, k)] = KR.knn_ref_torch(_CACHE[key], k)
    return _CACHE[key], _CACHE[(key, k)]


SIZES = [9, 63, 64, 65, LEAF - 1, LEAF, LEAF + 1, 4099, 8209]
SIZE_CASES = [(4, 3)] + [(n, k) for n in dict.fromkeys(SIZES) for k in (1, 3, 8)]


@pytest.mark.parametrize("n, k", SIZE_CASES)
def test_sizes(n, k):
    """The minimum legal N, wave and leaf edges (the leaf is one wave: LEAF = 64 from the header), several leaves, blocks and nodes."""
    assert LEAF == 64 and 8209 > 2 * 64 * LEAF   # (8209 points: 129 leaves, three nodes)
    p, ref = _case(("uniform", n), lambda: _uniform(n, 100 + n), k)
    _check(knn_distances(p, k), ref, f"uniform {n}")


@pytest.mark.parametrize("name", ["uniform", "clustered", "line", "plane", "identical", "groups", "lattice", "outlier", "offset"])
def test_distributions(name):
    p, ref = _case(("dist", name), lambda: _distribution(name), 3)
    d = knn_distances(p, 3)
    _check(d, ref, name)
    if name == "identical":
        assert int(torch.count_nonzero(d)) == 0
    if name == "groups":
        assert bool((d[[0, 63, 64, 1000, 4000]] == 0).all()) and bool((d[[17, 18, 2047, 4098]] == 0).all())
        assert bool((d[[5, 3000], 0] == 0).all()) and bool((d[[5, 3000], 1] > 0).all())
    if name == "lattice":   # every point's nearest neighbours are exactly one spacing away
        assert bool((d == 1.0 / 16.0).all())


def test_identical_points_with_eight_neighbours():
    p, ref = _case(("dist", "identical"), lambda: _distribution("identical"), 8)
    d = knn_distances(p, 8)
    _check(d, ref, "identical, k = 8")
    assert int(torch.count_nonzero(d)) == 0


def test_larger_clustered_cloud():
    """70 001 points, 1094 leaves, 18 nodes: the case where rejecting boxes decides most of the work."""
    p, ref = _case(("clustered", 70001), lambda: _clustered(70001, 21, n_centres=200), 3)
    _check(knn_distances(p, 3), ref, "clustered 70001")


def test_rows_follow_the_input_order():
    p, ref = _case(("dist", "clustered"), lambda: _distribution("clustered"), 3)
    d = knn_distances(p, 3)
    perm = torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(5)).to(p.device)
    dp = knn_distances(p[perm].contiguous(), 3)
    _check(dp, ref[perm], "clustered, shuffled")
    assert torch.equal(dp, d[perm])   # the rows depend on the points alone, not on where they stand


def test_two_calls_give_the_same_bits():
    for key, name in ((("dist", "clustered"), "clustered"), (("dist", "lattice"), "lattice")):
        p, _ = _case(key, lambda: _distribution(name), 3)
        a, b = knn_distances(p, 3), knn_distances(p, 3)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_on_a_side_stream_between_other_work():
    p, ref = _case(("dist", "uniform"), lambda: _distribution("uniform"), 3)
    want = knn_distances(p, 3)
    side = torch.cuda.Stream(device=p.device)
    side.wait_stream(torch.cuda.current_stream(p.device))
    with torch.cuda.stream(side):
        a = torch.ones((1024, 1024), device=p.device)
        for _ in range(8):
            a = (a @ a) * 1e-3          # work queued in front
        got = knn_distances(p, 3)
        b = a @ a                        # and behind
    side.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(b).all())
    _check(got, ref, "side stream")


def test_check_finite_refuses_before_a_launch():
    p = _uniform(100, 1).to(_dev())
    p[7, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN or infinity"):
        knn_distances(p)


# ---- GaussianModel.from_pointcloud(knn="device")

def _pc(shift):
    rng = np.random.default_rng(42)
    xyz = rng.random((2000, 3)) + np.asarray(shift, dtype=np.float64)
    return S.Pointcloud(xyz, rng.integers(0, 256, (2000, 3), dtype=np.uint8))


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (1e4, 1e4, 1e4)], ids=["unit", "shifted"])
def test_from_pointcloud_on_the_device(shift):
    pytest.importorskip("sklearn")   # (the host path this is compared with)
    dev = _dev()
    pc = _pc(shift)
    x64 = np.asarray(pc.xyzs, dtype=np.float64)
    m = GaussianModel.from_pointcloud(pc, sh_degree=2, sh_degree_interval=1000, knn="device", device=dev, white_background=True)
    host = GaussianModel.from_pointcloud(pc, sh_degree=2, sh_degree_interval=1000, white_background=True)
    for name, t in list(m.named_parameters()) + list(m.named_buffers()):
        assert t.device == dev, name
    # scales: half the mean of the float64 brute-force distances on the float64 coordinates
    want = 0.5 * KR.knn_ref_numpy(x64, 3).mean(axis=1)
    centred = x64 - 0.5 * (x64.min(axis=0) + x64.max(axis=0))
    bound = 4.0 * 2.0 ** -24 * np.sqrt(3.0) * np.abs(centred).max() + 2.0 ** -20 * want
    got = m.scales.detach().cpu().double().numpy()
    assert got.shape == (2000, 3) and np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    err = np.abs(got[:, 0] - want)
    print(f"[knn] from_pointcloud shift {shift[0]:g}: worst |scale error| / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    # without the float64 recentring the cast alone costs orders of magnitude more than the bound
    naive = 0.5 * knn_distances(torch.tensor(x64, dtype=torch.float32, device=dev), 3).mean(dim=1).cpu().double().numpy()
    if shift[0] != 0.0:
        assert float((np.abs(naive - want) / bound).max()) > 100.0
    # everything else is the host path's, bit for bit; the means are the uncentred cast
    for name in ("quats", "sh_0", "sh_rest", "logit_opacities", "means", "BACKGROUND"):
        assert torch.equal(getattr(m, name).detach().cpu(), getattr(host, name).detach()), name
    assert torch.equal(m.means.detach().cpu(), torch.tensor(x64, dtype=torch.float32))
    assert m.active_sh_degree == host.active_sh_degree == 0 and m.MAX_SH_DEGREE == host.MAX_SH_DEGREE == 2
    assert np.allclose(got, host.scales.detach().double().numpy(), rtol=1e-5)
    # the default device is the current one
    m2 = GaussianModel.from_pointcloud(pc, sh_degree=2, sh_degree_interval=1000, knn="device", white_background=True)
    assert m2.means.device == dev and torch.equal(m2.log_scales, m.log_scales)


def test_three_eager_train_steps_on_a_device_built_model():
    from scenes import make_scene
    dev = _dev()
    W, H = 64, 48
    sc = make_scene(16, W, H, sh_degree=1, n_views=1, seed=3, dist=4.0)   # (for its camera: view 0 looks at the origin from 4 away)
    rng = np.random.default_rng(9)
    pc = S.Pointcloud(rng.random((3000, 3)) * 2.0 - 1.0, rng.integers(0, 256, (3000, 3), dtype=np.uint8))
    model = GaussianModel.from_pointcloud(pc, sh_degree=1, knn="device", device=dev, white_background=True)
    opt = build_optimizers(model, 1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2, fused="hip")
    lc = LossComputer(0.2, clamp_input=True)
    data = {"w2c": torch.from_numpy(sc["viewmats"][0]).to(dev), "K": torch.from_numpy(sc["Ks"][0]).to(dev), "width": W, "height": H}
    gt = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    before = model.log_scales.detach().clone()
    losses = []
    for _ in range(3):
        out = model(data, clamp=False)
        loss = lc.get_loss_dict(out["render_img"], gt, None)["total"]
        loss.backward()
        model.update_statistics(data, out)
        opt.step(); opt.zero_grad()
        losses.append(float(loss))
    assert all(np.isfinite(v) for v in losses), losses
    assert bool(torch.isfinite(model.log_scales).all()) and not torch.equal(model.log_scales.detach(), before)
    assert float(model.collecting_counts.sum()) > 0
