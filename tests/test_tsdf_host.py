"""The TSDF integration and the marching tetrahedra of csrc/gs_tsdf.h built with the host compiler -- the device's own text -- and
held to float64 restatements (tests/tsdf_ref.py) and to analytic surfaces: no GPU.

Integration: outside the *razor* voxels (tsdf_ref.integrate64: a pixel boundary within 1e-3 px, the truncation edge, z = 0 or
depth_max within a float32 rounding -- decided by the float64 run alone, at most 2 % of the volume) the weights agree exactly and
    |tsdf - ref| <= 8 * 2^-24 * Zmax / trunc + n_views * 2^-23,
Zmax the largest camera-space coordinate magnitude: the first term is the rounding of the fmaf chain carried through the division by
trunc, the second one rounding per running-average step, which a convex combination does not amplify.  Colour: the same bound times
the largest colour value.

Marching tetrahedra: vertex set, owners, kinds and faces (as oriented triples up to rotation, in order) equal the plain-loop
reference, whose orientation is decided geometrically; positions within 4 * 2^-24 * max|coordinate| (one division, one product, one
fmaf).  Then the topology of analytic fields on a 16^3 grid."""
import numpy as np
import pytest
import torch

import tsdf_ref as TR

SEEDS = (11, 12)


@pytest.fixture(scope="module")
def ts(tmp_path_factory):
    return TR.host_lib(tmp_path_factory.mktemp("tsdf"))


# ---- integration ----

@pytest.mark.parametrize("seed", SEEDS)
def test_integration_matches_float64_outside_the_razor_voxels(ts, seed):
    g, P = TR.GRID_A, TR.PARAMS_A
    views = TR.views_a(seed)
    pts = TR.grid_points64(g["dims"], g["origin"], g["h"])
    tsdf, weight, color = TR.fresh(g["dims"])
    t64, w64, c64 = tsdf.astype(np.float64), weight.astype(np.float64), color.astype(np.float64)
    razor, zmax, behind = np.zeros(len(pts), bool), 0.0, 0
    for view in views:
        tsdf, weight, color = TR.host_integrate(ts, g["dims"], g["origin"], g["h"], g["trunc"], view, tsdf, weight, color, **P)
        r, zm = TR.integrate64(pts, view, g["trunc"], t64, w64, c64, **P)
        razor |= r
        zmax = max(zmax, zm)
        vm = view["viewmat"].astype(np.float64)
        behind += int(((pts @ vm[2, :3] + vm[2, 3]) <= 0).sum())
    share = razor.mean()
    ok = ~razor
    bound = 8 * TR.U * zmax / g["trunc"] + len(views) * 2.0 ** -23
    cmax = max(float(v["image"][..., :3].max()) for v in views)
    err_t, err_c = np.abs(tsdf - t64)[ok].max(), np.abs(color - c64)[ok].max()
    print(f"[tsdf host] seed {seed}: razor share {share:.4f}, voxels behind a camera {behind}, touched {int((w64 > 0).sum())} / {len(pts)}, "
          f"weights at max_weight {int((w64 == P['max_weight']).sum())}, Zmax {zmax:.3f}, tsdf err {err_t:.3g} (bound {bound:.3g}), "
          f"colour err {err_c:.3g} (bound {bound * cmax:.3g})")
    assert share <= 0.02
    assert behind > 0 and (w64 > 0).sum() > len(pts) // 4 and (w64 == 0).sum() > 0   # (the case does what it is there for)
    assert 0 < ((t64 > -1) & (t64 < 1) & (w64 > 0)).sum()
    assert np.array_equal(weight[ok], w64[ok].astype(np.float32))
    assert err_t <= bound
    assert err_c <= bound * cmax


def test_untouched_voxels_keep_their_bits(ts):
    g, P = TR.GRID_A, TR.PARAMS_A
    rng = np.random.default_rng(5)
    n = int(np.prod(g["dims"]))
    tsdf, weight, color = (rng.uniform(-1, 1, n).astype(np.float32), rng.integers(0, 3, n).astype(np.float32),
                           rng.uniform(0, 1, (n, 3)).astype(np.float32))
    t1, w1, c1 = TR.host_integrate(ts, g["dims"], g["origin"], g["h"], g["trunc"], TR.blind_view_a(11), tsdf, weight, color, **P)
    assert t1.tobytes() == tsdf.tobytes() and w1.tobytes() == weight.tobytes() and c1.tobytes() == color.tobytes()
    view = TR.views_a(11)[0]
    t2, w2, c2 = TR.host_integrate(ts, g["dims"], g["origin"], g["h"], g["trunc"], view, tsdf, weight, color, **P)
    same = w2 == weight   # (a touched voxel's weight grows, or sits at max_weight = 3 > every weight here)
    assert 0 < same.sum() < n
    assert np.array_equal(t2[same].view(np.uint32), tsdf[same].view(np.uint32))
    assert np.array_equal(c2[same].view(np.uint32), color[same].view(np.uint32))


def test_grid_limits(ts):
    ok = lambda d, h=0.1: bool(ts.ts_grid_ok(np.asarray(d, np.int32).ctypes.data, h))
    assert ok((2, 2, 2)) and ok((512, 512, 512)) and ok((674, 674, 674))
    assert 7 * 675 ** 3 >= 2 ** 31 and not ok((675, 675, 675))
    assert not ok((1, 8, 8)) and not ok((8, 8, 1)) and not ok((8, 0, 8)) and not ok((-4, 8, 8))
    assert not ok((65536, 65536, 2)) and not ok((2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))
    assert not ok((8, 8, 8), 0.0) and not ok((8, 8, 8), -1.0) and not ok((8, 8, 8), float("nan"))


# ---- marching tetrahedra against the plain-loop reference ----

def _extract(ts, case, min_weight=1.0):
    return TR.host_extract(ts, case["dims"], case["origin"], case["h"], min_weight, case["tsdf"], case["weight"], case["color"])


@pytest.mark.parametrize("seed", (3, 4))
def test_marching_tetrahedra_match_the_plain_loops(ts, seed):
    case = TR.smooth_case(seed)
    got = _extract(ts, case)
    ref = TR.extract64(case["dims"], case["origin"], case["h"], 1.0, case["tsdf"], case["weight"], case["color"])
    V, F = len(ref["keys"]), len(ref["faces"])
    print(f"[mt host] seed {seed}: {V} vertices, {F} faces, unobserved corners {int((case['weight'] == 0).sum())}")
    assert V > 100 and F > 100
    assert len(got["vertices"]) == V
    assert list(zip(got["owner"].tolist(), got["kind"].tolist())) == ref["keys"]
    assert TR.rotate_min_first(got["faces"]) == TR.rotate_min_first(ref["faces"])
    tol = 4 * TR.U * np.abs(ref["vertices"]).max()
    assert np.abs(got["vertices"] - ref["vertices"]).max() <= tol
    # colour: one division, one difference, one fmaf on values in [0, 1]
    assert np.abs(got["colors"] - ref["colors"]).max() <= 4 * TR.U


# ---- analytic topology, 16^3, h = 1/15 ----

def test_sphere_is_closed_oriented_and_near_the_surface(ts):
    case = TR.field_case(TR.sphere())
    m = _extract(ts, case)
    v, f = m["vertices"].astype(np.float64), m["faces"]
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v)
    TR.assert_closed_oriented(f)
    assert TR.euler(len(v), f) == 2
    tri = v[f]
    normals = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", normals, tri.mean(1) - TR.SPHERE_C) > 0).all()
    h, r = case["h"], TR.SPHERE_R
    off = np.abs(np.linalg.norm(v - TR.SPHERE_C, axis=1) - r)
    print(f"[mt host] sphere: {len(v)} vertices, {len(f)} faces, worst distance {off.max():.3g} (bound {3 * h * h / (8 * r) + 1e-6:.3g})")
    assert off.max() <= 3 * h * h / (8 * r) + 1e-6


def test_torus_has_euler_characteristic_zero(ts):
    c, R, r = np.array([0.507, 0.493, 0.511]), 0.28, 0.13

    def torus(p):
        q = p - c
        return np.sqrt((np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - R) ** 2 + q[:, 2] ** 2) - r
    m = _extract(ts, TR.field_case(torus))
    TR.assert_closed_oriented(m["faces"])
    assert TR.euler(len(m["vertices"]), m["faces"]) == 0


def test_two_spheres_have_euler_characteristic_four(ts):
    a, b = TR.sphere((0.27, 0.31, 0.29), 0.17), TR.sphere((0.73, 0.69, 0.71), 0.17)
    m = _extract(ts, TR.field_case(lambda p: np.minimum(a(p), b(p))))
    TR.assert_closed_oriented(m["faces"])
    assert TR.euler(len(m["vertices"]), m["faces"]) == 4


def test_half_observed_sphere_stops_at_the_unobserved_half(ts):
    case = TR.field_case(TR.sphere(), observed=lambda p: p[:, 0] < 0.5)
    m = _extract(ts, case)
    f = m["faces"]
    assert len(f) > 0
    und = TR.undirected_edges(f)
    assert set(und.values()) == {1, 2}                      # an open surface: a boundary, and nothing worse
    assert all(k == 1 for k in TR.directed_edges(f).values())
    nx, ny, _ = case["dims"]
    far = m["owner"] + (m["kind"] & 1) + nx * (((m["kind"] >> 1) & 1) + ny * ((m["kind"] >> 2) & 1))
    assert (case["weight"][m["owner"]] >= 1).all() and (case["weight"][far] >= 1).all()   # every vertex: both ends observed
    assert f.min() >= 0 and f.max() < len(m["vertices"])
    assert len(np.unique(f)) == len(m["vertices"])          # no vertex unreferenced


def test_plane_through_a_layer_of_corners(ts):
    """tsdf == 0 exactly on the layer iz = 7: zero is outside, t = f0 / (f0 - f1) is 1 there.  Zero-area faces are tolerated."""
    dims, h = (16, 16, 16), np.float32(1.0 / 15.0)
    iz = np.repeat(np.arange(16), 16 * 16)
    case = dict(dims=dims, origin=(0.0, 0.0, 0.0), h=float(h), tsdf=((iz - 7).astype(np.float32) * h), weight=np.ones(16 ** 3, np.float32),
                color=None)
    assert (case["tsdf"].reshape(16, 16, 16)[7] == 0).all()
    m = _extract(ts, case)
    assert len(m["faces"]) > 0 and np.isfinite(m["vertices"]).all()
    assert m["faces"].min() >= 0 and m["faces"].max() < len(m["vertices"])
    assert np.abs(m["vertices"][:, 2] - 7 * h).max() <= 4 * TR.U


def test_no_surface_no_output(ts):
    pos = TR.field_case(lambda p: np.full(len(p), 0.5))
    assert len(_extract(ts, pos)["vertices"]) == 0 and len(_extract(ts, pos)["faces"]) == 0
    unseen = TR.field_case(TR.sphere(), observed=lambda p: np.zeros(len(p), bool))
    assert len(_extract(ts, unseen)["vertices"]) == 0 and len(_extract(ts, unseen)["faces"]) == 0


# ---- PLY ----

def test_ply_round_trip(ts, tmp_path):
    from easy_gaussian_splatting_amd import mesh
    case = TR.smooth_case(3)
    m = _extract(ts, case)
    v, f, c = torch.from_numpy(m["vertices"].copy()), torch.from_numpy(m["faces"].copy()), torch.from_numpy(m["colors"].copy())
    c[0], c[1] = torch.tensor([-0.5, 1.5, 0.5]), torch.tensor([0.0, 1.0, 0.25])   # (clamped; exact ends)
    path = tmp_path / "mesh.ply"
    mesh.save_mesh_ply(path, v, f, c)
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "property list uchar int vertex_indices" in head
    assert head[2] == f"element vertex {len(v)}" and "property uchar red" in head
    v2, f2, c2 = mesh.load_mesh_ply(path)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32
    assert v2.numpy().tobytes() == v.numpy().tobytes() and f2.numpy().tobytes() == f.numpy().tobytes()
    assert (c2 - c.clamp(0, 1)).abs().max() <= 0.5 / 255 + 1e-7
    assert c2[0].tolist() == [0.0, 1.0, pytest.approx(128 / 255)]
    mesh.save_mesh_ply(path, v, f)   # without colours
    v3, f3, c3 = mesh.load_mesh_ply(path)
    assert c3 is None and v3.numpy().tobytes() == v.numpy().tobytes() and f3.numpy().tobytes() == f.numpy().tobytes()
    empty = (torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32))
    mesh.save_mesh_ply(path, *empty)
    v4, f4, _ = mesh.load_mesh_ply(path)
    assert v4.shape == (0, 3) and f4.shape == (0, 3)
