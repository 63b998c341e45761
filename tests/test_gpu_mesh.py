"""The device mesh extraction (csrc/gs_tsdf.hip through easy_gaussian_splatting_amd/mesh.py) against tests/hostmath/tsdf.cpp, the
host build of csrc/gs_tsdf.h -- the device's own text: the integrated volume, the vertices, their colours and the faces must match
it BIT FOR BIT (the host build itself is held to float64 and to analytic surfaces by tests/test_tsdf_host.py).

Shapes: the 24 x 20 x 17 volume under 37 x 29 views of the host test (no dimension a multiple of the 64 x 4 block, a camera inside the
volume, holes of every kind); extraction from the 9 x 8 x 7 smooth field with unobserved corners, the 16^3 sphere, and a 33 x 17 x 2
volume -- one dimension at its minimum, none a multiple of the block shape, two blocks along y.  Then the refusals, and a model of
20 000 Gaussians on a sphere through extract_mesh."""
import ctypes as ct
import math
import types

import numpy as np
import pytest
import torch

import tsdf_ref as TR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import mesh

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ts(tmp_path_factory):
    return TR.host_lib(tmp_path_factory.mktemp("tsdf"))


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape} words"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} words differ from the host build, first at {bad[0]}: {g[bad[0]]:#x} vs {w[bad[0]]:#x}"


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("depth_only", (False, True))
def test_integrate_is_the_host_build_bit_for_bit(ts, depth_only):
    dev, g, P = _dev(), TR.GRID_A, dict(TR.PARAMS_A)
    views = TR.views_a(11)
    if depth_only:   # a [H, W, 1] depth image into a volume without colour
        views = [dict(v, image=np.ascontiguousarray(v["image"][..., 3:4])) for v in views]
        P.update(depth_channel=0, color_channel=-1)
    vol = mesh.TSDFVolume(g["origin"], g["h"], g["dims"], trunc=g["trunc"], color=not depth_only, device=dev)
    assert tuple(vol.tsdf.shape) == g["dims"][::-1] and (vol.color is None) == depth_only
    tsdf, weight, color = TR.fresh(g["dims"], color=not depth_only)
    _same_bits(vol.tsdf, tsdf, "fresh tsdf")
    _same_bits(vol.weight, weight, "fresh weight")
    kw = dict(min_alpha=P["min_alpha"], depth_max=P["depth_max"], max_weight=P["max_weight"])
    kw.update(dict(color_channels=None) if depth_only else dict(depth_channel=3, color_channels=(0, 1, 2)))

    def fold(view):
        vol.integrate(_t(view["image"], dev), _t(view["viewmat"], dev), _t(view["K"], dev), alphas=_t(view["alphas"], dev), **kw)

    for i, view in enumerate(views):
        fold(view)
        tsdf, weight, color = TR.host_integrate(ts, g["dims"], g["origin"], g["h"], g["trunc"], view, tsdf, weight, color, **P)
        _same_bits(vol.tsdf, tsdf, f"tsdf after view {i}")
        _same_bits(vol.weight, weight, f"weight after view {i}")
        if not depth_only:
            _same_bits(vol.color, color, f"color after view {i}")
    assert (weight > 0).sum() > weight.size // 4
    blind = TR.blind_view_a(11)   # a view that sees nothing of the volume: every bit stays
    if depth_only:
        blind = dict(blind, image=np.ascontiguousarray(blind["image"][..., 3:4]))
    fold(blind)
    _same_bits(vol.tsdf, tsdf, "tsdf after the blind view")
    _same_bits(vol.weight, weight, "weight after the blind view")
    if not depth_only:
        _same_bits(vol.color, color, "color after the blind view")


CASES = {
    "smooth_9x8x7": lambda: TR.smooth_case(3),
    "sphere_16": lambda: TR.field_case(TR.sphere()),
    "thin_33x17x2": lambda: TR.smooth_case(8, dims=(33, 17, 2), unobserved=0.05),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_extract_is_the_host_build_bit_for_bit(ts, name):
    dev, case = _dev(), CASES[name]()
    nx, ny, nz = case["dims"]
    vol = mesh.TSDFVolume(case["origin"], case["h"], case["dims"], color=case["color"] is not None, device=dev)
    vol.tsdf.copy_(_t(case["tsdf"], dev).reshape(nz, ny, nx))
    vol.weight.copy_(_t(case["weight"], dev).reshape(nz, ny, nx))
    if case["color"] is not None:
        vol.color.copy_(_t(case["color"], dev).reshape(nz, ny, nx, 3))
    want = TR.host_extract(ts, case["dims"], case["origin"], case["h"], 1.0, case["tsdf"], case["weight"], case["color"])
    assert len(want["faces"]) > 20, "the case has a surface"
    v, f, c = vol.extract(min_weight=1.0)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and tuple(v.shape) == want["vertices"].shape and tuple(f.shape) == want["faces"].shape
    _same_bits(v, want["vertices"], "vertices")
    _same_bits(f, want["faces"], "faces")
    if case["color"] is None:
        assert c is None
    else:
        _same_bits(c, want["colors"], "colors")
    v2, f2, c2 = vol.extract(min_weight=1.0)   # no atomics: the same bits again
    _same_bits(v2, v, "vertices, second run")
    _same_bits(f2, f, "faces, second run")
    if c is not None:
        _same_bits(c2, c, "colors, second run")
    _same_bits(vol.tsdf, case["tsdf"], "the volume is read only")


def test_empty_surface_returns_empty_tensors():
    vol = mesh.TSDFVolume((0, 0, 0), 0.1, (5, 4, 3), device=_dev())
    v, f, c = vol.extract()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3)
    vol.tsdf.fill_(-1.0)   # a surface between unobserved corners is none either
    v, f, c = vol.extract()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_refusals():
    dev, L = _dev(), nat.lib()
    # beyond 7 nx ny nz < 2^31: through dims alone, against the C entries' own argument check; nothing is allocated or launched
    big = (ct.c_int32 * 3)(675, 675, 675)
    origin = (ct.c_float * 3)(0, 0, 0)
    assert 7 * 675 ** 3 >= 2 ** 31 and int(L.gs_mt_scan_workspace_ints(big)) == 0
    assert int(L.gs_mt_scan_workspace_ints((ct.c_int32 * 3)(674, 674, 674))) > 0
    assert L.gs_tsdf_integrate(None, big, origin, 0.1, 0.4, math.inf, 0.5, math.inf, None, None, 8, 8, None, 4, 3, 0, None, None, None, None) == nat.GS_ERR_ARG
    assert L.gs_mt_flags(None, big, 1.0, None, None, None, None, None, None, None, None) == nat.GS_ERR_ARG
    assert L.gs_mt_vertices(None, big, origin, 0.1, None, None, None, None, 0, None, None) == nat.GS_ERR_ARG
    assert L.gs_mt_faces(None, big, None, None, None, None, 0, 0, None) == nat.GS_ERR_ARG
    for dims in ((675, 675, 675), (1, 8, 8), (8, 8, 1), (2 ** 16, 2 ** 16, 2)):
        with pytest.raises(ValueError):
            mesh.check_dims(dims)
        with pytest.raises(ValueError):
            mesh.TSDFVolume((0, 0, 0), 0.1, dims, device=dev)
    # min_weight <= 0
    small = (ct.c_int32 * 3)(4, 4, 4)
    assert L.gs_mt_flags(None, small, 0.0, None, None, None, None, None, None, None, None) == nat.GS_ERR_ARG
    vol = mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device=dev)
    for mw in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            vol.extract(min_weight=mw)
    # CPU tensors
    with pytest.raises(NotImplementedError):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    eye, K = torch.eye(4, device=dev), torch.eye(3, device=dev)
    with pytest.raises(NotImplementedError):
        vol.integrate(torch.ones((8, 8, 4)), eye, K)
    with pytest.raises(NotImplementedError):
        vol.integrate(torch.ones((8, 8, 4), device=dev), eye.cpu(), K)
    cpu_model = types.SimpleNamespace(means=torch.zeros((4, 3)))
    with pytest.raises(NotImplementedError):
        mesh.extract_mesh(cpu_model, [])
    # non-pinhole cameras
    gpu_model = types.SimpleNamespace(means=torch.zeros((4, 3), device=dev))
    for cm in ("fisheye", "ortho"):
        view = dict(camera_model=cm, w2c=eye, K=K, width=8, height=8)
        with pytest.raises(NotImplementedError):
            mesh.fuse_model(gpu_model, [view], vol)
        with pytest.raises(NotImplementedError):
            mesh.extract_mesh(gpu_model, [view], bounds=((0, 0, 0), (1, 1, 1)), resolution=4)
    # argument errors of integrate
    with pytest.raises(ValueError):
        vol.integrate(torch.ones((8, 8, 4), device=dev), eye, K, color_channels=(0, 2, 3))
    with pytest.raises(ValueError):
        vol.integrate(torch.ones((8, 8, 4), device=dev), eye, K, depth_channel=4)
    _same_bits(vol.weight, np.zeros(64, np.float32), "a refused call touches nothing")


def test_model_on_a_sphere_end_to_end():
    """20 000 small opaque Gaussians on a sphere, 12 pinhole views at 96 x 96, a 40^3 volume: extract_mesh equals the chain written
    out by hand bit for bit.  Printed, not asserted: how far the vertices lie from the sphere, in voxels -- that depends on how the
    expected depth behaves on thin splats."""
    from easy_gaussian_splatting_amd.model import GaussianModel
    from easy_gaussian_splatting_amd.rendering import rasterization
    dev = _dev()
    gen = torch.Generator().manual_seed(2)
    n, r, c = 20000, 0.5, torch.tensor([0.02, -0.01, 0.03])
    d = torch.nn.functional.normalize(torch.randn((n, 3), generator=gen), dim=1)
    rgb = 0.5 + 0.4 * d
    quats = torch.zeros((n, 4))
    quats[:, 0] = 1.0
    model = GaussianModel(means=c + r * d, log_scales=torch.full((n, 3), math.log(0.01)), quats=quats,
                          sh_0=((rgb - 0.5) / 0.28209479177387814)[:, None, :].contiguous(), sh_rest=torch.zeros((n, 3, 3)),
                          logit_opacities=torch.full((n,), 4.0), sh_degree=1).to(dev)
    W = H = 96
    K = torch.tensor([[100.0, 0, 48.0], [0, 100.0, 48.0], [0, 0, 1]], device=dev)
    views = []
    for i in range(12):
        az, el = 2 * math.pi * i / 12, (-0.9, 0.1, 0.8)[i % 3]
        eye = np.asarray(c) + 1.8 * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])
        views.append(dict(w2c=_t(TR.look_at(eye, np.asarray(c)), dev), K=K, width=W, height=H))
    lo, hi = [float(v) - 0.7 for v in c], [float(v) + 0.7 for v in c]
    v, f, col = mesh.extract_mesh(model, views, bounds=(lo, hi), resolution=40)

    vol = mesh.TSDFVolume.from_bounds(lo, hi, 40, device=dev)
    assert vol.dims == (40, 40, 40)
    with torch.no_grad():
        for data in views:
            img, alphas, _ = rasterization(
                means=model.means, quats=model.quats, scales=model.log_scales, opacities=model.logit_opacities,
                colors=(model.sh_0, model.sh_rest), sh_degree=model.active_sh_degree, viewmats=data["w2c"][None], Ks=data["K"][None],
                width=W, height=H, backgrounds=model.BACKGROUND[None], packed=False, render_mode="RGB+ED", _tile_culling="tight",
                _activations="exp_sigmoid")
            assert tuple(img.shape) == (1, H, W, 4)
            vol.integrate(img[0], data["w2c"], data["K"], depth_channel=3, color_channels=(0, 1, 2), alphas=alphas[0], min_alpha=0.5)
    v2, f2, col2 = vol.extract(min_weight=1.0)
    _same_bits(v, v2, "vertices")
    _same_bits(f, f2, "faces")
    _same_bits(col, col2, "colors")
    assert v.shape[0] > 1000 and f.shape[0] > 1000
    (blo, bhi), vc = vol.bounds, v.cpu().double()
    assert all(float(vc[:, a].min()) >= blo[a] - 1e-5 and float(vc[:, a].max()) <= bhi[a] + 1e-5 for a in range(3))
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    off = ((vc - c.double()).norm(dim=1) - r).abs() / vol.voxel_size
    print(f"[mesh e2e] {v.shape[0]} vertices, {f.shape[0]} faces; | |v - c| - r | in voxels: median {float(off.median()):.3f}, "
          f"max {float(off.max()):.3f} (voxel {vol.voxel_size:.4f}, trunc {vol.trunc:.4f})")
