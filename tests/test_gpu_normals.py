"""The normal-consistency kernels (csrc/gs_normals.hip through easy_gaussian_splatting_amd/normals.py) against tests/hostmath/normals.cpp,
the host build of csrc/gs_normals.h -- the device's own text: the Gaussian normals, the depth-normal image, v_quats and v_render4 must
match it BIT FOR BIT, and the value must lie within the float64 reference's bound (the host build itself is held to float64 and to
analytic surfaces by tests/test_normals_host.py).

Shapes: N in {1, 63, 64, 65, 257} under 1 and 2 cameras; frames that are no multiple of the 64 x 8 tile (37 x 53), the smallest frame
with an interior pixel (3 x 3), frames without one (H = 2, W = 1), a width of one tile + 1 (65) and of two tiles - 1 (127), a frame
whose only valid pixels sit on tile borders and corners, frames with alpha holes and with a mask.  Output buffers are poisoned first.
Then the whole path on a small scene against the plain-torch expression, a plane of flat Gaussians, and the refusals."""
import types

import numpy as np
import pytest
import torch

import normals_ref as NR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import normals as NM

pytestmark = pytest.mark.gpu
GRAD_RTOL = 1e-3   # the project's bound on a gradient tensor (tests/test_gpu_depth.py): of the largest reference magnitude
SENTINEL = -7.25


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nm(tmp_path_factory):
    return NR.host_lib(tmp_path_factory.mktemp("normals"))


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


def test_the_reference_knows_the_tile():
    assert (nat.GS_NORMAL_TILE_W, nat.GS_NORMAL_TILE_H) == (NR.TILE_W, NR.TILE_H)


# ---- the per-Gaussian kernels ----

@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 257))
def test_gaussian_normals_and_v_quats_are_the_host_build_bit_for_bit(nm, N, C):
    dev = _dev()
    case = NR.gauss_case(N, C, 100 + N + C)
    v = np.random.default_rng(N).normal(size=(C, N, 3)).astype(np.float32)
    L = nat.lib()
    m, q, s, vm, vt = [_t(case[k], dev) for k in ("means", "quats", "scales", "viewmats")] + [_t(v, dev)]
    out = torch.full((C * N * 3 + 8,), SENTINEL, device=dev)      # (a canary behind each output)
    vq = torch.full((N * 4 + 8,), SENTINEL, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.check(L.gs_gauss_normals_fwd(st, N, C, m.data_ptr(), q.data_ptr(), s.data_ptr(), vm.data_ptr(), out.data_ptr()), "fwd")
    nat.check(L.gs_gauss_normals_bwd(st, N, C, m.data_ptr(), q.data_ptr(), s.data_ptr(), vm.data_ptr(), vt.data_ptr(), vq.data_ptr()), "bwd")
    torch.cuda.synchronize()
    _same_bits(out[:C * N * 3], NR.host_gauss_fwd(nm, case), "normals")
    _same_bits(vq[:N * 4], NR.host_gauss_bwd(nm, case, v), "v_quats")
    assert (out[C * N * 3:] == SENTINEL).all() and (vq[N * 4:] == SENTINEL).all()
    # the autograd wrapper: the same bits, gradients to the quaternions alone
    qq = q.clone().requires_grad_(True)
    mm, ss = m.clone().requires_grad_(True), s.clone().requires_grad_(True)
    n = NM.gaussian_normals(mm, qq, ss, vm)
    (n * vt).sum().backward()
    _same_bits(n, out[:C * N * 3], "gaussian_normals")
    _same_bits(qq.grad, vq[:N * 4], "gaussian_normals backward")
    assert mm.grad is None and ss.grad is None


# ---- the image kernels ----

def _frames():
    return {
        "37x53": NR.frame_case(37, 53, 31),
        "3x3": NR.frame_case(3, 3, 32, holes=False, bad_depths=False, mask=False),
        "H2": NR.frame_case(2, 70, 35),
        "W1": NR.frame_case(20, 1, 36),
        "tile+1": NR.frame_case(9, 65, 33),
        "2tiles-1": NR.frame_case(17, 127, 34),
        "borders": NR.border_case(24, 130, 61),
        "holes": NR.frame_case(40, 140, 37, mask=False),
        "mask": NR.frame_case(16, 64, 38, holes=False, bad_depths=False),
    }


FRAME_NAMES = ("37x53", "3x3", "H2", "W1", "tile+1", "2tiles-1", "borders", "holes", "mask")


@pytest.fixture(scope="module")
def frames():
    return _frames()


def _device_loss(frame, dev, *, detach_depth=False, v_loss=0.7):
    """value, depth normals and v_render4 from the kernels, outputs poisoned first"""
    L = nat.lib()
    r, a, K = _t(frame["render4"], dev), _t(frame["alphas"], dev), _t(frame["K"], dev)
    mask = None if frame.get("mask") is None else _t(frame["mask"], dev)
    H, W, _ = r.shape
    rec = torch.full((nat.GS_NORMAL_REC_FLOATS,), SENTINEL, device=dev)
    n_part = int(L.gs_normal_loss_partials_doubles(H, W))
    assert n_part == 2 * ((W + NR.TILE_W - 1) // NR.TILE_W) * ((H + NR.TILE_H - 1) // NR.TILE_H)
    partials = torch.full((n_part,), float("nan"), dtype=torch.float64, device=dev)
    dn = torch.full((H * W * 3 + 8,), SENTINEL, device=dev)
    vr = torch.full((H * W * 4 + 8,), SENTINEL, device=dev)
    v = torch.tensor([v_loss], dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    mp = None if mask is None else mask.data_ptr()
    nat.check(L.gs_normal_loss_fwd(st, H, W, K.data_ptr(), frame["min_alpha"], r.data_ptr(), a.data_ptr(), mp, rec.data_ptr(),
                                   partials.data_ptr(), dn.data_ptr()), "gs_normal_loss_fwd")
    nat.check(L.gs_normal_loss_bwd(st, H, W, K.data_ptr(), frame["min_alpha"], int(detach_depth), r.data_ptr(), a.data_ptr(), mp, rec.data_ptr(),
                                   v.data_ptr(), vr.data_ptr()), "gs_normal_loss_bwd")
    torch.cuda.synchronize()
    assert (dn[H * W * 3:] == SENTINEL).all() and (vr[H * W * 4:] == SENTINEL).all()
    return dict(value=rec[0].cpu().numpy(), inv_w=rec[1].cpu().numpy(), depth_normals=dn[:H * W * 3].view(H, W, 3), v_render4=vr[:H * W * 4].view(H, W, 4),
                partials=partials.cpu().numpy())


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_image_kernels_are_the_host_build_bit_for_bit(nm, frames, name):
    dev, frame = _dev(), frames[name]
    host = NR.host_loss(nm, frame, v_loss=0.7)
    ref = NR.loss64(frame, v_loss=0.7)
    got = _device_loss(frame, dev)
    H, W, _ = frame["render4"].shape
    print(f"[normals gpu] {name} {H}x{W}: {int(ref['valid'].sum())} valid, counted {ref['w'].sum():.0f}, value {float(got['value']):.7f} "
          f"(host {float(host['value']):.7f}, float64 {ref['value']:.7f}, bound {ref['value_bound']:.3g})")
    _same_bits(got["depth_normals"], host["depth_normals"], "depth normals")       # (every element written: the sentinel is gone)
    _same_bits(got["inv_w"], host["inv_w"], "1 / sum(w)")
    _same_bits(got["v_render4"], host["v_render4"], "v_render4")
    assert np.isfinite(got["partials"]).all() and got["partials"][1::2].sum() == ref["w"].sum()
    assert abs(float(got["value"]) - ref["value"]) <= ref["value_bound"]
    if name in ("H2", "W1"):
        assert ref["valid"].sum() == 0 and not _bits(got["value"]).any() and not _bits(got["v_render4"]).any()
    else:
        assert ref["w"].sum() > 0 and got["v_render4"][..., 3].abs().max() > 0
    if name == "borders":
        y, x = np.nonzero(ref["valid"])
        assert ((x % NR.TILE_W == 0) | (x % NR.TILE_W == NR.TILE_W - 1) | (y % NR.TILE_H == 0) | (y % NR.TILE_H == NR.TILE_H - 1)).all() and len(y) > 20
    if name == "holes":
        with np.errstate(invalid="ignore"):
            own = (frame["alphas"] >= 0.5) & np.isfinite(frame["render4"][..., 3]) & (frame["render4"][..., 3] > 0)
        assert 0 < ref["valid"].sum() < own[1:-1, 1:-1].sum() - 100    # the 5-pixel stencil decides: usable centres next to a hole
    if name == "mask":
        assert ref["w"].sum() < ref["valid"].sum()


@pytest.mark.parametrize("name", ("37x53", "borders"))
def test_detached_depth_writes_zeros_and_keeps_the_normal_channels(nm, frames, name):
    dev, frame = _dev(), frames[name]
    a, b = _device_loss(frame, dev), _device_loss(frame, dev, detach_depth=True)
    _same_bits(b["v_render4"], NR.host_loss(nm, frame, detach_depth=True, v_loss=0.7)["v_render4"], "v_render4 (detached)")
    assert not _bits(b["v_render4"][..., 3].contiguous()).any()
    _same_bits(b["v_render4"][..., :3].contiguous(), a["v_render4"][..., :3].contiguous(), "normal channels")
    assert a["v_render4"][..., 3].abs().max() > 0


def test_frames_with_no_valid_pixel_give_exact_zeros(frames):
    dev = _dev()
    base = frames["37x53"]
    cases = {"alpha": dict(base, alphas=np.minimum(base["alphas"], np.float32(0.49))), "mask": dict(base, mask=np.ones((37, 53), np.float32)),
             "H2": frames["H2"]}
    for name, frame in cases.items():
        got = _device_loss(frame, dev)
        assert not _bits(got["value"]).any() and not _bits(got["inv_w"]).any() and not _bits(got["v_render4"]).any(), name
        r = _t(frame["render4"], dev).requires_grad_(True)
        loss = NM.normal_consistency_loss(r, _t(frame["alphas"], dev), _t(frame["K"], dev), mask=_t(frame["mask"], dev))
        loss.backward()
        assert float(loss.detach()) == 0.0 and not _bits(r.grad).any(), name


def test_python_surface_matches_the_kernels(nm, frames):
    dev, frame = _dev(), frames["37x53"]
    host = NR.host_loss(nm, frame, v_loss=1.0)
    r = _t(frame["render4"], dev).requires_grad_(True)
    a, K, m = _t(frame["alphas"], dev), _t(frame["K"], dev), _t(frame["mask"], dev)
    loss = NM.normal_consistency_loss(r, a, K, mask=m)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    _same_bits(r.grad, host["v_render4"], "autograd v_render4")
    assert abs(float(loss.detach()) - float(host["value"])) <= 2 * NR.loss64(frame)["value_bound"]
    dn = NM.depth_to_normal(r.detach()[..., 3], a, K)
    _same_bits(dn, host["depth_normals"], "depth_to_normal")
    dn1 = NM.depth_to_normal(r.detach()[..., 3:], a[..., None], K)
    assert torch.equal(dn, dn1)
    # a [H, W, 4] view at an address that is not 16-byte aligned is copied, not refused
    buf = torch.zeros((37 * 53 * 4 + 1,), device=dev)
    buf[1:] = r.detach().reshape(-1)
    odd = buf[1:].view(37, 53, 4)
    assert float(NM.normal_consistency_loss(odd, a, K, mask=m)) == float(loss.detach())


# ---- end to end ----

def _model(sc, dev):
    from easy_gaussian_splatting_amd.model import GaussianModel
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    return GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=T(sc["shs"][:, :1].copy()),
                         sh_rest=T(sc["shs"][:, 1:].copy()), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                         white_background=False).to(dev)


def test_end_to_end_against_the_torch_expression():
    """render_normals + normal_consistency_loss(fused=True) + backward against the same render followed by the fused=False torch
    expression in float32: gradients within GRAD_RTOL of the largest reference magnitude.  Values: the fused one within the derived
    bound of the float64 evaluation of the expression on the same render; the float32 torch value within that bound plus its own --
    the same per-pixel analysis once more, and a float32 tree sum of n terms (at most ceil(log2 n) + 16 roundings, 16 for the
    elements a thread adds serially) over both sums."""
    from scenes import make_scene
    dev = _dev()
    W, H = 64, 48
    sc = make_scene(600, W, H, sh_degree=3, n_views=1, seed=5, scale_range=(0.08, 0.3), dist=4.0)
    sc["opacities"] = np.clip(sc["opacities"] * 0 + 0.8, 0, 1).astype(np.float32)
    m = _model(sc, dev)
    data = {"w2c": _t(sc["viewmats"][0], dev), "K": _t(sc["Ks"][0], dev), "width": W, "height": H}
    names = ("means", "quats", "log_scales", "logit_opacities")

    def run(fused):
        for k in m.param_names:
            getattr(m, k).grad = None
        out = NM.render_normals(m, data)
        assert tuple(out["render4"].shape) == (H, W, 4) and tuple(out["alphas"].shape) == (H, W)
        assert out["normals"].data_ptr() == out["render4"].data_ptr() and tuple(out["depth"].shape) == (H, W)
        loss = NM.normal_consistency_loss(out["render4"], out["alphas"], data["K"], fused=fused)
        loss.backward()
        return float(loss.detach()), {k: getattr(m, k).grad.clone() for k in names}, out

    v_f, g_f, out = run(True)
    v_t, g_t, out_t = run(False)
    assert torch.equal(out["render4"], out_t["render4"])
    frame = dict(render4=out["render4"].detach().cpu().numpy(), alphas=out["alphas"].detach().cpu().numpy(), K=sc["Ks"][0], mask=None, min_alpha=0.5)
    ref = NR.loss64(frame)
    n_valid = int(ref["valid"].sum())
    tree = 2 * (int(np.ceil(np.log2(max(2, n_valid)))) + 16) * NR.U * (abs(ref["value"]) + 1.0)
    print(f"[normals gpu] end to end: {n_valid} valid pixels of {H * W}, fused {v_f:.7f}, torch {v_t:.7f}, float64 {ref['value']:.7f}, bound {ref['value_bound']:.3g}, "
          f"torch's own {ref['value_bound'] + tree:.3g}")
    assert n_valid > 300
    assert abs(v_f - ref["value"]) <= ref["value_bound"]
    assert abs(v_f - v_t) <= 2 * ref["value_bound"] + tree
    for k in names:
        rel = float((g_f[k] - g_t[k]).abs().max()) / float(g_t[k].abs().max())
        print(f"[normals gpu]   {k}: |grad| up to {float(g_t[k].abs().max()):.3g}, rel err {rel:.3g}")
        assert float(g_t[k].abs().max()) > 0 and rel <= GRAD_RTOL, (k, rel)


def _plane_model(dev, quat):
    """Flat Gaussians (one scale 100 times smaller) on the plane z = 3 facing a camera at the origin, one per 0.1 x 0.1 cell, opacity 0.99"""
    xs, ys = np.arange(-2.0, 2.0001, 0.1), np.arange(-1.6, 1.6001, 0.1)
    gx, gy = np.meshgrid(xs, ys)
    N = gx.size
    means = np.stack([gx.ravel(), gy.ravel(), np.full(N, 3.0)], 1).astype(np.float32)
    log_scales = np.log(np.tile(np.array([0.1, 0.1, 0.001], np.float32), (N, 1)))
    quats = np.tile(np.asarray(quat, np.float32), (N, 1))
    return types.SimpleNamespace(means=_t(means, dev).requires_grad_(True), quats=_t(quats, dev).requires_grad_(True),
                                 log_scales=_t(log_scales, dev).requires_grad_(True),
                                 logit_opacities=torch.full((N,), float(np.log(0.99 / 0.01)), device=dev).requires_grad_(True))


def test_flat_gaussians_on_a_plane_are_consistent_until_they_are_rotated():
    """A plane's central differences are exact up to rounding and |Nb| there is alpha: loss = mean(1 - alpha) < 1e-3 with opacity 0.99
    under several overlapping Gaussians.  Rotated by 30 degrees about x, the blended normal tilts while the depth stays the plane's:
    the loss rises by alpha (1 - cos 30) = 0.13."""
    dev = _dev()
    W, H = 64, 48
    data = {"w2c": torch.eye(4, device=dev), "K": torch.tensor([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]], device=dev), "width": W, "height": H}
    values = []
    for quat in ((1.0, 0.0, 0.0, 0.0), (np.cos(np.pi / 12), np.sin(np.pi / 12), 0.0, 0.0)):
        out = NM.render_normals(_plane_model(dev, quat), data)
        loss = NM.normal_consistency_loss(out["render4"], out["alphas"], data["K"])
        frame = dict(render4=out["render4"].detach().cpu().numpy(), alphas=out["alphas"].detach().cpu().numpy(), K=data["K"].cpu().numpy(), mask=None,
                     min_alpha=0.5)
        ref = NR.loss64(frame)
        torch_value = float(NM.normal_consistency_loss(out["render4"].detach().double(), out["alphas"].detach().double(), data["K"].double(), fused=False))
        loss = loss.detach()
        print(f"[normals gpu] plane, quat {tuple(round(float(q), 4) for q in quat)}: loss {float(loss):.6f}, float64 {ref['value']:.6f}, valid {int(ref['valid'].sum())}, "
              f"alpha in [{frame['alphas'].min():.5f}, {frame['alphas'].max():.5f}], depth in [{frame['render4'][..., 3].min():.6f}, {frame['render4'][..., 3].max():.6f}]")
        assert ref["valid"].sum() == (H - 2) * (W - 2)
        assert abs(torch_value - ref["value"]) <= 1e-12 and abs(float(loss) - ref["value"]) <= ref["value_bound"]
        values.append((float(loss), ref["value"]))
    assert values[0][0] < 1e-3 and values[0][1] < 1e-3
    assert values[1][0] - values[0][0] > 0.1 and values[1][1] - values[0][1] > 0.1


# ---- refusals ----

def test_refusals(frames):
    dev, frame = _dev(), frames["37x53"]
    r, a, K = torch.from_numpy(frame["render4"]), torch.from_numpy(frame["alphas"]), torch.from_numpy(frame["K"])
    with pytest.raises(ValueError, match="HIP device"):
        NM.normal_consistency_loss(r, a, K, fused=True)                                      # CPU tensors
    with pytest.raises(ValueError, match="float32"):
        NM.normal_consistency_loss(r.to(dev).double(), a.to(dev), K.to(dev))
    with pytest.raises(ValueError):
        NM.normal_consistency_loss(r.to(dev)[..., :3], a.to(dev), K.to(dev))
    with pytest.raises(ValueError):
        NM.normal_consistency_loss(r.to(dev), a, K.to(dev))                                   # alphas on another device
    model = _plane_model(dev, (1.0, 0.0, 0.0, 0.0))
    data = {"w2c": torch.eye(4, device=dev), "K": K.to(dev), "width": 53, "height": 37}
    for cm in ("fisheye", "ortho"):
        with pytest.raises(NotImplementedError, match="camera_model"):
            NM.render_normals(model, dict(data, camera_model=cm))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        NM.render_normals(model, dict(data, w2c=torch.eye(4, device=dev).requires_grad_(True)))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        NM.gaussian_normals(model.means, model.quats, model.log_scales, torch.eye(4, device=dev)[None].requires_grad_(True))
    L = nat.lib()
    assert L.gs_normal_loss_partials_doubles(0, 5) == 0 and L.gs_normal_loss_partials_doubles(32768, 16384) == 0
    with pytest.raises(ValueError, match="2\\^31"):                                          # beyond the 32-bit offsets: before any launch
        nat.check(L.gs_normal_loss_fwd(None, 32768, 16384, 16, 0.5, 16, 16, None, 16, 16, None), "gs_normal_loss_fwd")
    with pytest.raises(ValueError, match="2\\^31"):
        nat.check(L.gs_normal_loss_bwd(None, 32768, 16384, 16, 0.5, 0, 16, 16, None, 16, 16, 32), "gs_normal_loss_bwd")
