"""Colour features of 1, 2 and 4 channels on the GPU (gs_rec_colors, gs_blend_fwd_ch / gs_blend_bwd_ch, gs_channel_grads):
forward and gradient parity against the float64 torch oracle, bitwise consistency with the RGB path, depth as a channel, depth
rounds and the walk re-run.  Bounds as tests/test_gpu_parity.py: 1e-4 abs on images outside the razor pixels (those within 1e-4 of
a blend discontinuity, oracle.c_oracle.blend_margin), gradients 1e-3 of each tensor's largest reference magnitude with the upstream
gradient zeroed on razor pixels."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import torch_oracle as TO
from scenes import config_bench_1m, make_scene

pytestmark = pytest.mark.gpu
FWD_ATOL = 1e-4
GRAD_RTOL = 1e-3
NAMES = ("means", "quats", "scales", "opacities")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _scene(C, seed, n=1500, W=100, H=80):
    return make_scene(n, W, H, sh_degree=0, n_views=C, seed=seed, scale_range=(0.02, 0.2), dist=4.0)


def _razor(sc):
    """[C,H,W] pixels within 1e-4 of a blend discontinuity; the contributor sets do not depend on the colours."""
    fw = CO.render(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["shs"][:, 0], sc["viewmats"], sc["Ks"],
                   int(sc["width"]), int(sc["height"]), sh_degree=None, dtype=np.float64)
    return CO.blend_margin(fw, mu_tol_ulps=1.0, conic_rtol=2.4e-7) < 1e-4


def hip(sc, colors, bg=None, grad=True, vc=None, va=None, rounds=None, culling="gsplat"):
    """rasterization() on the GPU; colors / bg / vc / va as torch tensors (moved to the device).  Returns (img, alpha, meta,
    {name: grad})."""
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = dev()
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(d) for k in NAMES + ("viewmats", "Ks")}
    ins = [t[k].clone().requires_grad_(grad) for k in NAMES]
    col = colors.detach().to(d).float().contiguous().requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        img, alpha, meta = rasterization(*ins, col, t["viewmats"], t["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=None,
                                         packed=False, backgrounds=None if bg is None else bg.to(d).float(), absgrad=True,
                                         _rounds=rounds, _tile_culling=culling)
    g = {}
    if grad:
        loss = (img * vc.to(d).float()).sum() + (0.0 if va is None else (alpha * va.to(d).float()).sum())
        gs = torch.autograd.grad(loss, ins + [col])
        g = dict(zip(NAMES + ("colors",), gs))
        g["absgrad"] = meta["means2d"].absgrad
    torch.cuda.synchronize()
    return img.detach(), alpha.detach(), meta, g


def oracle(sc, colors_fn, bg, vc, va):
    """float64 torch oracle; colors_fn(means, quats, scales, viewmats, Ks) -> colours (may depend on the geometry)."""
    T = {k: torch.from_numpy(np.asarray(sc[k], dtype=np.float64)) for k in NAMES + ("viewmats", "Ks")}
    ins = [T[k].clone().requires_grad_(True) for k in NAMES]
    col = colors_fn(*ins[:3], T["viewmats"], T["Ks"])
    if not col.requires_grad:
        col = col.clone().requires_grad_(True)
    col.retain_grad()
    img, alpha, meta = TO.rasterization(*ins, col, T["viewmats"], T["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=None,
                                        packed=False, backgrounds=bg, absgrad=True)
    loss = (img * vc).sum() + (alpha * va).sum()
    loss.backward()
    g = {k: x.grad for k, x in zip(NAMES, ins)}
    g["colors"] = col.grad
    g["absgrad"] = meta["means2d"].absgrad
    return img.detach(), alpha.detach(), g


def _check_fwd(img, alpha, ref_img, ref_alpha, razor):
    keep = torch.from_numpy(~razor)
    e_c = (img.cpu().double() - ref_img).abs().amax(-1)[keep].max().item()
    e_a = (alpha.cpu().double() - ref_alpha)[..., 0].abs()[keep].max().item()
    assert e_c <= FWD_ATOL and e_a <= FWD_ATOL, (e_c, e_a)


def _check_grad(name, got, ref):
    ref = ref.double()
    rel = ((got.cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30)).item()
    assert rel <= GRAD_RTOL, (name, rel)


def _upstream(sc, D, razor, seed):
    g = torch.Generator().manual_seed(seed)
    C, H, W = razor.shape
    keep = torch.from_numpy(~razor).double()[..., None]
    vc = torch.randn((C, H, W, D), generator=g, dtype=torch.float64) * keep
    va = torch.randn((C, H, W, 1), generator=g, dtype=torch.float64) * keep
    return vc, va


CASES = [(D, per_cam, use_bg, C) for D in (1, 2, 4) for (per_cam, use_bg, C) in
         ((False, False, 1), (True, True, 2), (False, True, 2), (True, False, 1))]


@pytest.mark.parametrize("D,per_cam,use_bg,C", CASES)
def test_channels_forward_and_gradients_match_the_oracle(D, per_cam, use_bg, C):
    sc = _scene(C, seed=11 + D + 3 * C)
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(D)
    colors = torch.randn((C, N, D) if per_cam else (N, D), generator=g, dtype=torch.float64)
    bg = torch.rand((C, D), generator=g, dtype=torch.float64) if use_bg else None
    razor = _razor(sc)
    assert razor.mean() < 0.05, razor.mean()
    vc, va = _upstream(sc, D, razor, seed=100 + D)
    img, alpha, meta, gh = hip(sc, colors, bg, vc=vc, va=va)
    assert img.shape == (C, int(sc["height"]), int(sc["width"]), D) and alpha.shape[-1] == 1
    assert gh["colors"].shape == colors.shape
    ref_img, ref_alpha, gr = oracle(sc, lambda *a: colors, bg, vc, va)
    _check_fwd(img, alpha, ref_img, ref_alpha, razor)
    for k in NAMES + ("colors", "absgrad"):
        _check_grad(k, gh[k], gr[k])


def _consistency(sc, culling, training):
    N, C = sc["means"].shape[0], sc["viewmats"].shape[0]
    g = torch.Generator().manual_seed(3)
    rgb = torch.rand((N, 3), generator=g)
    x = torch.randn((N, 1), generator=g)
    bg4 = torch.rand((C, 4), generator=g)
    H, W = int(sc["height"]), int(sc["width"])
    vc3 = torch.randn((C, H, W, 3), generator=g) / (H * W)
    vc4 = torch.cat([vc3, torch.zeros((C, H, W, 1))], -1)
    kw = dict(grad=training, culling=culling)
    i3, a3, _, g3 = hip(sc, rgb, bg4[:, :3], vc=vc3, **kw)
    i4, a4, _, g4 = hip(sc, torch.cat([rgb, x], -1), bg4, vc=vc4, **kw)
    i1, a1, _, _ = hip(sc, x, bg4[:, 3:], vc=torch.zeros((C, H, W, 1)), **kw)
    assert torch.equal(i4[..., :3], i3) and torch.equal(a4, a3)
    assert torch.equal(i1[..., 0], i4[..., 3]) and torch.equal(a1, a4)
    if training:
        for k in NAMES + ("absgrad",):
            rel = ((g4[k] - g3[k]).abs().max() / (g3[k].abs().max() + 1e-30)).item()
            assert rel <= 1e-6, (k, rel)


@pytest.mark.parametrize("training", [False, True])
def test_channels_agree_bitwise_with_the_rgb_path_small(training):
    _consistency(_scene(2, seed=5), "gsplat", training)


@pytest.mark.parametrize("training", [False, True])
def test_channels_agree_bitwise_with_the_rgb_path_bench_scene(training):
    sc = config_bench_1m(seed=42, n=200_000)
    _consistency(sc, "tight", training)


def test_depth_as_a_channel():
    """gsplat's "RGB+D": colours concatenated with camera-space z (INTEGRATION.md "Depth as a channel")."""
    C = 2
    sc = _scene(C, seed=23)
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(9)
    rgb = torch.rand((C, N, 3), generator=g, dtype=torch.float64)
    razor = _razor(sc)
    vc, va = _upstream(sc, 4, razor, seed=5)
    # HIP side: z from the means in torch, differentiable
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = dev()
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(d) for k in NAMES + ("viewmats", "Ks")}
    ins = [t[k].clone().requires_grad_(True) for k in NAMES]
    vm = t["viewmats"]
    z = vm[:, 2, :3] @ ins[0].T + vm[:, 2, 3:]                     # [C, N]
    colors = torch.cat([rgb.to(d).float(), z[..., None]], -1)       # [C, N, 4]
    img, alpha, _ = rasterization(*ins, colors, vm, t["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=None, packed=False)
    loss = (img * vc.to(d).float()).sum() + (alpha * va.to(d).float()).sum()
    v_means = torch.autograd.grad(loss, ins[0])[0]
    # oracle side: the projection's depths as the fourth channel
    def cols(means, quats, scales, viewmats, Ks):
        _, _, depths, _ = TO.project(means, quats, scales, viewmats, Ks, int(sc["width"]), int(sc["height"]))
        return torch.cat([rgb, depths[..., None]], -1)
    ref_img, ref_alpha, gr = oracle(sc, cols, None, vc, va)
    keep = torch.from_numpy(~razor)
    e = (img[..., 3].detach().cpu().double() - ref_img[..., 3]).abs()[keep].max().item()
    scale = max(1.0, ref_img[..., 3].abs().max().item())
    assert e <= FWD_ATOL * scale, e
    _check_grad("means", v_means, gr["means"])


def test_four_channels_with_depth_rounds_equal_one_round():
    sc = _scene(1, seed=31, n=4000, W=160, H=96)
    N = sc["means"].shape[0]
    colors = torch.randn((N, 4), generator=torch.Generator().manual_seed(1))
    on = hip(sc, colors, grad=False, rounds="on")
    off = hip(sc, colors, grad=False, rounds="off")
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_four_channel_walk_rerun_equals_a_primed_call():
    """A training call whose first walk outgrows the first-guess cap_units repeats the blend into a larger walk arena; the fourth
    channel's checkpoint plane must follow it (workspace.Lease.ckpt_ext)."""
    from easy_gaussian_splatting_amd import rendering
    from easy_gaussian_splatting_amd import workspace as WS
    sc = _scene(1, seed=41, n=30000, W=256, H=192)
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(2)
    colors = torch.randn((N, 4), generator=g)
    vc = torch.randn((1, 192, 256, 4), generator=g)
    rendering.reset_hints()
    WS.pool.clear()
    reruns = rendering.stats["walk_reruns"]
    first = hip(sc, colors, vc=vc, culling="tight")
    rendering.reset_hints()
    # prime, then cut the work-unit capacity of the learnt hint below what the walk needs
    primed = hip(sc, colors, vc=vc, culling="tight")
    keys = [k for k in rendering._hints if k[4]]
    assert len(keys) == 1, list(rendering._hints)
    with rendering._state_lock:
        rendering._hints[keys[0]]["cap_units"] = 512
    before = rendering.stats["walk_reruns"]
    cut = hip(sc, colors, vc=vc, culling="tight")
    assert rendering.stats["walk_reruns"] == before + 1
    assert rendering.stats["walk_reruns"] >= reruns + 1
    again = hip(sc, colors, vc=vc, culling="tight")
    for run in (first, cut):
        assert torch.equal(run[0], again[0]) and torch.equal(run[1], again[1])
        for k in NAMES + ("colors", "absgrad"):
            assert torch.equal(run[3][k], again[3][k]), k
    for k in NAMES + ("colors",):
        assert torch.equal(primed[3][k], again[3][k]), k
