"""Colour features of more than four channels on the GPU (chunks of four over one projection and one set of lists --
gs_rec_colors_chunk, gs_blend_fwd_ch / gs_blend_bwd_ch per chunk, gs_rows_accumulate, gs_channel_grads_chunk, gs_chunk_scatter /
gs_chunk_gather): parity with the float64 torch oracle, every chunk bit for bit the call on the channel slice, the alpha gradient
counted once, repeated backwards, the walk re-run and the keywords that ride along.  Bounds as tests/test_gpu_channels.py: 1e-4 abs on
images outside the razor pixels, gradients 1e-3 of each tensor's largest reference magnitude with the upstream zeroed on razor pixels;
sums over chunks against the sum of the slices' gradients: 1e-6 of the tensor's largest magnitude (float32 sums of a few terms in
another order)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import torch_oracle as TO
from scenes import make_scene

pytestmark = pytest.mark.gpu
FWD_ATOL = 1e-4
GRAD_RTOL = 1e-3
SUM_RTOL = 1e-6
NAMES = ("means", "quats", "scales", "opacities")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _scene(C, seed, n=1500, W=100, H=80):
    return make_scene(n, W, H, sh_degree=0, n_views=C, seed=seed, scale_range=(0.02, 0.2), dist=4.0)


def _chunks(D):
    from easy_gaussian_splatting_amd.rendering import channel_chunks
    return channel_chunks(D)


def _razor(sc):
    """[C,H,W] pixels within 1e-4 of a blend discontinuity; the contributor sets do not depend on the colours."""
    fw = CO.render(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["shs"][:, 0], sc["viewmats"], sc["Ks"],
                   int(sc["width"]), int(sc["height"]), sh_degree=None, dtype=np.float64)
    return CO.blend_margin(fw, mu_tol_ulps=1.0, conic_rtol=2.4e-7) < 1e-4


class Render:
    """One rasterization() call on the GPU, kept open for backwards: .img, .alpha, .meta and .grads(vc, va) -> {name: gradient}."""
    def __init__(self, sc, colors, bg=None, grad=True, culling="gsplat", cam_grads=False, raw=False, **kw):
        from easy_gaussian_splatting_amd.rendering import rasterization
        d = dev()
        t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).float().to(d) for k in NAMES + ("viewmats", "Ks")}
        if raw:   # `_activations="exp_sigmoid"`: log-scales and logit opacities
            t["scales"], t["opacities"] = t["scales"].log(), torch.logit(t["opacities"])
        self.names = NAMES + ("colors",) + (("viewmats",) if cam_grads else ())
        self.ins = [t[k].clone().requires_grad_(grad) for k in NAMES]
        self.ins.append(colors.detach().to(d).float().contiguous().requires_grad_(grad))
        vm = t["viewmats"].clone().requires_grad_(True) if cam_grads else t["viewmats"]
        if cam_grads:
            self.ins.append(vm)
        with torch.set_grad_enabled(grad):
            self.img, self.alpha, self.meta = rasterization(
                *self.ins[:5], vm, t["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=None, packed=False,
                backgrounds=None if bg is None else bg.to(d).float(), _tile_culling=culling, _camera_grads=cam_grads, **kw)

    def grads(self, vc=None, va=None, retain=False):
        d = dev()
        outs, ups = [], []
        if vc is not None:
            outs.append(self.img); ups.append(vc.to(d).float())
        if va is not None:
            outs.append(self.alpha); ups.append(va.to(d).float())
        gs = torch.autograd.grad(outs, self.ins, grad_outputs=ups, retain_graph=retain, allow_unused=True)
        torch.cuda.synchronize()
        return dict(zip(self.names, gs))


def _slices(sc, colors, bg, vc, va_chunk=None, va=None, **kw):
    """The loop a caller writes without the feature: one call per chunk of four channels.  Returns ([(img, alpha)], [grads])."""
    D = colors.shape[-1]
    outs, grads = [], []
    for j, (f, c) in enumerate(_chunks(D)):
        r = Render(sc, colors[..., f:f + c], None if bg is None else bg[:, f:f + c], **kw)
        outs.append((r.img.detach(), r.alpha.detach()))
        if kw.get("grad", True):
            grads.append(r.grads(vc[..., f:f + c], va if j == va_chunk else None))
    return outs, grads


def _rel(got, ref):
    return ((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30)).item()


def _oracle(sc, colors, bg, vc, va):
    T = {k: torch.from_numpy(np.asarray(sc[k], dtype=np.float64)) for k in NAMES + ("viewmats", "Ks")}
    ins = [T[k].clone().requires_grad_(True) for k in NAMES] + [colors.clone().requires_grad_(True)]
    img, alpha, _ = TO.rasterization(*ins, T["viewmats"], T["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=None, packed=False,
                                     backgrounds=bg)
    gs = torch.autograd.grad((img * vc).sum() + (alpha * va).sum(), ins)
    return img.detach(), alpha.detach(), dict(zip(NAMES + ("colors",), gs))


@pytest.mark.parametrize("D,per_cam,use_bg,C", [(5, False, False, 1), (7, True, False, 1), (8, False, True, 2), (9, True, True, 2)])
def test_wide_channels_forward_and_gradients_match_the_oracle(D, per_cam, use_bg, C):
    sc = _scene(C, seed=31 + D + 3 * C)
    N, H, W = sc["means"].shape[0], int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(D)
    colors = torch.randn((C, N, D) if per_cam else (N, D), generator=g, dtype=torch.float64)
    bg = torch.rand((C, D), generator=g, dtype=torch.float64) if use_bg else None
    razor = _razor(sc)
    print("razor fraction", razor.mean())
    assert razor.mean() < 0.05, razor.mean()
    keep = torch.from_numpy(~razor)
    vc = torch.randn((C, H, W, D), generator=g, dtype=torch.float64) * keep.double()[..., None]
    va = torch.randn((C, H, W, 1), generator=g, dtype=torch.float64) * keep.double()[..., None]
    r = Render(sc, colors, bg)
    assert r.img.shape == (C, H, W, D) and r.alpha.shape == (C, H, W, 1)
    gh = r.grads(vc, va)
    assert gh["colors"].shape == colors.shape
    ref_img, ref_alpha, gr = _oracle(sc, colors, bg, vc, va)
    e_c = (r.img.detach().cpu().double() - ref_img).abs().amax(-1)[keep].max().item()
    e_a = (r.alpha.detach().cpu().double() - ref_alpha)[..., 0].abs()[keep].max().item()
    print("forward", e_c, e_a)
    assert e_c <= FWD_ATOL and e_a <= FWD_ATOL, (e_c, e_a)
    for k in NAMES + ("colors",):
        rel = _rel(gh[k].cpu(), gr[k])
        print(k, rel)
        assert rel <= GRAD_RTOL, (k, rel)


@pytest.mark.parametrize("culling", ["gsplat", "tight"])
@pytest.mark.parametrize("training", [False, True])
def test_chunks_equal_the_sliced_calls_bit_for_bit(culling, training):
    C, D = 2, 9
    sc = _scene(C, seed=5)
    N, H, W = sc["means"].shape[0], int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(3)
    colors = torch.randn((N, D), generator=g)
    bg = torch.rand((C, D), generator=g)
    vc = torch.randn((C, H, W, D), generator=g) / (H * W)
    kw = dict(grad=training, culling=culling)
    r = Render(sc, colors, bg, **kw)
    outs, grads = _slices(sc, colors, bg, vc, **kw)
    for (f, c), (img, alpha) in zip(_chunks(D), outs):
        assert torch.equal(r.img.detach()[..., f:f + c], img), f
        assert torch.equal(r.alpha.detach(), alpha), f
    if training:
        gw = r.grads(vc)
        for (f, c), gs in zip(_chunks(D), grads):
            assert torch.equal(gw["colors"][..., f:f + c], gs["colors"]), f
        for k in NAMES:
            rel = _rel(gw[k], sum(gs[k] for gs in grads))
            assert rel <= SUM_RTOL, (k, rel)


def test_the_alpha_gradient_is_counted_once():
    C, D = 1, 8
    sc = _scene(C, seed=7)
    N, H, W = sc["means"].shape[0], int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(4)
    colors = torch.randn((N, D), generator=g)
    va = torch.randn((C, H, W, 1), generator=g) / (H * W)
    gw = Render(sc, colors).grads(None, va)
    g4 = Render(sc, colors[:, :4]).grads(None, va)
    for k in NAMES:
        rel = _rel(gw[k], g4[k])
        assert rel <= SUM_RTOL, (k, rel)
    assert gw["colors"].shape == (N, D) and float(gw["colors"].abs().max()) == 0.0


def test_repeated_backward_over_one_forward():
    C, D = 2, 9
    sc = _scene(C, seed=9)
    N, H, W = sc["means"].shape[0], int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(5)
    colors = torch.randn((C, N, D), generator=g)
    bg = torch.rand((C, D), generator=g)
    v1c, v2c = (torch.randn((C, H, W, D), generator=g) / (H * W) for _ in range(2))
    v1a, v2a = (torch.randn((C, H, W, 1), generator=g) / (H * W) for _ in range(2))
    r = Render(sc, colors, bg)
    a = r.grads(v1c, v1a, retain=True)
    b = r.grads(v1c, v1a, retain=True)   # (the lease now holds the last chunk's walk, the records its colours)
    for k in NAMES + ("colors",):
        assert torch.equal(a[k], b[k]), k
    c = r.grads(v2c, v2a, retain=True)
    both = r.grads(v1c + v2c, v1a + v2a)
    for k in NAMES + ("colors",):
        rel = _rel(a[k] + c[k], both[k])
        assert rel <= 1e-5, (k, rel)


def test_wide_walk_rerun_equals_a_primed_call():
    """tests/test_gpu_channels.py::test_four_channel_walk_rerun_equals_a_primed_call at D = 9: the overflow re-run blends the chunk
    whose colours the records hold, and the chunks after it find capacities that fit."""
    from easy_gaussian_splatting_amd import rendering
    from easy_gaussian_splatting_amd import workspace as WS
    sc = _scene(1, seed=41, n=30000, W=256, H=192)
    N, D = sc["means"].shape[0], 9
    g = torch.Generator().manual_seed(2)
    colors = torch.randn((N, D), generator=g)
    vc = torch.randn((1, 192, 256, D), generator=g)
    va = torch.randn((1, 192, 256, 1), generator=g)

    def run():
        r = Render(sc, colors, culling="tight")
        return r.img.detach(), r.alpha.detach(), r.grads(vc, va)
    rendering.reset_hints()
    WS.pool.clear()
    run()
    primed = run()
    keys = [k for k in rendering._hints if k[4]]
    assert len(keys) == 1, list(rendering._hints)
    with rendering._state_lock:
        rendering._hints[keys[0]]["cap_units"] = 512
    before = rendering.stats["walk_reruns"]
    cut = run()
    assert rendering.stats["walk_reruns"] == before + 1
    assert torch.equal(cut[0], primed[0]) and torch.equal(cut[1], primed[1])
    for k in NAMES + ("colors",):
        assert torch.equal(cut[2][k], primed[2][k]), k


@pytest.mark.parametrize("kw", [dict(camera_model="fisheye"),
                                dict(rasterize_mode="antialiased", _activations="exp_sigmoid", cam_grads=True, raw=True)],
                         ids=["fisheye", "antialiased-exp_sigmoid-camera_grads"])
def test_keywords_ride_along(kw):
    C, D = 2, 6
    sc = _scene(C, seed=13)
    N, H, W = sc["means"].shape[0], int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(6)
    colors = torch.randn((N, D), generator=g)
    bg = torch.rand((C, D), generator=g)
    vc = torch.randn((C, H, W, D), generator=g) / (H * W)
    va = torch.randn((C, H, W, 1), generator=g) / (H * W)
    r = Render(sc, colors, bg, **kw)
    gw = r.grads(vc, va)
    outs, grads = _slices(sc, colors, bg, vc, va_chunk=0, va=va, **kw)
    for (f, c), (img, alpha) in zip(_chunks(D), outs):
        assert torch.equal(r.img.detach()[..., f:f + c], img) and torch.equal(r.alpha.detach(), alpha), f
    for k in NAMES + (("viewmats",) if kw.get("cam_grads") else ()):
        assert float(gw[k].abs().max()) > 0.0, k
        rel = _rel(gw[k], sum(gs[k] for gs in grads))
        assert rel <= SUM_RTOL, (k, rel)
    for (f, c), gs in zip(_chunks(D), grads):
        rel = _rel(gw["colors"][..., f:f + c], gs["colors"])
        assert rel <= SUM_RTOL, (f, rel)


def test_unused_outputs_and_empty_scenes():
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = dev()
    D = 5
    V = torch.eye(4, device=d)[None]
    K = torch.tensor([[50.0, 0, 16], [0, 50.0, 16], [0, 0, 1]], device=d)[None]
    bg = torch.tensor([[0.25, 0.5, 0.75, -1.0, 2.0]], device=d)
    full = bg.expand(1, 32, 32, D).contiguous()
    # N = 0
    z = lambda *s: torch.zeros(*s, device=d, requires_grad=True)
    ins = [z(0, 3), z(0, 4), z(0, 3), z(0), z(0, D)]
    img, alpha, meta = rasterization(*ins, V, K, 32, 32, sh_degree=None, packed=False, backgrounds=bg)
    assert img.shape == (1, 32, 32, D) and alpha.shape == (1, 32, 32, 1) and meta["radii"].shape == (1, 0)
    assert torch.equal(img.detach(), full) and float(alpha.detach().abs().max()) == 0.0
    gs = torch.autograd.grad(img.sum() + alpha.sum(), ins)
    assert gs[4].shape == (0, D)
    # everything behind the camera: nothing visible, the gradients exist and are zero
    means = torch.tensor([[0.0, 0, -2.0], [0.1, 0, -3.0]], device=d, requires_grad=True)
    quats = torch.ones(2, 4, device=d, requires_grad=True)
    scales = torch.full((2, 3), 0.1, device=d, requires_grad=True)
    op = torch.full((2,), 0.5, device=d, requires_grad=True)
    col = torch.ones(2, D, device=d, requires_grad=True)
    img, alpha, meta = rasterization(means, quats, scales, op, col, V, K, 32, 32, sh_degree=None, packed=False, backgrounds=bg)
    assert int((meta["radii"] > 0).sum()) == 0 and torch.equal(img.detach(), full) and float(alpha.detach().abs().max()) == 0.0
    for gr, p in zip(torch.autograd.grad(img.sum() + alpha.sum(), (means, quats, scales, op, col)), (means, quats, scales, op, col)):
        assert gr.shape == p.shape and float(gr.abs().max()) == 0.0
    # a loss on the alphas alone (v_render_colors = None): geometry gradients flow, the colour gradient is zero
    means = torch.tensor([[0.0, 0, 2.0], [0.1, 0, 3.0]], device=d, requires_grad=True)
    img, alpha, meta = rasterization(means, quats, scales, op, col, V, K, 32, 32, sh_degree=None, packed=False, backgrounds=bg)
    assert img.shape == (1, 32, 32, D) and int((meta["radii"] > 0).sum()) == 2
    v_means, v_col = torch.autograd.grad(alpha.sum(), (means, col))
    assert float(v_means.abs().max()) > 0.0 and v_col.shape == (2, D) and float(v_col.abs().max()) == 0.0
    # ... and where no Gaussian reaches, the background is reproduced
    assert torch.equal(img.detach()[0, 0, 0], bg[0]) and float(alpha.detach()[0, 0, 0, 0]) == 0.0
