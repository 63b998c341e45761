"""Depth render modes on the GPU (`rasterization(render_mode="D" | "ED" | "RGB+D" | "RGB+ED")`: gs_rec_depth, the blend at Dc + 1
channels, gs_depth_grads, gs_expected_depth_fwd / _bwd) against the oracle composed in tests/depth_ref.py.

Bounds -- the project's own, as tests/test_gpu_channels.py applies them: colour channels and alphas 1e-4 abs outside the razor pixels
(within 1e-4 of a blend discontinuity); the accumulated depth 1e-4 * max(1, max |reference depth image|); gradients 1e-3 of each
tensor's largest reference magnitude with the upstream gradient zeroed on the razor pixels (their share below 0.05); view-matrix
gradients 1e-3 of the largest entry per camera.  The ED forward follows by error propagation through D / alpha:
|ED - ED_ref| <= 1e-4 * (max(1, max |D_ref|) + |ED_ref|) / alpha_ref on covered, non-razor pixels; and ED equals
D_out / alpha_out.clamp_min(1e-10) as torch evaluates it on the GPU to 2.4e-7 relative (the storage bound of the parity suite)."""
import numpy as np
import pytest
import torch

import cameras
import depth_ref as DR

pytestmark = pytest.mark.gpu
FWD_ATOL = 1e-4
GRAD_RTOL = 1e-3
STORAGE_RTOL = 2.4e-7
GRAD_NAMES = DR.GEO


def _rel(got, ref):
    ref = ref.double()
    return ((got.detach().cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _check_forward(mode, out, ref, rz):
    """Colours, alphas and the last (depth) channel of `out` against the composed oracle, outside the razor pixels."""
    keep = torch.from_numpy(~rz)
    img, alpha = out["img"].cpu().double(), out["alpha"].cpu().double()
    assert img.shape == ref["img"].shape and alpha.shape == ref["alpha"].shape
    e_a = (alpha - ref["alpha"])[..., 0].abs()[keep].max().item()
    print(f"{mode}: max alpha error {e_a:.3g}")
    assert e_a <= FWD_ATOL, e_a
    if img.shape[-1] > 1:
        e_c = (img[..., :-1] - ref["img"][..., :-1]).abs().amax(-1)[keep].max().item()
        print(f"{mode}: max colour error {e_c:.3g}")
        assert e_c <= FWD_ATOL, e_c
    d_scale = max(1.0, ref["acc"][..., -1].abs().max().item())
    err = (img[..., -1] - ref["img"][..., -1]).abs()
    if mode.endswith("ED"):
        a_ref = ref["alpha"][..., 0]
        covered = keep & (a_ref > 0)
        bound = FWD_ATOL * (d_scale + ref["img"][..., -1].abs()) / a_ref.clamp(min=1e-300)
        worst = (err / bound)[covered].max().item()
        print(f"{mode}: max ED error / bound {worst:.3g} over {int(covered.sum())} covered pixels")
        assert worst <= 1.0, worst
        uncovered = keep & (a_ref == 0)   # exactly 0 on both sides
        if uncovered.any():
            assert float(img[..., -1][uncovered].abs().max()) == 0.0 and float(ref["img"][..., -1][uncovered].abs().max()) == 0.0
    else:
        e_d = err[keep].max().item()
        print(f"{mode}: max depth error {e_d:.3g} (bound {FWD_ATOL * d_scale:.3g})")
        assert e_d <= FWD_ATOL * d_scale, (e_d, d_scale)


def _check_grads(out, ref, n_colour_leaves, colours_get_none):
    for i, name in enumerate(GRAD_NAMES):
        r = _rel(out["grads"][i], ref["grads"][i])
        print(f"  v_{name}: rel err {r:.3g}")
        assert r <= GRAD_RTOL, (name, r)
    for j in range(n_colour_leaves):
        got, want = out["grads"][len(GRAD_NAMES) + j], ref["grads"][len(GRAD_NAMES) + j]
        if colours_get_none:   # D / ED: the colours are replaced by the depth
            assert want is None and (got is None or float(got.abs().max()) == 0.0)
        else:
            r = _rel(got, want)
            print(f"  v_colors[{j}]: rel err {r:.3g}")
            assert r <= GRAD_RTOL, (j, r)
    r = _rel(out["absgrad"], ref["absgrad"])
    print(f"  absgrad: rel err {r:.3g}")
    assert r <= GRAD_RTOL, r


def _parity(sc, mode, colors, sh_degree, bg, seed, culling="gsplat", **kw):
    rz = DR.razor(sc)
    assert rz.mean() < 0.05, rz.mean()
    Dc = 0 if mode in ("D", "ED") else (3 if sh_degree is not None else np.asarray(colors[0]).shape[-1])
    vc, va = DR.upstream(rz, Dc + 1, seed)
    out = DR.gpu(sc, mode, colors, sh_degree, bg, vc, va, culling=culling, **kw)
    ref = DR.reference(sc, mode, colors, sh_degree, bg, vc, va)
    assert out["img"].shape == (sc["viewmats"].shape[0], int(sc["height"]), int(sc["width"]), Dc + 1)
    _check_forward(mode, out, ref, rz)
    _check_grads(out, ref, len(colors), colours_get_none=Dc == 0)
    if mode.endswith("ED"):   # ... and the division itself, against torch's own on the GPU
        acc = DR.gpu(sc, mode.replace("ED", "D"), colors, sh_degree, bg, grad=False, culling=culling, **kw)
        assert torch.equal(acc["alpha"], out["alpha"]) and torch.equal(acc["img"][..., :-1], out["img"][..., :-1])
        want = acc["img"][..., -1:] / acc["alpha"].clamp_min(1e-10)
        assert bool(((out["img"][..., -1:] - want).abs() <= STORAGE_RTOL * want.abs()).all())
    return out, ref


# ---- 1. parity against the composed oracle ----

def test_rgb_d_with_sh_colours_and_backgrounds():
    sc = DR.scene("B")
    _parity(sc, "RGB+D", [sc["shs"]], 3, sc["backgrounds"], seed=1)


def test_rgb_ed_with_the_sh_pair_on_ragged_tiles():
    sc = DR.scene("D")
    shs = sc["shs"]
    _parity(sc, "RGB+ED", [np.ascontiguousarray(shs[:, :1]), np.ascontiguousarray(shs[:, 1:])], 2, sc["backgrounds"], seed=2, culling="tight")


def test_d_alone_with_two_cameras():
    sc = DR.scene("A")
    _parity(sc, "D", [sc["shs"]], 0, sc["backgrounds"], seed=3)   # (a given background is replaced by zero)


def test_ed_alone_on_a_sparse_scene():
    sc = DR.scene("E")
    _parity(sc, "ED", [sc["shs"]], 1, None, seed=4, culling="gsplat_eager")


@pytest.mark.parametrize("per_cam", [False, True])
@pytest.mark.parametrize("Dc", [1, 2, 3])
def test_features_plus_depth(Dc, per_cam):
    sc = DR.scene("A")
    C, N = sc["viewmats"].shape[0], sc["means"].shape[0]
    rng = np.random.default_rng(10 + Dc)
    feats = rng.standard_normal((C, N, Dc) if per_cam else (N, Dc)).astype(np.float32)
    bg = rng.random((C, Dc)).astype(np.float32) if per_cam else None
    out, _ = _parity(sc, "RGB+D", [feats], None, bg, seed=20 + Dc)
    assert out["grads"][4].shape == feats.shape


def test_activations_inside_the_projection_with_a_depth_mode():
    """`_activations="exp_sigmoid"` (the model's raw parameters): the same render against the same reference and, by the chain rule,
    the gradients w.r.t. the raw parameters."""
    sc = DR.scene("B")
    op = np.clip(sc["opacities"], 1e-4, 1 - 1e-4).astype(np.float32)
    act_sc = dict(sc, opacities=op)
    raw = dict(sc, scales=np.log(sc["scales"]).astype(np.float32), opacities=np.log(op / (1 - op)).astype(np.float32))
    # (the reference takes the activations of the float32 raw parameters)
    act_sc["scales"], act_sc["opacities"] = np.exp(raw["scales"].astype(np.float64)), 1.0 / (1.0 + np.exp(-raw["opacities"].astype(np.float64)))
    rz = DR.razor(act_sc)
    assert rz.mean() < 0.05
    vc, va = DR.upstream(rz, 4, 7)
    out = DR.gpu(raw, "RGB+ED", [sc["shs"]], 3, sc["backgrounds"], vc, va, _activations="exp_sigmoid")
    ref = DR.reference(act_sc, "RGB+ED", [sc["shs"]], 3, sc["backgrounds"], vc, va)
    _check_forward("RGB+ED", out, ref, rz)
    s64, o64 = torch.from_numpy(act_sc["scales"]), torch.from_numpy(act_sc["opacities"])
    ref["grads"][2], ref["grads"][3] = ref["grads"][2] * s64, ref["grads"][3] * o64 * (1 - o64)
    _check_grads(out, ref, 1, colours_get_none=False)


# ---- 2. consistency with the RGB call, bit for bit ----

@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("culling", ["gsplat", "tight"])
def test_depth_modes_leave_the_rgb_render_alone(culling, training):
    sc = DR.scene("B")
    C, H, W = sc["viewmats"].shape[0], int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(3)
    vc3 = torch.randn((C, H, W, 3), generator=g) / (H * W)
    vc4 = torch.cat([vc3, torch.zeros((C, H, W, 1))], -1)
    kw = dict(grad=training, culling=culling)
    rgb = DR.gpu(sc, "RGB", [sc["shs"]], 3, sc["backgrounds"], vc3, **kw)
    rgbd = DR.gpu(sc, "RGB+D", [sc["shs"]], 3, sc["backgrounds"], vc4, **kw)
    d = DR.gpu(sc, "D", [sc["shs"]], 3, sc["backgrounds"], torch.zeros((C, H, W, 1)), **kw)
    assert torch.equal(rgbd["img"][..., :3], rgb["img"]) and torch.equal(rgbd["alpha"], rgb["alpha"])
    assert torch.equal(d["img"][..., 0], rgbd["img"][..., 3]) and torch.equal(d["alpha"], rgbd["alpha"])
    assert float(rgbd["img"][..., 3].max()) > 1.0   # (a depth map, not zeros)
    if training:
        for i in range(len(rgb["grads"])):
            rel = ((rgbd["grads"][i] - rgb["grads"][i]).abs().max() / (rgb["grads"][i].abs().max() + 1e-30)).item()
            assert rel <= 1e-6, (i, rel)
        rel = ((rgbd["absgrad"] - rgb["absgrad"]).abs().max() / (rgb["absgrad"].abs().max() + 1e-30)).item()
        assert rel <= 1e-6, rel


# ---- 3. the whole-item path of the row reduction ----

def test_depth_gradient_of_gaussians_that_own_whole_items():
    """Scene C: footprints of up to every tile of the image -- a Gaussian then owns runs of more than 64 gradient rows and
    quad_sums_wave takes its whole-item path."""
    sc = DR.scene("C")
    rz = DR.razor(sc)
    assert rz.mean() < 0.05
    vc, va = DR.upstream(rz, 1, 5)
    out = DR.gpu(sc, "D", [sc["shs"]], 1, None, vc, va, culling="gsplat_eager")
    most = int(out["meta"]["tiles_per_gauss"].max())
    print("largest footprint:", most, "tiles")
    assert most >= 32   # (x 4 quadrants: at least one whole 64-row item inside one Gaussian's range)
    ref = DR.reference(sc, "D", [sc["shs"]], 1, None, vc, va)
    r = _rel(out["grads"][0], ref["grads"][0])
    print(f"v_means rel err {r:.3g}")
    assert r <= GRAD_RTOL, r


# ---- 4. camera gradients ----

def test_view_matrix_gradient_with_the_depth_channel():
    sc, proj = cameras.config_scene("inside", n=1500, W=96, H=64, C=2)
    rz = DR.razor(sc, **proj)
    assert rz.mean() < 0.05
    vc, va = DR.upstream(rz, 4, 6)
    args = (sc, "RGB+D", [sc["shs"]], 3, sc["backgrounds"], vc, va)
    a = DR.gpu(*args, cam=True, **proj)
    b = DR.gpu(*args, cam=True, **proj)
    plain = DR.gpu(*args, cam=False, **proj)
    ref = DR.reference(*args, cam=True, **proj)
    got, want = a["v_viewmats"].cpu().double().numpy(), ref["v_viewmats"].numpy()
    assert np.isfinite(got).all()
    for c in range(want.shape[0]):
        rel = np.abs(got[c] - want[c]).max() / np.abs(want[c]).max()
        print(f"camera {c}: rel err of v_viewmats {rel:.3g}; largest entry of row 2 / of the matrix: {np.abs(want[c][2]).max() / np.abs(want[c]).max():.3g}")
        assert rel <= GRAD_RTOL, (c, rel)
    assert torch.equal(a["v_viewmats"], b["v_viewmats"])   # (fixed-order sums: the same bits)
    assert torch.equal(a["img"], plain["img"]) and torch.equal(a["alpha"], plain["alpha"]) and torch.equal(a["absgrad"], plain["absgrad"])
    for i, (x, y) in enumerate(zip(a["grads"], plain["grads"])):
        assert torch.equal(x, y), f"gradient {i}"


# ---- 5. expected depth where most pixels are uncovered ----

def test_expected_depth_is_zero_and_finite_where_nothing_is_covered():
    sc = DR.scene("E")
    C, H, W = 1, int(sc["height"]), int(sc["width"])
    g = torch.Generator().manual_seed(8)
    for mode, D in (("ED", 1), ("RGB+ED", 4)):
        vc, va = torch.randn((C, H, W, D), generator=g), torch.randn((C, H, W, 1), generator=g)   # (nonzero everywhere)
        out = DR.gpu(sc, mode, [sc["shs"]], 1, sc["backgrounds"], vc, va)
        uncovered = out["alpha"][..., 0] == 0
        assert 0.5 < float(uncovered.float().mean()) < 0.95
        assert float(out["img"][..., -1][uncovered].abs().max()) == 0.0
        assert float(out["img"][..., -1][~uncovered].min()) > 0.0
        assert bool(torch.isfinite(out["img"]).all()) and bool(torch.isfinite(out["alpha"]).all())
        for gr in out["grads"] + [out["absgrad"]]:
            assert gr is None or bool(torch.isfinite(gr).all())
        assert float(out["grads"][0].abs().max()) > 0


# ---- 6. nothing to render ----

def test_empty_and_invisible_inputs_in_rgb_d():
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = torch.device("cuda:0")
    V = torch.eye(4, device=d)[None]
    K = torch.tensor([[50.0, 0, 16], [0, 50.0, 16], [0, 0, 1]], device=d)[None]
    bg = torch.tensor([[0.25, 0.5, 0.75]], device=d)
    want = torch.cat([bg, bg.new_zeros((1, 1))], 1).expand(1, 32, 32, 4).contiguous()
    z = lambda *s: torch.zeros(*s, device=d)
    for mode in ("RGB+D", "RGB+ED"):
        img, alpha, meta = rasterization(z(0, 3), z(0, 4), z(0, 3), z(0), z(0, 16, 3), V, K, 32, 32, sh_degree=3, packed=False, backgrounds=bg,
                                         render_mode=mode)
        assert img.shape == (1, 32, 32, 4) and torch.allclose(img, want) and float(img[..., 3].abs().max()) == 0.0 and float(alpha.abs().max()) == 0.0
        means = torch.tensor([[0.0, 0, -2.0], [0.1, 0, -3.0]], device=d, requires_grad=True)
        quats = torch.ones(2, 4, device=d, requires_grad=True)
        scales = torch.full((2, 3), 0.1, device=d, requires_grad=True)
        op = torch.full((2,), 0.5, device=d, requires_grad=True)
        sh = torch.zeros(2, 16, 3, device=d, requires_grad=True)
        img, alpha, meta = rasterization(means, quats, scales, op, sh, V, K, 32, 32, sh_degree=3, packed=False, backgrounds=bg, absgrad=True,
                                         render_mode=mode)
        assert int((meta["radii"] > 0).sum()) == 0 and torch.allclose(img.detach(), want) and float(img.detach()[..., 3].abs().max()) == 0.0
        img.sum().backward()
        for p in (means, quats, scales, op, sh):
            assert p.grad is not None and float(p.grad.abs().max()) == 0.0


# ---- 7. the model layer ----

def test_model_forward_returns_the_depth_map():
    from easy_gaussian_splatting_amd.model import GaussianModel
    from easy_gaussian_splatting_amd.rendering import rasterization
    from scenes import make_scene
    d = torch.device("cuda:0")
    W, H = 128, 96
    sc = make_scene(4000, W, H, sh_degree=3, n_views=1, seed=3, scale_range=(0.01, 0.08), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    m = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=T(sc["shs"][:, :1].copy()),
                      sh_rest=T(sc["shs"][:, 1:].copy()), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                      white_background=True).to(d)
    data = {"w2c": T(sc["viewmats"][0]).to(d), "K": T(sc["Ks"][0]).to(d), "width": W, "height": H}
    vc = torch.randn((H, W, 3), generator=torch.Generator().manual_seed(0)).to(d)

    def grads(out):
        for k in m.param_names:
            getattr(m, k).grad = None
        (out["render_img"] * vc).sum().backward()
        return [getattr(m, k).grad.clone() for k in m.param_names]

    base = m(data)
    dflt = m(data, depth=None)
    assert "render_depth" not in base and "render_depth" not in dflt and torch.equal(base["render_img"], dflt["render_img"])
    for x, y in zip(grads(base), grads(dflt)):
        assert torch.equal(x, y)
    with_depth = m(data, depth="ED")
    assert with_depth["render_depth"].shape == (H, W, 1) and with_depth["render_img"].shape == (H, W, 3)
    assert torch.equal(with_depth["render_img"], base["render_img"])   # (the clamp applies to the RGB part; same bits as the RGB render)
    img, _, _ = rasterization(m.means, m.quats, m.log_scales, m.logit_opacities, (m.sh_0, m.sh_rest), data["w2c"][None], data["K"][None], W, H,
                              sh_degree=m.active_sh_degree, packed=False, backgrounds=m.BACKGROUND[None], _activations="exp_sigmoid",
                              _tile_culling="tight", render_mode="RGB+ED")
    assert torch.equal(with_depth["render_depth"], img[0, ..., 3:])
    assert float(with_depth["render_depth"].max()) > 1.0   # (unclamped)
    # the depth map is differentiable
    for k in m.param_names:
        getattr(m, k).grad = None
    m(data, depth="D")["render_depth"].sum().backward()
    assert float(m.means.grad.abs().max()) > 0 and bool(torch.isfinite(m.means.grad).all())
    with pytest.raises(ValueError):
        m(data, depth="RGB+D")
