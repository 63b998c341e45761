"""Blend-weight scores on the GPU (rendering.blend_weights: gs_blend_scores, gs_score_reduce; importance.py: gs_score_accumulate;
GaussianModel.prune) -- DESIGN.md 28.

1. Exact against the forward.  `rasterization(colors=torch.eye(N))` renders one-hot features: channel n of a pixel is that pixel's
   w for Gaussian n exactly (the forward accumulates fma(colour, w, acc) with colour in {0, 1}).  From that image: hits equal exactly,
   weight_max equal bit for bit, |weight_sum - sum_ref| <= hits * 2^-23 * sum_ref (the fp32 summation bound for at most `hits`
   additions of non-negative terms, doubled for the final rounding).
2. Identities on an ordinary scene of 20 k Gaussians, where one-hot features are infeasible.
3. The accumulator against its torch restatement.
4. collect -> prune_mask -> GaussianModel.prune on a trained model: the views render bit for bit as before."""
import numpy as np
import pytest
import torch

import blend_weights_ref as BR
from scenes import make_scene

pytestmark = pytest.mark.gpu
MODES = ("gsplat", "tight", "gsplat_eager")
_CACHE = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _t(sc):
    return {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev()) for k in ("means", "quats", "scales", "opacities", "viewmats", "Ks")}


def _geom(t):
    return t["means"], t["quats"], t["scales"], t["opacities"]


def _one_hot(sc, **kw):
    """(w [C,H,W,N] -- the forward's per-pixel weights --, render_alphas, radii) from the one-hot render."""
    from easy_gaussian_splatting_amd.rendering import rasterization
    t = _t(sc)
    n = t["means"].shape[0]
    with torch.no_grad():
        img, alphas, meta = rasterization(*_geom(t), torch.eye(n, device=dev()), t["viewmats"], t["Ks"], sc["width"], sc["height"],
                                          sh_degree=None, backgrounds=None, packed=False, **kw)
    return img, alphas, meta["radii"]


def _scores(sc, mode="gsplat", **kw):
    from easy_gaussian_splatting_amd.rendering import blend_weights
    t = _t(sc)
    out = blend_weights(*_geom(t), t["viewmats"], t["Ks"], sc["width"], sc["height"], _tile_culling=mode, **kw)
    assert not any(v.requires_grad for v in out.values())
    assert out["weight_sum"].dtype == torch.float32 and out["weight_max"].dtype == torch.float32
    assert out["hits"].dtype == torch.int32 and out["radii"].dtype == torch.int32
    return out


def _check_exact(sc, img, radii, modes=MODES, **kw):
    """The three scores of every mode against the one-hot image `img`; returns the first mode's scores."""
    hits_ref = (img > 0).sum(dim=(1, 2)).to(torch.int32)
    max_ref = img.amax(dim=(1, 2))
    sum_ref = img.double().sum(dim=(1, 2))
    first = None
    for mode in modes:
        out = _scores(sc, mode, **kw)
        assert torch.equal(out["radii"], radii), mode
        assert torch.equal(out["hits"], hits_ref), (mode, (out["hits"] - hits_ref).abs().max().item())
        assert torch.equal(out["weight_max"].view(torch.int32), max_ref.view(torch.int32)), (mode, (out["weight_max"] - max_ref).abs().max().item())
        err = (out["weight_sum"].double() - sum_ref).abs()
        bound = hits_ref.double() * 2.0 ** -23 * sum_ref
        print(f"[blend_weights] {mode}: N {img.shape[-1]} largest |sum - ref| / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), (mode, (err - bound).max().item())
        if first is None:
            first = out
        else:   # the list mode changes neither the taken pixels nor the largest weight by a bit
            assert torch.equal(out["hits"], first["hits"]) and torch.equal(out["weight_max"].view(torch.int32), first["weight_max"].view(torch.int32))
    return first


@pytest.mark.parametrize("n", [5, 12, 20, 29, 33, 64, 203])
def test_faint_stack_matches_the_forward_exactly(n):
    """Every Gaussian covers the image, nothing saturates: tail classes 1-4, the unit boundary at 32 / 33, many units per sublist."""
    sc = BR.stack_scene(n, seed=100 + n)
    img, alphas, radii = _one_hot(sc)
    out = _check_exact(sc, img, radii)
    assert bool((radii > 0).all())
    if n <= 64:   # (the scene is what it claims: every pixel takes every Gaussian; 203 of them saturate the last pixels of the stack)
        assert bool((out["hits"] == BR.W * BR.H).all())


def test_saturated_stack_matches_the_forward_exactly():
    sc = BR.stack_scene(203, seed=7, opacity=(0.6, 0.99))
    img, alphas, radii = _one_hot(sc)
    out = _check_exact(sc, img, radii)
    # every Gaussian reaches alpha >= 1/255 at every pixel, so a pixel that took fewer Gaussians than are visible ended on the stop
    # rule; such a pixel has T just above 1e-4
    taken = (img > 0).sum(dim=-1)
    stopped = (taken < (radii > 0).sum(dim=1)[:, None, None]) & (alphas[..., 0] > 0.99)
    assert stopped.float().mean().item() > 0.5, stopped.float().mean().item()
    assert bool(((radii > 0) & (out["hits"] == 0)).any())   # hidden behind saturated pixels: visible, never taken


def test_sparse_scene_matches_the_forward_exactly():
    sc, dead = BR.sparse_scene(seed=3)
    img, alphas, radii = _one_hot(sc)
    out = _check_exact(sc, img, radii)
    dead = torch.from_numpy(dead).to(dev())
    assert bool((out["hits"] > 0).any()) and bool((radii[:, dead] > 0).any()) and bool((radii[:, dead] <= 0).any())
    for k in ("weight_sum", "weight_max", "hits"):
        assert bool((out[k][:, dead] == 0).all()), k
        assert bool((out[k][radii <= 0] == 0).all()), k


@pytest.mark.parametrize("kw", [dict(rasterize_mode="antialiased"), dict(camera_model="fisheye")], ids=["antialiased", "fisheye"])
def test_other_modes_match_the_forward_exactly(kw):
    sc = BR.stack_scene(33, seed=133)
    img, alphas, radii = _one_hot(sc, **kw)
    _check_exact(sc, img, radii, modes=("gsplat", "tight"), **kw)


def test_activations_see_the_activated_opacity():
    sc = BR.stack_scene(29, seed=129)
    raw = dict(sc, scales=np.log(sc["scales"]), opacities=np.log(sc["opacities"] / (1 - sc["opacities"])).astype(np.float32))
    img, alphas, radii = _one_hot(raw, _activations="exp_sigmoid")
    _check_exact(raw, img, radii, modes=("tight",), _activations="exp_sigmoid")


# ---------------------------------------------------------------------------------------------------------------- 2. identities
def _ordinary():
    if "ordinary" not in _CACHE:
        sc = make_scene(20_000, 256, 192, sh_degree=0, n_views=2, seed=5)
        _CACHE["ordinary"] = (sc, _scores(sc, "tight"))
    return _CACHE["ordinary"]


def test_identities_at_size():
    from easy_gaussian_splatting_amd.rendering import rasterization
    sc, out = _ordinary()
    t = _t(sc)
    C, N, W, H = 2, t["means"].shape[0], sc["width"], sc["height"]
    ones = torch.ones((C, N, 1), device=dev(), requires_grad=True)
    img, alphas, meta = rasterization(*_geom(t), ones, t["viewmats"], t["Ks"], W, H, sh_degree=None, packed=False, _tile_culling="tight")
    (v_ones,) = torch.autograd.grad(img.sum(), [ones])
    # sum_n weight_sum[c, n] = sum_p (1 - T_final): the forward criterion (1e-4 abs per pixel) summed over the image
    e_alpha = (out["weight_sum"].double().sum(dim=1) - alphas.detach().double().sum(dim=(1, 2, 3))).abs().max().item()
    print(f"[blend_weights] sum of weight_sum against sum of render_alphas: {e_alpha:.3e} (bound {1e-4 * H * W:.3e})")
    assert e_alpha <= 1e-4 * H * W
    # weight_sum = the colour gradient of the 1-channel workaround (tests/test_gpu_parity.py: 1e-3 of the tensor's largest magnitude, relative L2 1e-4)
    ref = v_ones[..., 0].double()
    d = (out["weight_sum"].double() - ref).abs()
    e_max, e_l2 = (d.max() / ref.abs().max()).item(), (d.norm() / ref.norm()).item()
    print(f"[blend_weights] weight_sum against the workaround's colour gradient: max {e_max:.3e} l2 {e_l2:.3e}")
    assert e_max <= 1e-3 and e_l2 <= 1e-4
    zero = out["hits"] == 0
    assert torch.equal(zero, out["weight_max"] == 0) and torch.equal(zero, out["weight_sum"] == 0)
    assert bool((out["hits"] >= 0).all()) and 0.0 < out["weight_max"].max().item() <= 0.999
    assert bool((out["hits"][out["radii"] <= 0] == 0).all())
    again = _scores(sc, "tight")
    for k in ("weight_sum", "weight_max", "hits", "radii"):
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k


# ---------------------------------------------------------------------------------------------------------------- 3. accumulator
@pytest.mark.parametrize("fused", [True, False])
def test_accumulator_matches_its_restatement(fused):
    from easy_gaussian_splatting_amd.importance import BlendWeightStats
    g = torch.Generator().manual_seed(4)
    n = 1003
    views = []
    for C in (1, 2, 1):   # three add calls, four cameras
        hits = torch.randint(0, 3000, (C, n), generator=g, dtype=torch.int32) * (torch.rand((C, n), generator=g) < 0.6)
        views.append({"weight_sum": torch.rand((C, n), generator=g) * hits, "weight_max": torch.rand((C, n), generator=g) * (hits > 0),
                      "hits": hits.to(torch.int32), "radii": torch.randint(-1, 20, (C, n), generator=g, dtype=torch.int32)})
    stats = BlendWeightStats(n, dev(), fused=fused)
    for v in views:
        stats.add({k: x.to(dev()) for k, x in v.items()})
    rows = [{k: x[c] for k, x in v.items()} for v in views for c in range(v["hits"].shape[0])]
    s = torch.zeros(n, dtype=torch.float64)
    for r in rows:
        s = s + r["weight_sum"].double()
    assert stats.n_views == 4
    assert stats.weight_sum.dtype == torch.float64 and torch.equal(stats.weight_sum.cpu(), s)
    assert torch.equal(stats.weight_max.cpu(), torch.stack([r["weight_max"] for r in rows]).amax(dim=0))
    assert stats.hits.dtype == torch.int64 and torch.equal(stats.hits.cpu(), torch.stack([r["hits"] for r in rows]).long().sum(dim=0))
    assert torch.equal(stats.views_seen.cpu(), torch.stack([r["radii"] > 0 for r in rows]).sum(dim=0).int())
    assert torch.equal(stats.views_hit.cpu(), torch.stack([r["hits"] > 0 for r in rows]).sum(dim=0).int())
    stats.reset()
    assert stats.n_views == 0 and not bool(stats.hits.any()) and not bool(stats.weight_sum.any())


# ---------------------------------------------------------------------------------------------------------------- 4. prune
def _trained_model(fused):
    """A small model after a few training steps (non-zero moments) and its three views.  Half of the Gaussians lie where no
    view can see them contribute: behind the cameras."""
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
    sc = make_scene(3000, 96, 64, sh_degree=1, n_views=3, seed=9, dist=5.0)
    sc["means"][1::2, 1] += 40.0   # every other Gaussian far above every view's frustum
    d = dev()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    model = GaussianModel(T(sc["means"]), torch.log(T(sc["scales"])), T(sc["quats"]), T(sc["shs"][:, :1]), T(sc["shs"][:, 1:]),
                          torch.logit(T(sc["opacities"]).clamp(1e-4, 1 - 1e-4)), sh_degree=1).to(d)
    build_optimizers(model, 1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2, fused="hip" if fused else None)
    views = [{"w2c": T(sc["viewmats"][c]), "K": T(sc["Ks"][c]), "width": 96, "height": 64} for c in range(3)]
    g = torch.Generator().manual_seed(1)
    targets = [torch.rand((64, 96, 3), generator=g).to(d) for _ in views]
    return model, views, targets


def _render(model, views):
    with torch.no_grad():
        return [model(v, clamp=False)["render_img"].clone() for v in views]


@pytest.mark.parametrize("fused", [True, False], ids=["device", "torch"])
def test_prune_by_hits_keeps_the_renders_bit_for_bit(fused):
    from easy_gaussian_splatting_amd import importance
    from easy_gaussian_splatting_amd.loss import LossComputer
    model, views, targets = _trained_model(fused)
    runner = None
    lc = LossComputer(0.2, clamp_input=True)
    if fused:   # the device path: the steps run captured
        from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
        runner = TrainStepGraph(model, model.optimizer, lc, views[0], targets[0])
        for i in range(3):
            out = runner.step(views[i], targets[i])
        runner.finish()
        assert bool(torch.isfinite(out["loss3"]).all())
    else:
        for i in range(3):
            o = model(views[i], clamp=False)
            lc.get_loss_dict(o["render_img"], targets[i], None)["total"].backward()
            model.update_statistics(views[i], o)
            model.optimizer.step()
            model.optimizer.zero_grad()
    before = _render(model, views)
    stats = importance.collect(model, views)
    assert stats.n_views == 3
    drop = importance.prune_mask(stats, min_views_hit=1)
    assert torch.equal(drop, stats.hits == 0)
    keep = ~drop
    old = {k: getattr(model, k).detach().clone() for k in model.param_names}
    old_m = {k: tuple(x.clone() for x in model._moments(k)) for k in model.param_names}
    assert any(bool(m.any()) for m, _ in old_m.values())   # the moments are not all zero: the steps above ran
    old_s = {k: getattr(model, k).clone() for k in ("grad_norm_accum", "collecting_counts", "max_radii")}
    n_old = model.nbr_gaussians
    info = model.prune(drop)
    n_new = int(keep.sum())
    assert info == {"pruned": n_old - n_new, "n_before": n_old, "train/nbr_gaussians": n_new}
    assert 0.1 * n_old <= info["pruned"] < 0.9 * n_old, info
    assert model.nbr_gaussians == n_new
    for k in model.param_names:
        assert torch.equal(getattr(model, k).detach(), old[k][keep]), k
        m, v = model._moments(k)
        assert torch.equal(m, old_m[k][0][keep]) and torch.equal(v, old_m[k][1][keep]), k
    for k, x in old_s.items():
        assert torch.equal(getattr(model, k), x[keep]), k
    after = _render(model, views)
    for a, b in zip(before, after):   # the contributing entries and their order are unchanged
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (a - b).abs().max().item()
    if runner is not None:
        out = runner.step(views[0], targets[0])   # (N and the parameter storage changed: the runner re-captures, as after densify_and_prune)
        runner.finish()
        assert bool(torch.isfinite(out["loss3"]).all()) and model.nbr_gaussians == n_new and runner.N == n_new
