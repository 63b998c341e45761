"""Blend-weight scores, host side: the float64 reference of the definitions (tests/blend_weights_ref.py) tied to the
oracle's CPU render, and the behaviour of importance.py / GaussianModel.prune / rendering.blend_weights that needs no GPU."""
import numpy as np
import pytest
import torch

import blend_weights_ref as BR
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import importance
from easy_gaussian_splatting_amd.importance import BlendWeightStats, prune_mask
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.rendering import blend_weights
from scenes import make_scene

FWD_ATOL = 1e-4   # the project's forward criterion


# ---- the reference against the oracle ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_scene():
    from oracle import c_oracle as CO
    sc = make_scene(400, 72, 56, sh_degree=0, n_views=2, seed=21, scale_range=(0.03, 0.4), dist=4.0)
    rng = np.random.default_rng(2)
    colors = rng.random((400, 3))
    bg = rng.random((2, 3))
    fw = CO.render(sc["means"], sc["quats"], sc["scales"], sc["opacities"], colors, sc["viewmats"], sc["Ks"], 72, 56, sh_degree=None,
                   backgrounds=bg, dtype=np.float64)
    ws = [BR.pixel_weights(fw["means2d"][c], fw["conics"][c], fw["opacities"][c], fw["depths"][c], fw["radii"][c], 72, 56) for c in range(2)]
    return fw, colors, bg, ws


def test_reference_weights_reproduce_the_oracle_image(oracle_scene):
    fw, colors, bg, ws = oracle_scene
    for c, (w, T) in enumerate(ws):
        img = w @ colors + (1.0 - w.sum(axis=-1))[..., None] * bg[c]
        assert np.abs(img - fw["render_colors"][c]).max() <= FWD_ATOL
        assert (w > 0).any(axis=(0, 1)).sum() > 100   # (a scene in which most Gaussians contribute)


def test_reference_weights_sum_to_the_accumulated_opacity(oracle_scene):
    fw, _, _, ws = oracle_scene
    for c, (w, T) in enumerate(ws):
        assert np.abs(w.sum(axis=-1) - (1.0 - T)).max() <= 1e-12
        assert np.abs((1.0 - T) - fw["render_alphas"][c][..., 0]).max() <= FWD_ATOL
        assert T.min() > BR.T_MIN and w.max() <= BR.ALPHA_MAX
        s, m, h = BR.scores_from_weights(w)
        assert ((h == 0) == (m == 0)).all() and ((h == 0) == (s == 0)).all() and (h[fw["radii"][c] <= 0] == 0).all()


def test_reference_stop_rule_and_thresholds():
    """Three pixels' worth of hand arithmetic: a Gaussian below 1/255 is never taken; the pair that would push T to 1e-4 finishes
    the pixel unblended, and everything behind it gets nothing."""
    one = lambda v: np.array([v], dtype=np.float64)
    m2, con, rad = np.tile([[0.5, 0.5]], (4, 1)), np.tile([[1.0, 0.0, 1.0]], (4, 1)), np.full(4, 5)
    w, T = BR.pixel_weights(m2, con, [0.003, 0.999, 0.999, 0.5], [1.0, 2.0, 3.0, 4.0], rad, 1, 1)
    # T: 1 -> (0.003 skipped) -> 1e-3 -> 1e-6 would be <= 1e-4: stop
    assert w[0, 0, 0] == 0 and w[0, 0, 1] == 0.999 and w[0, 0, 2] == 0 and w[0, 0, 3] == 0
    assert np.isclose(T[0, 0], 1e-3) and one(T[0, 0]) > BR.T_MIN


# ---- prune_mask ----------------------------------------------------------------------------------------------------------
def _stats(weight_sum, weight_max, hits, views_hit):
    s = BlendWeightStats(len(weight_sum))
    s.weight_sum = torch.tensor(weight_sum, dtype=torch.float64)
    s.weight_max = torch.tensor(weight_max, dtype=torch.float32)
    s.hits = torch.tensor(hits, dtype=torch.int64)
    s.views_hit = torch.tensor(views_hit, dtype=torch.int32)
    return s


def test_prune_mask_criteria_and_their_or():
    s = _stats([5.0, 0.2, 3.0, 0.0, 9.0], [0.5, 0.01, 0.2, 0.0, 0.03], [50, 2, 30, 0, 90], [3, 1, 2, 0, 3])
    assert prune_mask(s).tolist() == [False] * 5
    assert prune_mask(s, min_weight_max=0.05).tolist() == [False, True, False, True, True]
    assert prune_mask(s, min_views_hit=2).tolist() == [False, True, False, True, False]
    assert prune_mask(s, keep_fraction=0.4).tolist() == [False, True, True, True, False]                       # top 2 by weight_sum
    assert prune_mask(s, keep_fraction=0.4, rank_by="weight_max").tolist() == [False, True, False, True, True]
    assert prune_mask(s, keep_fraction=0.4, rank_by="hits").tolist() == [False, True, True, True, False]
    assert prune_mask(s, min_weight_max=0.05, min_views_hit=3).tolist() == [False, True, True, True, True]                      # OR
    assert prune_mask(s, min_views_hit=2, keep_fraction=0.4, rank_by="weight_max").tolist() == [False, True, False, True, True]  # OR
    assert prune_mask(s, keep_fraction=1.0).tolist() == [False] * 5 and prune_mask(s, keep_fraction=0.0).tolist() == [True] * 5
    assert prune_mask(s, keep_fraction=0.41).tolist() == [False, True, False, True, False]                     # ceil(2.05) = 3 kept
    with pytest.raises(ValueError):
        prune_mask(s, rank_by="opacity")
    with pytest.raises(ValueError):
        prune_mask(s, keep_fraction=1.5)


def test_prune_mask_ties_break_by_lower_index():
    s = _stats([1.0, 2.0, 1.0, 2.0, 1.0, 1.0], [0.1] * 6, [7] * 6, [1] * 6)
    assert prune_mask(s, keep_fraction=0.5).tolist() == [False, False, True, False, True, True]    # 2, 2 and the FIRST of the 1s
    assert prune_mask(s, keep_fraction=0.5, rank_by="hits").tolist() == [False, False, False, True, True, True]
    assert prune_mask(s, keep_fraction=0.5, rank_by="weight_max").tolist() == [False, False, False, True, True, True]


def test_prune_mask_of_empty_stats():
    m = prune_mask(BlendWeightStats(0), min_weight_max=0.1, min_views_hit=1, keep_fraction=0.5)
    assert m.shape == (0,) and m.dtype == torch.bool


# ---- BlendWeightStats on CPU tensors -------------------------------------------------------------------------------------
def test_stats_on_cpu_tensors_against_hand_computed_totals():
    s = BlendWeightStats(3)
    i32, f32 = torch.int32, torch.float32
    s.add({"weight_sum": torch.tensor([[1.5, 0.0, 0.25], [0.5, 0.0, 0.0]], dtype=f32), "weight_max": torch.tensor([[0.5, 0.0, 0.25], [0.125, 0.0, 0.0]], dtype=f32),
           "hits": torch.tensor([[4, 0, 1], [9, 0, 0]], dtype=i32), "radii": torch.tensor([[3, 2, 1], [5, 0, 7]], dtype=i32)})
    s.add({"weight_sum": torch.tensor([[0.0, 0.0, 2.0]], dtype=f32), "weight_max": torch.tensor([[0.0, 0.0, 0.75]], dtype=f32),
           "hits": torch.tensor([[0, 0, 2_000_000_000]], dtype=i32), "radii": torch.tensor([[-1, 0, 1]], dtype=i32)})
    s.add({"weight_sum": torch.tensor([0.0, 0.0, 1.0], dtype=f32), "weight_max": torch.tensor([0.0, 0.0, 0.5], dtype=f32),
           "hits": torch.tensor([0, 0, 2_000_000_000], dtype=i32), "radii": torch.tensor([0, 0, 1], dtype=i32)})   # ([N]: one camera)
    assert s.n_views == 4
    assert s.weight_sum.dtype == torch.float64 and s.weight_sum.tolist() == [2.0, 0.0, 3.25]
    assert s.weight_max.dtype == f32 and s.weight_max.tolist() == [0.5, 0.0, 0.75]
    assert s.hits.dtype == torch.int64 and s.hits.tolist() == [13, 0, 4_000_000_001]   # (beyond int32)
    assert s.views_seen.tolist() == [2, 1, 4] and s.views_hit.tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        s.add({"weight_sum": torch.zeros((1, 4)), "weight_max": torch.zeros((1, 4)), "hits": torch.zeros((1, 4), dtype=i32), "radii": torch.zeros((1, 4), dtype=i32)})
    with pytest.raises(ValueError):
        s.add({"weight_sum": torch.zeros((1, 3)), "weight_max": torch.zeros((1, 3)), "hits": torch.zeros((1, 3)), "radii": torch.zeros((1, 3), dtype=i32)})
    s.reset()
    assert s.n_views == 0 and s.hits.tolist() == [0, 0, 0] and s.weight_sum.tolist() == [0.0, 0.0, 0.0] and s.views_seen.tolist() == [0, 0, 0]


# ---- GaussianModel.prune, torch path -------------------------------------------------------------------------------------
def _cpu_model(n=37, K=4, steps=2):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g)
    m = GaussianModel(means=r(n, 3), log_scales=r(n, 3), quats=r(n, 4), sh_0=r(n, 1, 3), sh_rest=r(n, K - 1, 3), logit_opacities=r(n), sh_degree=1)
    opt = build_optimizers(m, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3)
    for _ in range(steps):   # non-zero moments
        for k in m.param_names:
            getattr(m, k).grad = torch.randn(getattr(m, k).shape, generator=g)
        opt.step()
    m.grad_norm_accum, m.collecting_counts, m.max_radii = torch.rand(n, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g)
    return m, opt


@pytest.mark.parametrize("which", ["some", "none", "all"])
def test_model_prune_on_the_cpu_against_hand_indexing(which):
    m, opt = _cpu_model()
    n = m.nbr_gaussians
    mask = {"some": torch.arange(n) % 3 == 1, "none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool)}[which]
    keep = ~mask
    old = {k: getattr(m, k).detach().clone() for k in m.param_names}
    old_m = {k: tuple(x.clone() for x in m._moments(k)) for k in m.param_names}
    old_s = {k: getattr(m, k).clone() for k in ("grad_norm_accum", "collecting_counts", "max_radii")}
    steps = {k: opt.state[getattr(m, k)]["step"] for k in m.param_names}
    info = m.prune(mask)
    assert info == {"pruned": int(mask.sum()), "n_before": n, "train/nbr_gaussians": int(keep.sum())}
    assert m.nbr_gaussians == int(keep.sum())
    for group, k in zip(opt.param_groups, m.param_names):
        p = getattr(m, k)
        assert group["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert torch.equal(p.detach(), old[k][keep]), k
        assert torch.equal(opt.state[p]["exp_avg"], old_m[k][0][keep]) and torch.equal(opt.state[p]["exp_avg_sq"], old_m[k][1][keep]), k
        assert opt.state[p]["step"] == steps[k] and len(opt.state) == 6
    for k, x in old_s.items():
        assert torch.equal(getattr(m, k), x[keep]), k
    for k in m.param_names:   # the optimizer still steps
        getattr(m, k).grad = torch.ones_like(getattr(m, k))
    opt.step()


def test_model_prune_refusals():
    m, _ = _cpu_model(n=5, steps=0)
    with pytest.raises(ValueError):
        m.prune(torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        m.prune(torch.zeros(5))
    bare = GaussianModel(torch.zeros(2, 3), torch.zeros(2, 3), torch.ones(2, 4), torch.zeros(2, 1, 3), torch.zeros(2, 0, 3), torch.zeros(2), sh_degree=0)
    with pytest.raises(RuntimeError):
        bare.prune(torch.zeros(2, dtype=torch.bool))


def test_distributed_use_is_refused(monkeypatch):
    import easy_gaussian_splatting_amd.model as M
    m, _ = _cpu_model(n=5, steps=0)
    monkeypatch.setattr(importance, "is_distributed", lambda: True)
    monkeypatch.setattr(M, "is_distributed", lambda: True)
    for call in (lambda: importance.collect(m, []), lambda: BlendWeightStats(5).add_view(m, {}), lambda: prune_mask(BlendWeightStats(5)),
                 lambda: m.prune(torch.zeros(5, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="single-process"):
            call()


# ---- rendering.blend_weights: refusals ------------------------------------------------------------------------------------
def _cpu_call(**kw):
    n = 4
    return blend_weights(torch.zeros(n, 3), torch.ones(n, 4), torch.ones(n, 3), torch.ones(n), torch.eye(4)[None], torch.eye(3)[None], 32, 32, **kw)


def test_blend_weights_refusals():
    with pytest.raises(NotImplementedError, match="GPU only"):
        _cpu_call()
    with pytest.raises(NotImplementedError, match="GPU only"):
        _cpu_call(rasterize_mode="antialiased", _activations="exp_sigmoid", _tile_culling="tight", camera_model="pinhole")
    with pytest.raises(NotImplementedError, match="pinhole model only"):
        _cpu_call(rasterize_mode="antialiased", camera_model="fisheye")
    for kw in (dict(camera_model="panorama"), dict(rasterize_mode="smooth"), dict(_activations="softplus"), dict(_tile_culling="loose")):
        with pytest.raises(ValueError):
            _cpu_call(**kw)
    with pytest.raises(TypeError):   # the options are keyword-only
        blend_weights(torch.zeros(4, 3), torch.ones(4, 4), torch.ones(4, 3), torch.ones(4), torch.eye(4)[None], torch.eye(3)[None], 32, 32, 0.01)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_in_the_binding():
    import ctypes as ct
    P = ct.c_void_p
    assert nat.SIGNATURES["gs_blend_scores"] == (ct.c_int, [P, ct.c_int, ct.c_int, ct.c_int, P, P, P, P, ct.c_int64, P, P, P, P, P, ct.c_int64, P])
    assert nat.SIGNATURES["gs_score_reduce"] == (ct.c_int, [P, ct.c_int, ct.c_int64, P, P, P, P, ct.c_int64, P, P, P, P, P, P])
    assert nat.SIGNATURES["gs_score_accumulate"] == (ct.c_int, [P, ct.c_int, ct.c_int64] + [P] * 9)
    assert nat.PARAMS["gs_blend_scores"][-3:] == ["score_rows", "cap_rows", "unit_classes"]
    assert nat.PARAMS["gs_score_accumulate"][-5:] == ["total_weight_sum", "total_weight_max", "total_hits", "views_seen", "views_hit"]
