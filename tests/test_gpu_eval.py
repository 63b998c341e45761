"""Held-out evaluation on the device: gs_image_metrics (csrc/gs_metrics.hip) and the Evaluator built on it.

The kernel is held to the independent fp64 reference of tests/loss_ref.py (direct 11 x 11 window; a float64 mean of squares) in
the form tests/test_gpu_loss.py uses: edge shapes, tile counts around the eight-way XCD deal of the blocks, the image regimes
under the three kinds of mask.  Criteria of a case (`_judge`):

  ssim  within 2e-5 (the project's value bound);
  PSNR  within 1e-3 dB wherever the composite is exact (no mask or a binary one) and the mse is not 0.  A term (c - gt)^2 carries
        three roundings at most (the difference is exact there, the square and the accumulating FMA round); a thread adds at most
        18 of them serially (6 owned rows x 3 channels), then 8 levels of pairwise sums (64 lanes, 4 waves), then the block pairs
        in double: under 130 ulp = 8e-6 relative = 3.4e-5 dB.  The bound leaves a thirtyfold margin;
  and, per metric, e_hip <= F * max(e32, floor): e32 is the error of the float32 plain-torch evaluation (`image_metrics` on CPU
        tensors) of the same inputs against the same reference, the floors are loss_ref.VALUE_FLOOR for ssim and 2^-22 relative
        for the mse.  The F's were calibrated once on an MI355X over every case of this module (profiles/eval_parity.json): twice
        the worst ratio, rounded up to a power of two, never below 2.  Where the reference mse is exactly 0 the ratio is not
        formed: the kernel must return exactly 0.
"""
import math
import random

import numpy as np
import pytest
import torch

import loss_ref as LR
import parity_log
from easy_gaussian_splatting_amd.evaluate import Evaluator, image_metrics, psnr_from_mse

pytestmark = pytest.mark.gpu

MSE_FLOOR = 2.0 ** -22   # relative: four float32 roundings
# e_hip <= F * max(e32, floor): twice the worst ratio measured over every case of this module (profiles/eval_parity.json), rounded
# up to a power of two, never below 2.  Measured worst ratios beside them.
F_BOUND = {
    "ssim": 8.0,   # worst measured 3.31 (test_edge_shapes_match_fp64_reference[11-11-white_bg-frac]: one interior pixel, three windows;
                   # e_hip 1.9e-6 against e32 5.7e-7); next 2.21 (test_edge_shapes_match_fp64_reference[43-33-white_bg-frac]), the rest below 2
    "mse": 2.0,    # worst measured 0.82 (test_regimes_and_masks[converged-frac-shape0]): the float32 torch mean is no better
}

_REF_CACHE = {}


def _ref64(render, gt, m, clamp):
    r, g = render.double(), gt.double()
    if clamp:
        r = r.clamp(0.0, 1.0)
    if m is not None:
        mm = m.double().unsqueeze(2)
        r = mm * g + (1.0 - mm) * r
    return float(((r - g) ** 2).mean()), float(LR.ssim64(r, g))


def _reference(regime, H, W, seed, mask, clamp):
    """Inputs, fp64 reference and the float32 plain-torch evaluation's error of a case: computed once on the CPU, left unchanged."""
    key = (regime, H, W, seed, mask, clamp)
    if key not in _REF_CACHE:
        render, gt, m = LR.make_case(regime, H, W, seed, mask)
        mse, ss = _ref64(render, gt, m, clamp)
        c32 = image_metrics(render, gt, m, clamp_input=clamp)
        e32 = {"mse": abs(float(c32[0]) - mse) / mse if mse > 0 else abs(float(c32[0])), "ssim": abs(float(c32[1]) - ss)}
        _REF_CACHE[key] = (render, gt, m, {"mse": mse, "ssim": ss}, e32)
    return _REF_CACHE[key]


def _hip(render, gt, m, clamp):
    dev = torch.device("cuda:0")
    out = image_metrics(render.to(dev), gt.to(dev), None if m is None else m.to(dev), clamp_input=clamp)
    assert out.device.type == "cuda" and out.shape == (2,)
    return [float(x) for x in out.cpu()]


def _judge(got, ref, e32, mask):
    mse, ss = got
    assert math.isfinite(mse) and math.isfinite(ss) and mse >= 0.0
    e_ssim = abs(ss - ref["ssim"])
    ratio = {"ssim": e_ssim / max(e32["ssim"], LR.VALUE_FLOOR)}
    e_hip = {"ssim": e_ssim}
    if ref["mse"] > 0:
        e_hip["mse"] = abs(mse - ref["mse"]) / ref["mse"]
        ratio["mse"] = e_hip["mse"] / max(e32["mse"], MSE_FLOOR)
    parity_log.record(eval_parity={"e_hip": e_hip, "e32": e32, "ratio": ratio})
    print("eval parity:", {k: "%.3g / %.3g = %.3g" % (e_hip[k], e32[k], ratio[k]) for k in e_hip})
    assert e_ssim <= 2e-5, e_ssim
    if ref["mse"] == 0:
        assert mse == 0.0, mse
    elif mask in ("none", "binary"):
        d_db = abs(float(psnr_from_mse(mse)) - 10.0 * math.log10(1.0 / ref["mse"]))
        assert d_db <= 1e-3, d_db
    for k in ratio:
        assert ratio[k] <= F_BOUND[k], (k, e_hip[k], e32[k], ratio[k])


def _check(regime, H, W, seed, mask, clamp=False):
    render, gt, m, ref, e32 = _reference(regime, H, W, seed, mask, clamp)
    _judge(_hip(render, gt, m, clamp), ref, e32, mask)


# the minimum image (one interior pixel), last tiles of 1..5 columns or rows (wholly outside the interior), 38 (the last tile holds
# exactly one interior column), one to ten tiles in a row or column
_EDGE_SHAPES = [(11, 11), (11, 12), (12, 11), (33, 33), (38, 38), (42, 43), (43, 33), (11, 300), (300, 11)]


@pytest.mark.parametrize("mask", LR.MASKS)
@pytest.mark.parametrize("regime", ["noisy", "white_bg"])
@pytest.mark.parametrize("H,W", _EDGE_SHAPES)
def test_edge_shapes_match_fp64_reference(H, W, regime, mask):
    _check(regime, H, W, 100 + H * 7 + W, mask)


# the blocks are dealt over eight XCD runs of ceil(nt / 8) tiles: tile counts below, at and above one and two runs' worth (9 tiles
# on a grid of 16: seven blocks lie past the end of their run and write zero partials), and (70 rows) three tile rows
@pytest.mark.parametrize("mask", LR.MASKS)
@pytest.mark.parametrize("H,nt", [(20, n) for n in (1, 2, 7, 8, 9, 16, 17)] + [(70, 4)])
def test_tile_counts_around_the_xcd_deal(H, nt, mask):
    _check("noisy", H, 32 * nt - 7, 200 + nt, mask)


# Every regime under every mask at the two sizes tests/test_gpu_loss.py holds the regimes to the same 2e-5 at.  The flat regimes are
# NOT crossed with the edge shapes: a float32 window of a flat bright image errs by up to eps (E[xx] + E[yy] + mu^2) / C2 ~ 2e-4
# in ANY float32 evaluation (the cancellation in front of C2 = 9e-4; tests/test_eval_host.py states the bound per window), and
# the 2e-5 on the MEAN presupposes the thousands of windows of an image, not the three of an 11 x 11 one.
_S, _B = (38, 45), (96, 131)


@pytest.mark.parametrize("shape", [_S, _B])
@pytest.mark.parametrize("mask", LR.MASKS)
@pytest.mark.parametrize("regime", LR.REGIMES)
def test_regimes_and_masks(regime, mask, shape):
    """noisy, white_bg, converged, bright_flat and dark_flat without the clamp; `unclamped` with clamp_input=True."""
    _check(regime, shape[0], shape[1], 300 + shape[0], mask, clamp=regime == "unclamped")


# ---------------------------------------------------------------------------------------------------------------------------
# the C entry itself

def _bits(t):
    return t.view(torch.int32)


def _c_inputs(H, W, use_mask, seed, regime="unclamped"):
    dev = torch.device("cuda:0")
    render, gt, m = LR.make_case(regime, H, W, seed, "frac" if use_mask else "none")
    return render.to(dev), gt.to(dev), None if m is None else m.to(dev)


def _c_run(H, W, render, gt, m, fill, clamp=1):
    """gs_image_metrics through the C ABI with the workspace and out2 pre-filled with `fill` -> (out2, workspace)"""
    from easy_gaussian_splatting_amd import _native as nat
    L = nat.lib()
    dev = render.device
    n = int(L.gs_metrics_workspace_floats(H, W))
    assert n == 2 * 8 * ((((W + 31) // 32) * ((H + 31) // 32) + 7) // 8)
    ws = torch.full((n,), fill, dtype=torch.float32, device=dev)
    out = torch.full((2,), fill, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.check(L.gs_image_metrics(st, H, W, render.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(), clamp, ws.data_ptr(),
                                 out.data_ptr()), "gs_image_metrics")
    torch.cuda.synchronize(dev)
    return out, ws


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,W", [(11, 11), (12, 13), (70, 93)])
def test_identical_images_give_exactly_zero_error_and_ssim_one(H, W, use_mask):
    """render == gt (a binary mask composes it exactly: 1 * gt + 0 * render and 0 * gt + 1 * render): mse == 0.0, and every
    window's numerators equal its denominators bit for bit (gs_math.h: ssim_from_moments rounds the products of the means on
    their own), so SSIM is 1 to the reciprocals' rounding -- on textured, bright and dark images alike, and at 11 x 11 and
    12 x 13 (three and eighteen windows) with no averaging over windows to lean on: fused products would leave up to 7e-5 on a
    window of the bright image."""
    dev = torch.device("cuda:0")
    for regime in ("noisy", "bright_flat", "dark_flat"):
        _, gt, _ = LR.make_case(regime, H, W, 40, "none")
        m = LR.make_mask("binary", H, W, 41).to(dev) if use_mask else None
        out = image_metrics(gt.to(dev).clone(), gt.to(dev), m).cpu()
        assert float(out[0]) == 0.0, regime
        assert abs(float(out[1]) - 1.0) <= LR.VALUE_FLOOR, (regime, float(out[1]))   # four ulps of 1.0
    const = torch.full((H, W, 3), 0.97, device=dev)   # a constant bright image: both variances are 0 to the moments' rounding
    out = image_metrics(const.clone(), const).cpu()
    assert float(out[0]) == 0.0 and abs(float(out[1]) - 1.0) <= LR.VALUE_FLOOR, float(out[1])


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,W", [(38, 45), (129, 257)])
def test_the_entry_is_bit_reproducible_and_reads_nothing_stale(H, W, use_mask):
    """No atomics, fixed-order sums: two calls give the same bits; a workspace pre-filled with NaN gives the bits of one pre-filled
    with zeros, and the pair of every launched block is written (129 x 257: 45 tiles on a grid of 48)."""
    args = _c_inputs(H, W, use_mask, 600 + H)
    out_a, ws_a = _c_run(H, W, *args, fill=0.0)
    out_b, ws_b = _c_run(H, W, *args, fill=0.0)
    out_n, ws_n = _c_run(H, W, *args, fill=float("nan"))
    assert bool(torch.isfinite(out_a).all()) and float(out_a[0]) > 0
    assert torch.equal(_bits(out_a), _bits(out_b)) and torch.equal(_bits(ws_a), _bits(ws_b))
    assert not bool(torch.isnan(ws_n).any()), "a launched block's partial pair was left unwritten"
    assert torch.equal(_bits(out_n), _bits(out_a)) and torch.equal(_bits(ws_n), _bits(ws_a))


@pytest.mark.parametrize("use_mask", [False, True])
def test_clamp_input_equals_clamping_first(use_mask):
    H, W = 70, 93
    render, gt, m = _c_inputs(H, W, use_mask, 77)
    assert float(render.min()) < 0.0 and float(render.max()) > 1.0
    a = image_metrics(render, gt, m, clamp_input=True)
    b = image_metrics(torch.clamp(render, 0.0, 1.0), gt, m, clamp_input=False)
    assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(_bits(a), _bits(image_metrics(render, gt, m, clamp_input=False)))


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,W,regime", [(38, 45, "unclamped"), (129, 257, "unclamped"), (70, 93, "noisy")])
def test_ssim_equals_the_loss_kernels(H, W, regime, use_mask):
    """ssim == 1 - out3[1] of gs_l1_ssim_fwd on the same inputs to 2 ulp of 1.0 (both round a double to float; the loss kernel
    forms 1 - ssim in double first).  The inputs are the loss tests' own (`_c_inputs` of tests/test_gpu_loss.py) and a noisy
    frame.  Per window the two kernels differ in rounding only: the loss kernel's body fuses the products of the means into the
    sums that read them, the metric's function rounds them first (gs_math.h); on textured images that is 1e-7 per window."""
    from easy_gaussian_splatting_amd import _native as nat
    L = nat.lib()
    render, gt, m = _c_inputs(H, W, use_mask, 800 + H, regime)
    dev = render.device
    clamp = int(regime == "unclamped")
    ws = torch.zeros((int(L.gs_loss_workspace_floats(H, W)),), dtype=torch.float32, device=dev)
    out3 = torch.zeros((3,), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.check(L.gs_l1_ssim_fwd(st, H, W, 0.2, render.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(), clamp, ws.data_ptr(),
                               out3.data_ptr()), "gs_l1_ssim_fwd")
    out2 = image_metrics(render, gt, m, clamp_input=bool(clamp))
    assert abs(float(out2[1]) - (1.0 - float(out3[1]))) <= 2 * 2.0 ** -23


@pytest.mark.parametrize("H,W", [(10, 40), (40, 10), (5, 7)])
def test_images_smaller_than_the_window_are_refused(H, W):
    dev = torch.device("cuda:0")
    out = torch.full((2,), -1.0, device=dev)
    with pytest.raises(ValueError, match="larger than the 11x11 window"):
        image_metrics(torch.rand(H, W, 3, device=dev), torch.rand(H, W, 3, device=dev), None, out=out)
    assert bool((out == -1.0).all())   # nothing was launched


def test_the_binding_casts_and_routes_like_the_loss():
    dev = torch.device("cuda:0")
    render, gt, m = (t.to(dev) for t in LR.make_case("noisy", 38, 45, 50, "frac"))
    base = image_metrics(render, gt, m)
    for g_in, m_in in ((gt.double(), m), (gt, m.double()), (gt.double(), m.double())):
        assert torch.equal(_bits(image_metrics(render, g_in, m_in)), _bits(base))
    buf = torch.full((3, 2), -1.0, device=dev)
    assert image_metrics(render, gt, m, out=buf[1]).data_ptr() == buf[1].data_ptr()
    assert torch.equal(_bits(buf[1]), _bits(base)) and bool((buf[[0, 2]] == -1.0).all())
    # other channel counts take the torch path on the device
    one = image_metrics(render[..., :1].contiguous(), gt[..., :1].contiguous(), m).cpu()
    mse1, ss1 = _ref64(render[..., :1].cpu(), gt[..., :1].cpu(), m.cpu(), False)
    assert abs(float(one[1]) - ss1) <= 2e-5 and abs(float(one[0]) - mse1) <= 1e-5 * mse1
    with pytest.raises(ValueError, match="gt_img is on"):
        image_metrics(render, gt.cpu(), m)
    with pytest.raises(ValueError, match="mask has shape"):
        image_metrics(render, gt, m.t().contiguous())


# ---------------------------------------------------------------------------------------------------------------------------
# the Evaluator

LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def _scene(n=2000, W=64, H=48, n_views=4, seed=3):
    """-> (make(perturb) -> (model, optimizer), the views as CPU loader items with targets rendered from a perturbed copy)"""
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
    from easy_gaussian_splatting_amd.synthetic import make_scene
    dev = torch.device("cuda:0")
    sc = make_scene(n, W, H, sh_degree=3, n_views=n_views, seed=seed, scale_range=(0.02, 0.12), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"])

    def make(perturb=0.0):
        g = torch.Generator().manual_seed(5)
        means = T(sc["means"]) + perturb * torch.randn(n, 3, generator=g)
        sh0 = shs[:, :1] + 4 * perturb * torch.randn(n, 1, 3, generator=g)
        m = GaussianModel(means=means, log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=sh0.contiguous(),
                          sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                          white_background=True, means_lr_schedule_max_steps=40).to(dev)
        return m, build_optimizers(m, *LRS, fused="hip")

    target_model, _ = make(0.03)
    views = []
    with torch.no_grad():
        for v in range(n_views):
            d = {"w2c": T(sc["viewmats"][v]).clone(), "K": T(sc["Ks"][v]).clone(), "width": W, "height": H}
            img = target_model({**d, "w2c": d["w2c"].to(dev), "K": d["K"].to(dev)})["render_img"]
            d["image"] = img.cpu().clone()
            d["mask"] = LR.make_mask("binary", H, W, 70 + v) if v % 2 else torch.zeros(H, W)
            views.append(d)
    return make, views


def _fresh(views):
    return [dict(d) for d in views]   # (data_to_device moves a view's tensors in place)


def test_evaluator_fused_equals_unfused_on_a_rendered_scene():
    make, views = _scene()
    model, _ = make()
    model.eval()
    random.seed(7)
    a = Evaluator(2, fused=True)(_fresh(views), model)
    random.seed(7)
    b = Evaluator(2, fused=False)(_fresh(views), model)
    assert 5.0 < a["psnr"] < 60.0 and 0.0 < a["ssim"] < 1.0 and math.isnan(a["lpips"])
    assert abs(a["psnr"] - b["psnr"]) <= 1e-3 and abs(a["ssim"] - b["ssim"]) <= 2e-5
    for r in (a, b):
        assert r["fps"] > 0 and math.isfinite(r["fps"]) and r["fps_host"] > 0 and math.isfinite(r["fps_host"])
        assert sorted(k for k in r if k.startswith("render_")) == ["render_1", "render_2"] and r["render_1"].shape == (48, 128, 3)
    assert np.array_equal(a["render_1"], b["render_1"]) and np.array_equal(a["render_2"], b["render_2"])
    # mask None and mask absent: the same numbers as a mask of zeros
    zeros = [dict(d, mask=torch.zeros(48, 64)) for d in views]
    none = [dict(d, mask=None) for d in views]
    absent = [{k: v for k, v in d.items() if k != "mask"} for d in views]
    rz, rn, ra = (Evaluator(0)(vs, model) for vs in (zeros, none, absent))
    assert rn["psnr"] == ra["psnr"] and rn["ssim"] == ra["ssim"]
    assert abs(rz["psnr"] - rn["psnr"]) <= 1e-3 and abs(rz["ssim"] - rn["ssim"]) <= 2e-5


def test_views_of_different_sizes_share_one_loader():
    """The workspace grows to the largest view; a smaller view behind a larger one reads only what its own call wrote."""
    make, views = _scene()
    model, _ = make()
    dev = torch.device("cuda:0")
    small = dict(views[1])
    small["K"] = views[1]["K"].clone()
    small["K"][:2] *= 0.5
    small["width"], small["height"] = 32, 24
    with torch.no_grad():
        small["image"] = model({**small, "w2c": small["w2c"].to(dev), "K": small["K"].to(dev)})["render_img"].cpu().flip(0).contiguous()
    small["mask"] = torch.zeros(24, 32)
    mixed = [views[0], small, views[2]]
    a = Evaluator(0, fused=True)(_fresh(mixed), model)
    b = Evaluator(0, fused=False)(_fresh(mixed), model)
    assert math.isfinite(a["psnr"]) and abs(a["psnr"] - b["psnr"]) <= 1e-3 and abs(a["ssim"] - b["ssim"]) <= 2e-5
    # ... and in either order
    c = Evaluator(0, fused=True)(_fresh([small, views[0], views[2]]), model)
    assert abs(a["psnr"] - c["psnr"]) <= 1e-9 and abs(a["ssim"] - c["ssim"]) <= 1e-9


def test_evaluation_between_captured_steps_leaves_the_run_bit_identical():
    """12 TrainStepGraph steps with an Evaluator call after steps 4 and 8 (on the caller's stream: the next step waits for it on
    entry) end on the parameters and Adam moments of the same 12 steps without the calls, and each evaluation gives the numbers
    of an evaluator run on a saved copy of the parameters at that step."""
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    make, views = _scene()
    dev = torch.device("cuda:0")
    datas = [{"w2c": d["w2c"].to(dev), "K": d["K"].to(dev), "width": d["width"], "height": d["height"]} for d in views]
    gts = [d["image"].to(dev) for d in views]
    lc = LossComputer(0.2, clamp_input=True)
    ev = Evaluator(0)

    def run(with_eval):
        model, opt = make()
        runner = TrainStepGraph(model, opt, lc, datas[0], gts[0])
        evals, saved = [], []
        for it in range(12):
            model.update_learning_rate(it)
            runner.step(datas[it % 4], gts[it % 4])
            if with_eval and it + 1 in (4, 8):
                saved.append({k: getattr(model, k).detach().clone() for k in model.param_names})
                model.eval()
                evals.append(ev(_fresh(views), model))
                model.train()
        runner.finish()
        assert runner.report()["overflows"] == 0
        return model, opt, evals, saved

    ma, oa, evals, saved = run(True)
    mb, ob, _, _ = run(False)
    for k in ma.param_names:
        assert torch.equal(getattr(ma, k).detach(), getattr(mb, k).detach()), k
        for x, y in zip(oa.moments_of(getattr(ma, k)), ob.moments_of(getattr(mb, k))):
            assert torch.equal(x, y), (k, "moment")
    assert len(evals) == 2 and evals[0]["psnr"] != evals[1]["psnr"]
    for got, params in zip(evals, saved):
        copy, _ = make()
        with torch.no_grad():
            for k, v in params.items():
                getattr(copy, k).copy_(v)
        want = ev(_fresh(views), copy.eval())
        assert got["psnr"] == want["psnr"] and got["ssim"] == want["ssim"]


def test_evaluate_output_reports_both_sets(tmp_path):
    """The reference's eval(): a tiny Blender-layout dataset (64 x 64, 4 train + 2 test views, one train view with a mask), a
    model from 500 points saved the reference's way, a config.yaml -- both sets reported, the repeated train indexes
    de-duplicated, the numbers those of a direct Evaluator call."""
    import os
    import sys
    import yaml
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from make_synthetic_dataset import write_blender
    from easy_gaussian_splatting_amd.checkpoint import load_gaussian_model, save_gaussian_model
    from easy_gaussian_splatting_amd.evaluate import evaluate_output
    from easy_gaussian_splatting_amd.model import GaussianModel
    from easy_gaussian_splatting_amd.scene import Scene, generate_pointcloud
    data, out = tmp_path / "data", tmp_path / "run"
    write_blender(data, n_train=4, n_val=0, n_test=2, size=64, with_masks=True)
    cfg = dict(random_seed=3, device="cuda:0", data=str(data), data_format="blender", output=str(out), total_iterations=10, eval=True,
               eval_split_ratio=0.125, eval_in_val=False, eval_in_test=True, use_masks=True, mask_expand_pixels=0, white_background=True,
               dataloader_workers=0, eval_render_num=3)
    out.mkdir()
    with open(out / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    scene_args = (cfg["data"], "blender", None, 10, True, 0.125, False, True, True, 0, True)
    scene = Scene(*scene_args)
    assert len(scene.train_indexes) == 10 and len(set(scene.train_indexes)) == 4 and len(scene.eval_indexes) == 2
    np.random.seed(0)
    model = GaussianModel.from_pointcloud(generate_pointcloud([scene.frames[i] for i in set(scene.train_indexes)], 500), sh_degree=1,
                                          white_background=True)
    save_gaussian_model(out / "checkpoints" / "iterations_10.pth", model)
    res = evaluate_output(str(out))
    assert sorted(res) == ["eval", "train"]
    loaded = load_gaussian_model(out, 10).eval()
    want = {"train": Evaluator(0)([scene.frames[i].to_data() for i in sorted(set(scene.train_indexes))], loaded),
            "eval": Evaluator(0)([scene.get_data("eval", i) for i in range(2)], loaded)}
    for name in ("train", "eval"):
        r = res[name]
        assert math.isfinite(r["psnr"]) and 0.0 < r["ssim"] < 1.0 and math.isnan(r["lpips"]) and r["fps"] > 0 and r["fps_host"] > 0
        assert not any(k.startswith("render_") for k in r)   # eval_render_num = 0, as the reference sets it
        assert r["psnr"] == want[name]["psnr"] and r["ssim"] == want[name]["ssim"], name
    assert res["train"]["psnr"] != res["eval"]["psnr"]
    # the same through `cfg`, and a run without held-out views reports the train set alone
    again = evaluate_output(str(out), iterations=10, cfg=dict(cfg, eval=False, eval_in_test=False))
    assert sorted(again) == ["train"] and again["train"]["psnr"] == res["train"]["psnr"]
