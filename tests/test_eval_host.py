"""Held-out evaluation (easy_gaussian_splatting_amd/evaluate.py), host side: the per-pixel SSIM arithmetic of gs_math.h compiled
for the host (tests/hostmath/ssimmath.cpp) against float64, `image_metrics` on CPU tensors against the independent fp64
reference of tests/loss_ref.py, the `Evaluator` loop with a stub model, and the refusals.  Nothing here launches a kernel."""
import ctypes as ct
import math
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import loss_ref as LR
from easy_gaussian_splatting_amd.evaluate import Evaluator, image_metrics, psnr_from_mse

HM = os.path.join(os.path.dirname(__file__), "hostmath")
EPS = 2.0 ** -24   # half an ulp of 1.0: one float32 rounding, relative
C1, C2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))


# ---- the arithmetic ----

@pytest.fixture(scope="module")
def sm():
    so = os.path.join(HM, "libssimmath.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "ssimmath.cpp")], check=True)
    return ct.CDLL(so)


def _host_ssim(sm, mu_x, mu_y, ess, exy):
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (mu_x, mu_y, ess, exy)]
    out = np.zeros_like(a[0])
    sm.sm_ssim_from_moments(a[0].size, *(v.ctypes.data_as(ct.c_void_p) for v in a), out.ctypes.data_as(ct.c_void_p))
    return out


def _ssim64(mu_x, mu_y, ess, exy):
    """The same statement from the same float32 moments in float64 -> (ssim, mm, d2)."""
    mu_x, mu_y, ess, exy = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (mu_x, mu_y, ess, exy))
    mm = mu_x * mu_x + mu_y * mu_y
    d2 = (ess - mm) + C2
    return ((2 * mu_x * mu_y + C1) * (2 * (exy - mu_x * mu_y) + C2)) / ((mm + C1) * d2), mm, d2


def _moments(rng, n, spread):
    """Moments of n random 121-tap windows: pixel values around a per-window level with the given spread."""
    w = LR.window64().reshape(-1).numpy()
    level = rng.uniform(0.02, 0.98, (n, 1))
    x = np.clip(level + spread * rng.standard_normal((n, 121)), 0, 1).astype(np.float32).astype(np.float64)
    y = np.clip(x + spread * rng.standard_normal((n, 121)), 0, 1).astype(np.float32).astype(np.float64)
    return x @ w, y @ w, (x * x + y * y) @ w, (x * y) @ w


def _bound(mm, ess, d2):
    """The float32 evaluation's error against `_ssim64`.  n2 = 2 (exy - mu_x mu_y) + C2 and d2 = (ess - mm) + C2 are differences of
    quantities up to ess + mm, each formed with at most three roundings: absolute error <= 3 eps (ess + mm) each, which SSIM sees
    relative to d2 (n2 <= d2 up to that error); n1 / d1 are sums of positive terms (three roundings each, relative) and the two
    reciprocals, their product, n1 n2 and the last product add one each: 11 eps relative to a value of at most ~1."""
    return EPS * (11.0 + 2 * 3.0 * (ess + mm) / d2)


def test_ssim_from_moments_on_ordinary_windows(sm):
    rng = np.random.default_rng(1)
    mu_x, mu_y, ess, exy = _moments(rng, 4000, 0.15)
    got = _host_ssim(sm, mu_x, mu_y, ess, exy)
    ref, mm, d2 = _ssim64(mu_x, mu_y, ess, exy)
    assert 0.05 < ref.mean() < 0.95 and ref.std() > 0.05
    assert np.all(np.abs(got - ref) <= _bound(mm, np.float32(ess).astype(np.float64), d2) * np.maximum(1.0, np.abs(ref)))


def test_ssim_from_moments_on_flat_windows_where_both_variances_cancel(sm):
    """bright_flat / dark_flat: sigma^2 ~ 1e-6 .. 0 under means up to 1 -- E[xx] + E[yy] - mu^2 cancels to about nothing in front
    of C2 = 9e-4.  The result stays finite, inside SSIM's range and within the cancellation's own bound."""
    rng = np.random.default_rng(2)
    mu_x, mu_y, ess, exy = _moments(rng, 4000, 1e-3)
    got = _host_ssim(sm, mu_x, mu_y, ess, exy)
    ref, mm, d2 = _ssim64(mu_x, mu_y, ess, exy)
    var = np.float32(ess).astype(np.float64) - mm
    assert np.abs(var).max() < 2e-5 and np.isfinite(got).all()
    assert np.all(np.abs(got - ref) <= _bound(mm, np.float32(ess).astype(np.float64), d2))
    # exactly constant windows: both variances are 0 to the rounding of the moments
    c = rng.uniform(0, 1, 500).astype(np.float32)
    c2 = (c.astype(np.float64) ** 2).astype(np.float32)
    got = _host_ssim(sm, c, c, 2 * c2, c2)
    assert np.all(np.abs(got - 1.0) <= 4 * 2 * EPS)


def test_ssim_of_identical_images_is_one_to_four_ulp(sm):
    """x == y: mu_x == mu_y, E[xx] + E[yy] == 2 E[xy] exactly (the window passes keep the factor two exact): numerators and
    denominators are the same floats and only the reciprocals' and the products' roundings are left.  This host build (g++,
    no FMA on its default target) rounds every product on its own; the device build is made to round the same three products
    (`ssim_rounded`) and uses reciprocals instead of divisions -- its own run of this property is in tests/test_gpu_eval.py."""
    rng = np.random.default_rng(3)
    w = LR.window64().reshape(-1).numpy()
    for spread in (0.3, 0.05, 1e-3, 0.0):
        x = np.clip(rng.uniform(0.02, 0.98, (2000, 1)) + spread * rng.standard_normal((2000, 121)), 0, 1)
        mu32, exx = (x @ w).astype(np.float32), ((x * x) @ w).astype(np.float32)
        got = _host_ssim(sm, mu32, mu32, 2 * exx, exx)
        assert np.all(np.abs(got.astype(np.float64) - 1.0) <= 4 * 2 * EPS), (spread, np.abs(got - 1.0).max())


# ---- image_metrics on CPU tensors ----

def _ref_metrics(render, gt, mask, clamp):
    r, g = render.double(), gt.double()
    if clamp:
        r = r.clamp(0.0, 1.0)
    if mask is not None:
        m = mask.double().unsqueeze(2)
        r = m * g + (1.0 - m) * r
    return float(((r - g) ** 2).mean()), float(LR.ssim64(r, g))


# Every regime under every mask at 38 x 45, the size tests/test_gpu_loss.py holds the regimes to the same 2e-5 at; the edge shapes
# (one interior pixel; a last tile of one column; one and two tiles) in the two regimes that module takes them in.  The flat
# regimes are NOT taken at the edge shapes: a float32 window there errs by up to eps (E[xx] + E[yy] + mu^2) / C2 ~ 2e-4 (the
# cancellation `_bound` states), and the bound on the MEAN presupposes the few thousand windows of an image, not six.
_CPU_CASES = [(r, 38, 45, m) for r in LR.REGIMES for m in LR.MASKS] + \
             [(r, H, W, "frac") for r in ("noisy", "white_bg") for H, W in ((11, 11), (11, 12), (33, 33), (42, 43))]


@pytest.mark.parametrize("regime,H,W,mask", _CPU_CASES)
def test_image_metrics_on_cpu_tensors_match_the_fp64_reference(regime, H, W, mask):
    clamp = regime == "unclamped"
    render, gt, m = LR.make_case(regime, H, W, 900 + H, mask)
    mse, ss = _ref_metrics(render, gt, m, clamp)
    got = image_metrics(render, gt, m, clamp_input=clamp)
    assert got.shape == (2,) and got.dtype == torch.float32
    assert abs(float(got[1]) - ss) <= 2e-5, (float(got[1]), ss)
    assert abs(float(got[0]) - mse) <= 1e-5 * mse, (float(got[0]), mse)
    out = torch.full((3, 2), -1.0)
    assert image_metrics(render, gt, m, clamp_input=clamp, out=out[1]) is not None
    assert torch.equal(out[1], got) and bool((out[[0, 2]] == -1.0).all())
    # other float dtypes of gt / mask are cast
    got64 = image_metrics(render, gt.double(), None if m is None else m.double(), clamp_input=clamp)
    assert torch.equal(got64, got)


@pytest.mark.parametrize("C", [1, 4])
def test_other_channel_counts_take_the_same_statement(C):
    H, W = 38, 45
    g = torch.Generator().manual_seed(60 + C)
    gt = torch.rand(H, W, C, generator=g)
    render = (gt + 0.15 * torch.randn(H, W, C, generator=g)).clamp(0, 1)
    m = LR.make_mask("frac", H, W, C)
    mse, ss = _ref_metrics(render, gt, m, False)
    got = image_metrics(render, gt, m)
    assert abs(float(got[1]) - ss) <= 2e-5 and abs(float(got[0]) - mse) <= 1e-5 * mse


def test_psnr_from_mse():
    p = psnr_from_mse(np.array([1.0, 0.01, 0.0, 2.5e-4], dtype=np.float32))
    assert p.dtype == np.float64 and p[0] == 0.0 and abs(p[1] - 20.0) < 1e-6 and np.isinf(p[2]) and p[2] > 0
    assert abs(p[3] - 10.0 * math.log10(1.0 / float(np.float32(2.5e-4)))) < 1e-12


# ---- refusals ----

def test_wrong_shapes_and_devices_are_refused():
    r, g = torch.rand(20, 24, 3), torch.rand(20, 24, 3)
    with pytest.raises(ValueError, match="mask has shape"):
        image_metrics(r, g, torch.ones(24, 20))
    with pytest.raises(ValueError, match="mask has shape"):
        image_metrics(r, g, torch.ones(20, 24, 1))
    with pytest.raises(ValueError, match="gt_img has shape"):
        image_metrics(r, torch.rand(20, 25, 3))
    with pytest.raises(ValueError, match="gt_img is on"):
        image_metrics(r, torch.empty(20, 24, 3, device="meta"))
    with pytest.raises(ValueError, match="mask is on"):
        image_metrics(r, g, torch.empty(20, 24, device="meta"))
    with pytest.raises(ValueError, match="out must be"):
        image_metrics(r, g, out=torch.zeros(3))
    with pytest.raises(ValueError, match=r"\[H, W, C\]"):
        image_metrics(r[None], g[None])
    ev = Evaluator(0, fused=False)
    with pytest.raises(ValueError, match="mask has shape"):
        ev([{"image": g, "mask": torch.ones(24, 20)}], lambda d: {"render_img": r})


def test_the_entry_point_is_declared_and_refuses_bad_sizes_before_a_launch():
    from easy_gaussian_splatting_amd import _native as nat
    P, I = ct.c_void_p, ct.c_int
    assert nat.SIGNATURES["gs_metrics_workspace_floats"] == (ct.c_size_t, [I, I])
    assert nat.SIGNATURES["gs_image_metrics"] == (ct.c_int, [P, I, I, P, P, P, I, P, P])
    L = nat.lib()
    assert L.gs_version() >= 330
    dummy = (ct.c_float * 4)()
    p = ct.addressof(dummy)
    err = lambda: L.gs_last_error().decode()
    for H, W in ((10, 40), (40, 10), (5, 7)):
        assert L.gs_image_metrics(None, H, W, p, p, None, 0, p, p) == -1 and "larger than the 11x11 window" in err()
    assert L.gs_image_metrics(None, 20000, 20000, p, p, None, 0, p, p) == -1 and "too large" in err()
    assert L.gs_image_metrics(None, 16, 1 << 21, p, p, None, 0, p, p) == -1 and "too large" in err()
    for k in (0, 1, 3, 4):   # render, gt, workspace, out2 (the mask may be NULL)
        a = [p, p, None, p, p]
        a[k] = None
        assert L.gs_image_metrics(None, 16, 16, a[0], a[1], a[2], 0, a[3], a[4]) == -1 and "null pointer" in err(), k
    # two floats per LAUNCHED block: the tile count rounded up to the eight XCD runs
    assert L.gs_metrics_workspace_floats(1080, 1920) == 2 * 2040 and L.gs_metrics_workspace_floats(11, 11) == 16
    assert L.gs_metrics_workspace_floats(20, 281) == 2 * 16 and L.gs_metrics_workspace_floats(0, 5) == 0


# ---- the Evaluator loop ----

def _views(n, H=24, W=30, mask=None, seed=5):
    g = torch.Generator().manual_seed(seed)
    views = []
    for i in range(n):
        d = {"K": torch.eye(3), "w2c": torch.eye(4), "height": H, "width": W, "image": torch.rand(H, W, 3, generator=g)}
        if mask == "none":
            d["mask"] = None
        elif mask is not None:
            d["mask"] = mask(i)
        views.append(d)
    return views


def _stub(render):
    return lambda data: {"render_img": render}


def test_evaluator_means_equal_the_hand_computed_means():
    H, W = 24, 30
    render = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(9))
    frac = lambda i: LR.make_mask("frac", H, W, 40 + i)
    views = _views(3, H, W, mask=frac)
    res = Evaluator(0, fused=False)(views, _stub(render))
    per = [_ref_metrics(render, d["image"], d["mask"], False) for d in views]
    psnr = sum(10.0 * math.log10(1.0 / m) for m, _ in per) / 3
    ss = sum(s for _, s in per) / 3
    assert abs(res["psnr"] - psnr) <= 1e-4 and abs(res["ssim"] - ss) <= 2e-5   # (mse to 1e-5 relative is 4.3e-5 dB)
    assert math.isnan(res["lpips"]) and res["fps"] > 0 and res["fps_host"] == res["fps"]   # (CPU tensors: both are the host figure)
    assert not any(k.startswith("render_") for k in res)


def test_a_mask_of_ones_gives_infinite_psnr_and_ssim_one():
    views = _views(2, mask=lambda i: torch.ones(24, 30))
    res = Evaluator(0, fused=False)(views, _stub(torch.rand(24, 30, 3)))
    assert res["psnr"] == math.inf and abs(res["ssim"] - 1.0) <= 4 * 2 * EPS


def test_mask_none_and_mask_absent_behave_alike():
    render = torch.rand(24, 30, 3, generator=torch.Generator().manual_seed(2))
    a = Evaluator(0, fused=False)(_views(3, mask="none"), _stub(render))
    b = Evaluator(0, fused=False)(_views(3, mask=None), _stub(render))
    c = Evaluator(0, fused=False)(_views(3, mask=lambda i: torch.zeros(24, 30)), _stub(render))
    assert a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"] and math.isfinite(a["psnr"])
    assert abs(a["psnr"] - c["psnr"]) <= 1e-4 and abs(a["ssim"] - c["ssim"]) <= 2e-5


@pytest.mark.parametrize("n,k", [(7, 3), (4, 4), (3, 5), (5, 0)])
def test_render_k_are_the_views_the_references_lines_pick(n, k):
    H, W = 24, 30
    render = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3))
    views = _views(n, H, W)
    # the reference's eval.py:32-34
    random.seed(1234)
    picked = list(range(n))
    if len(picked) > k:
        picked = random.sample(picked, k=k)
    random.seed(1234)
    res = Evaluator(k, fused=False)(views, _stub(render))
    keys = sorted(kk for kk in res if kk.startswith("render_"))
    assert keys == [f"render_{j + 1}" for j in range(min(n, k))]
    for j, i in enumerate(sorted(picked)):   # (numbered in loader order, as the reference's render_count)
        got = res[f"render_{j + 1}"]
        assert isinstance(got, np.ndarray) and got.shape == (H, 2 * W, 3)
        assert np.array_equal(got, torch.cat((views[i]["image"], render), dim=1).numpy())


def test_the_lpips_callable_sees_nchw_images_with_the_ground_truth_first():
    H, W = 24, 30
    render = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(4))
    views = _views(3, H, W, mask=lambda i: LR.make_mask("binary", H, W, i))
    seen = []

    def lpips(gt, img):
        seen.append((gt.clone(), img.clone()))
        return torch.tensor(0.25 * len(seen))

    res = Evaluator(0, lpips=lpips, fused=False)(views, _stub(render))
    assert abs(res["lpips"] - 0.5) < 1e-12 and len(seen) == 3
    for d, (gt, img) in zip(views, seen):
        assert gt.shape == img.shape == (1, 3, H, W)
        assert torch.equal(gt[0].permute(1, 2, 0), d["image"])
        m = d["mask"].unsqueeze(2)
        assert torch.equal(img[0].permute(1, 2, 0), m * d["image"] + (1.0 - m) * render)   # the composite, as the reference hands it over


def test_an_empty_loader_raises():
    with pytest.raises(ValueError, match="empty"):
        Evaluator(0, fused=False)([], _stub(torch.rand(24, 30, 3)))


def test_the_package_exports_the_evaluation():
    import easy_gaussian_splatting_amd as pkg
    from easy_gaussian_splatting_amd import evaluate as E
    assert pkg.Evaluator is E.Evaluator and pkg.image_metrics is E.image_metrics and pkg.evaluate_output is E.evaluate_output
