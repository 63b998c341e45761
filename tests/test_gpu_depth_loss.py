"""Depth supervision on the GPU: the kernels of csrc/gs_depth_loss.hip against the fp64 reference (tests/depth_loss_ref.py states the
bounds), `depth_loss.depth_loss` in the eager loop, and `TrainStepGraph(depth=DepthSupervision(...))` against its eager form, against
the eager autograd loop and against the fp64 oracle composed with the reference loss."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_loss_ref as R
import depth_ref as DR
import loss_ref as LR
import test_gpu_train_graph as TGT
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.bilagrid import BilateralGrids
from easy_gaussian_splatting_amd.depth_loss import DepthSupervision, depth_loss
from easy_gaussian_splatting_amd.exposure import ExposureTable
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel
from easy_gaussian_splatting_amd.train_graph import HostFeed, TrainStepGraph
from oracle import torch_oracle as TO

pytestmark = pytest.mark.gpu
GRAD_RTOL = 1e-3   # tests/test_gpu_depth.py's bound on a gradient tensor: of its largest reference magnitude
DEV = torch.device("cuda:0")
LAM = 0.37


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _kernels(H, W, mode, c4, alpha, t, m, v_render, staged=False, slots=False, lam=LAM, loss3_0=0.625):
    """split + finish + join through the C ABI; by value, or (`staged`) from the record gs_depth_step_inputs writes, the mask through
    a {gt, mask} slot pair (`slots`).  Returns the outputs as host arrays."""
    L, st = nat.lib(), torch.cuda.current_stream(DEV).cuda_stream
    p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    f32 = dict(dtype=torch.float32, device=DEV)
    rec = torch.zeros(nat.GS_DEPTH_REC_FLOATS, **f32)
    img3, depth = torch.full((H, W, 3), 7.0, **f32), torch.full((H, W), 7.0, **f32)
    v4, va = torch.full((H, W, 4), 7.0, **f32), torch.full((H, W), 7.0, **f32)
    part = torch.empty(int(L.gs_depth_loss_partials_doubles(H, W)), dtype=torch.float64, device=DEV)
    loss3 = torch.tensor([0.1, 0.2, loss3_0], **f32)
    img_slots = torch.tensor([0, 0 if m is None else m.data_ptr()], dtype=torch.int64, device=DEV) if slots else None
    mi = R.MODES.index(mode)
    a_lam, a_mode, a_target = (0.0, 0, None) if staged else (lam, mi, p(t))   # by value, or all from the record
    if staged:
        nat.check(L.gs_depth_step_inputs(st, lam, mi, p(t), p(rec)), "gs_depth_step_inputs")
    mk = None if slots else p(m)
    nat.check(L.gs_depth_loss_split(st, H, W, p(rec), a_lam, a_mode, a_target, mk, p(img_slots), p(c4), p(alpha), p(img3), p(depth), p(part)), "gs_depth_loss_split")
    nat.check(L.gs_depth_loss_finish(st, H, W, p(rec), lam, int(staged), p(part), p(loss3)), "gs_depth_loss_finish")
    nat.check(L.gs_depth_loss_join(st, H, W, p(rec), a_lam, a_mode, a_target, mk, p(img_slots), p(c4), p(alpha), p(depth), p(v_render), p(v4), p(va)), "gs_depth_loss_join")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(rec=rec, image3=img3, depth=depth, v_colors4=v4, v_alphas=va, loss3=loss3).items()}


def _frame(H, W, mask, seed):
    rng = np.random.default_rng(seed)
    c4, alpha = R.blend_like(rng, H, W)
    d = R.expected_depth32(c4[..., 3], alpha)
    _, t, m = R.make_case(rng, H, W, mask, d=d)
    v_render = (1e-4 * rng.standard_normal((H, W, 3))).astype(np.float32)
    return c4, alpha, d, t, m, v_render


def _check_against_reference(out, mode, c4, alpha, d, t, m, v_render, lam=LAM, loss3_0=0.625):
    assert np.array_equal(out["image3"].view(np.uint32), c4[..., :3].view(np.uint32))          # the RGB plane: the same bits
    assert np.array_equal(out["depth"].view(np.uint32), d.view(np.uint32))                      # an IEEE division
    value, inv_w = out["rec"][nat.GS_DEPTH_REC_VALUE], out["rec"][nat.GS_DEPTH_REC_INV_W]
    ref, bound = R.value64(d, t, m, mode)
    v_acc, v_alpha, b_acc, b_alpha = R.join64(c4[..., 3], alpha, d, t, m, mode, np.float32(lam))
    ratios = {"value": abs(float(value) - ref) / bound, "v_acc": R.worst_ratio(out["v_colors4"][..., 3], v_acc, b_acc),
              "v_alpha": R.worst_ratio(out["v_alphas"], v_alpha, b_alpha)}
    print(f"{d.shape} {mode}: value {value} (ref {ref}), worst |error| / bound {ratios}")
    assert ref > 0 and all(r <= 1.0 for r in ratios.values()), ratios
    assert np.array_equal(out["v_colors4"][..., :3].view(np.uint32), v_render.view(np.uint32))
    assert np.isfinite(out["v_colors4"]).all() and np.isfinite(out["v_alphas"]).all()
    assert not out["v_colors4"][..., 3][v_acc == 0].any() and not out["v_alphas"][v_alpha == 0].any()
    # the total: the product rounded on its own, then one add
    assert out["loss3"][2] == np.float32(np.float32(loss3_0) + np.float32(np.float32(lam) * value)) and out["loss3"][0] == np.float32(0.1)


# ---- 1. kernel level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("H,W", R.FRAMES)
def test_split_loss_and_join_keep_their_bounds_and_their_bits(H, W, mode, mask):
    c4, alpha, d, t, m, v_render = _frame(H, W, mask, 1000 * H + W + (5 if mask else 0))
    args = [_dev(x) for x in (c4, alpha, t, m, v_render)]
    out = _kernels(H, W, mode, *args)
    _check_against_reference(out, mode, c4, alpha, d, t, m, v_render)
    again = _kernels(H, W, mode, *args)
    assert all(np.array_equal(out[k].view(np.uint32), again[k].view(np.uint32)) for k in out)   # no atomics: the same bits


def test_a_frame_beyond_the_block_cap_strides():
    H, W = R.BIG_FRAME
    c4, alpha, d, t, m, v_render = _frame(H, W, True, 77)
    args = [_dev(x) for x in (c4, alpha, t, m, v_render)]
    out = _kernels(H, W, "disparity", *args)
    _check_against_reference(out, "disparity", c4, alpha, d, t, m, v_render)
    again = _kernels(H, W, "disparity", *args)
    assert all(np.array_equal(out[k].view(np.uint32), again[k].view(np.uint32)) for k in out)


@pytest.mark.parametrize("mode", R.MODES)
def test_a_target_without_a_measurement_gives_exact_zeros(mode):
    H, W = 37, 53
    c4, alpha, d, t, m, v_render = _frame(H, W, True, 9)
    for hole in (np.zeros_like(t), np.full_like(t, np.nan), np.full_like(t, -np.inf)):
        out = _kernels(H, W, mode, _dev(c4), _dev(alpha), _dev(hole), _dev(m), _dev(v_render))
        assert out["rec"][nat.GS_DEPTH_REC_VALUE] == 0.0 and out["rec"][nat.GS_DEPTH_REC_INV_W] == 0.0 and out["loss3"][2] == np.float32(0.625)
        assert not out["v_colors4"][..., 3].any() and not out["v_alphas"].any()
        assert np.array_equal(out["v_colors4"][..., :3].view(np.uint32), v_render.view(np.uint32))


@pytest.mark.parametrize("mode", R.MODES)
def test_staged_record_equals_its_by_value_form(mode):
    H, W = 37, 53
    c4, alpha, d, t, m, v_render = _frame(H, W, True, 13)
    args = [_dev(x) for x in (c4, alpha, t, m, v_render)]
    by_value = _kernels(H, W, mode, *args)
    staged = _kernels(H, W, mode, *args, staged=True, slots=True)
    rec = staged["rec"]
    assert rec[nat.GS_DEPTH_REC_LAMBDA] == np.float32(LAM) and rec.view(np.int32)[nat.GS_DEPTH_REC_MODE] == R.MODES.index(mode)
    assert int(rec.view(np.uint64)[nat.GS_DEPTH_REC_TARGET // 2]) == args[2].data_ptr()
    for k in ("image3", "depth", "v_colors4", "v_alphas", "loss3"):
        assert np.array_equal(by_value[k].view(np.uint32), staged[k].view(np.uint32)), k
    assert np.array_equal(by_value["rec"][4:6].view(np.uint32), rec[4:6].view(np.uint32))


def test_kernels_honour_the_step_guard():
    H, W = 11, 13
    c4, alpha, d, t, m, v_render = _frame(H, W, False, 3)
    L = nat.lib()
    info = torch.zeros(nat.GS_INFO_WORDS, dtype=torch.int64, device=DEV)
    info[nat.GS_INFO_FLAGS] = 1   # a tripped guard: every kernel of a voided step is a no-op
    nat.check(L.gs_guard_set(info.data_ptr(), 1, 1), "gs_guard_set")
    try:
        out = _kernels(H, W, "depth", _dev(c4), _dev(alpha), _dev(t), None, _dev(v_render))
    finally:
        L.gs_guard_set(None, 0, 0)
    assert (out["image3"] == 7.0).all() and (out["depth"] == 7.0).all() and (out["v_colors4"] == 7.0).all() and (out["v_alphas"] == 7.0).all()
    assert not out["rec"].any() and out["loss3"][2] == np.float32(0.625)


# ---- 2. eager level ---------------------------------------------------------------------------------------------------------------
def _model_of(sc, sh_degree):
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    m = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=T(sc["shs"][:, :1].copy()),
                      sh_rest=T(sc["shs"][:, 1:].copy()), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=sh_degree,
                      white_background=True).to(DEV)
    data = {"w2c": T(sc["viewmats"][0]).to(DEV), "K": T(sc["Ks"][0]).to(DEV), "width": int(sc["width"]), "height": int(sc["height"])}
    return m, data


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("scene,deg", [("B", 3), ("D", 2)])
def test_eager_depth_loss_against_the_plain_torch_form_in_fp64(scene, deg, mode, mask):
    model, data = _model_of(DR.scene(scene), deg)
    H, W = data["height"], data["width"]
    out = model(data, clamp=False, depth="ED")
    rd = out["render_depth"]
    assert rd.shape == (H, W, 1)
    d_np = rd.detach().cpu().numpy()[..., 0]
    _, t_np, m_np = R.make_case(np.random.default_rng(31), H, W, mask, d=d_np)
    t, m = _dev(t_np), _dev(m_np)
    loss = depth_loss(rd, t, m, mode=mode)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (g_rd,) = torch.autograd.grad(LAM * loss, rd, retain_graph=True)
    d64 = rd.detach().double().requires_grad_(True)
    ref = depth_loss(d64, t.double(), None if m is None else m.double(), mode=mode, fused=False)
    (g_ref,) = torch.autograd.grad(float(np.float32(LAM)) * ref, d64)
    _, vbound = R.value64(d_np, t_np, m_np, mode)
    _, gbound = R.grad64(d_np, t_np, m_np, mode, np.float32(LAM))
    ratios = {"value": abs(float(loss.detach()) - float(ref.detach())) / vbound, "grad": R.worst_ratio(g_rd.cpu().numpy()[..., 0], g_ref.cpu().numpy()[..., 0], gbound)}
    print(f"scene {scene} {mode} mask={mask}: value {float(loss)} (fp64 {float(ref)}), worst |error| / bound {ratios}")
    assert float(ref) > 0 and all(r <= 1.0 for r in ratios.values()), ratios
    assert _same_bits(depth_loss(rd, t, m, mode=mode), loss)   # two runs: the same bits
    # ... and the gradient reaches the means through the expected depth, the blend and the projection
    (LAM * loss).backward()
    g = model.means.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert float(depth_loss(rd.detach(), torch.zeros_like(t), m, mode=mode)) == 0.0


def test_eager_refusals_on_the_device():
    d, t = torch.ones(8, 6, 1, device=DEV), torch.ones(8, 6, device=DEV)
    with pytest.raises(ValueError, match="on cpu"):
        depth_loss(d, t.cpu())
    with pytest.raises(ValueError, match="mask on cpu"):
        depth_loss(d, t, torch.zeros(8, 6))
    with pytest.raises(ValueError, match="gt_depth of shape"):
        depth_loss(d, t.T.contiguous())
    view = torch.ones(8 * 6 + 1, device=DEV)[1:].view(8, 6)   # maps that start 4 bytes into their buffers are copied, not refused
    assert view.data_ptr() % 16 == 4 and float(depth_loss(d * 2, view, mode="depth")) == 1.0
    assert float(depth_loss(view, t * 3, view * 0, mode="depth")) == 2.0


# ---- 3. step level ----------------------------------------------------------------------------------------------------------------
def _targets(make, datas, n, seed=5, sigma=0.02):
    """Depth maps rendered from a perturbed copy of the model, each with a hole of zeros: [H, W] float32 on the device."""
    pm, _ = make()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        pm.means.add_((sigma * torch.randn(pm.means.shape, generator=g)).to(DEV))
        outs = []
        for v in range(n):
            t = pm(datas[v % len(datas)], clamp=False, depth="ED")["render_depth"][..., 0].clone()
            t[30 + 10 * v:60 + 10 * v, 50:120] = 0.0
            outs.append(t.contiguous())
    return outs


def _mask(H=208, W=320):
    mask = torch.zeros((H, W), device=DEV)
    mask[40:90, 100:200] = 1.0
    return mask


def _same_outputs(a, b, what):
    for k in ("loss3", "render_img", "render_depth", "depth_loss"):
        assert _same_bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize("mode,with_mask", [("disparity", False), ("depth", True)])
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_captured_step_equals_its_eager_form(fuse_adam, mode, with_mask):
    dev, make, datas, gts = TGT._setup()
    tg = _targets(make, datas, 3)
    mask = _mask() if with_mask else None
    runs = []
    for use_graph in (True, False):
        m, o = make()
        r = TrainStepGraph(m, o, LossComputer(0.2, clamp_input=True), datas[0], gts[0], mask, use_graph=use_graph, check_every=2,
                           fuse_adam=fuse_adam, depth=DepthSupervision(LAM, mode), gt_depth=tg[0])
        rep = r.report()
        assert rep["depth"] and rep["depth_mode"] == mode and rep["graph"] == use_graph and not rep["rounds"]
        runs.append((m, o, r, []))
    for it in range(5):
        v = it % 3
        for m, o, r, outs in runs:
            m.update_learning_rate(it)
            out = r.step(datas[v], gts[v], mask, gt_depth=None if it == 3 else tg[v])   # (step 3: the previous step's target)
            r.finish()
            outs.append({k: out[k].clone() for k in ("loss3", "render_img", "render_depth", "depth_loss")})
        _same_outputs(runs[0][3][-1], runs[1][3][-1], f"step {it}")
        TGT._assert_same(runs[0][0], runs[0][1], runs[1][0], runs[1][1], f"step {it}")
    o0 = runs[0][3][0]
    assert o0["render_depth"].shape == (208, 320) and o0["render_img"].shape == (208, 320, 3) and o0["depth_loss"].dim() == 0
    assert float(o0["depth_loss"]) > 0 and float(o0["render_depth"].max()) > 1.0


@pytest.mark.parametrize("combo", ["plain", "scale_reg", "mcmc"])
def test_fused_adam_equals_the_gradient_tensors_bit_for_bit(combo):
    dev, make, datas, gts = TGT._setup()
    tg = _targets(make, datas, 3)
    runs = []
    for fuse_adam in (True, False):
        m, o = make()
        kw, lc = {}, LossComputer(0.2, clamp_input=True)
        if combo == "scale_reg":
            m.USE_SCALE_REGULARIZATION, m.MAX_SCALE_RATIO = True, 2.0
            lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05)
        elif combo == "mcmc":
            kw = dict(mcmc=M.MCMCStrategy(m, cap_max=m.nbr_gaussians, noise_lr=5e4, refine_start=10 ** 9, refine_stop=10 ** 9, refine_every=1,
                                          generator=torch.Generator(device=dev).manual_seed(5), noise="counter", seed=2 ** 63 + 12345),
                      mcmc_reg=(0.01, 0.01))
        r = TrainStepGraph(m, o, lc, datas[0], gts[0], check_every=2, fuse_adam=fuse_adam, depth=DepthSupervision(LAM, "disparity"),
                           gt_depth=tg[0], **kw)
        outs = []
        for it in range(4):
            m.update_learning_rate(it)
            out = r.step(datas[it % 3], gts[it % 3], gt_depth=tg[it % 3])
            r.finish()
            outs.append({k: out[k].clone() for k in ("loss3", "render_img", "render_depth", "depth_loss")})
        runs.append((m, o, outs))
    for it in range(4):
        _same_outputs(runs[0][2][it], runs[1][2][it], f"step {it}")
    TGT._assert_same(runs[0][0], runs[0][1], runs[1][0], runs[1][1], combo)


def _oracle_means_grad(model, data, gt, mask, t, mode, lam, lambda_ssim=0.2):
    """d total / d means of the fp64 oracle composed with the reference loss: project, SH, 4-channel blend, expected depth,
    (1 - l) L1 + l (1 - SSIM) on the clamped and masked image, + lam * depth_loss(fused=False)."""
    f64 = lambda x: x.detach().cpu().double()   # noqa: E731
    means = f64(model.means).requires_grad_(True)
    quats, scales, opac = f64(model.quats), f64(model.log_scales).exp(), torch.sigmoid(f64(model.logit_opacities))
    shs = torch.cat([f64(model.sh_0), f64(model.sh_rest)], dim=1)
    V, Ks, W, H = f64(data["w2c"])[None], f64(data["K"])[None], data["width"], data["height"]
    radii, _, depths, _ = TO.project(means, quats, scales, V, Ks, W, H)
    rgb = TO.spherical_harmonics(model.active_sh_degree, means, V, shs, radii)
    bg = torch.cat([f64(model.BACKGROUND), torch.zeros(1, dtype=torch.float64)])[None]
    acc, alpha, _ = TO.rasterization(means, quats, scales, opac, torch.cat([rgb, depths[..., None]], dim=-1), V, Ks, W, H, sh_degree=None,
                                     packed=False, backgrounds=bg)
    img, d = acc[0, ..., :3], acc[0, ..., 3] / alpha[0, ..., 0].clamp(min=1e-10)
    g, mk = f64(gt), f64(mask)
    r = img.clamp(0.0, 1.0)
    r = mk[..., None] * g + (1.0 - mk[..., None]) * r
    total = (1.0 - lambda_ssim) * F.l1_loss(r, g) + lambda_ssim * (1.0 - LR.ssim64(r, g))
    total = total + lam * depth_loss(d, f64(t), mk, mode=mode, fused=False)
    (grad,) = torch.autograd.grad(total, means)
    return grad


@pytest.mark.parametrize("mode", R.MODES)
def test_step_against_the_eager_autograd_loop_and_the_fp64_oracle(mode):
    """Forward: the captured step's render, depth map, depth loss and total equal the eager autograd loop's bit for bit.  Gradient:
    d total / d means of the fuse_adam=False step -- read back from Adam's first moment after the first step, exp_avg = (1 - beta1) g --
    against the fp64 oracle composed with the reference loss, within GRAD_RTOL of the largest reference magnitude.  The pixels within
    1e-4 of a blend discontinuity are masked out of both terms (tests/test_gpu_depth.py zeroes their upstream gradient)."""
    dev, make, datas, gts = TGT._setup(n=1500, W=100, H=80, n_views=1)
    (ma, oa), (mb, ob) = make(), make()
    data, gt = datas[0], gts[0]
    H, W = 80, 100
    tg = _targets(make, datas, 1)[0]
    sc = dict(means=ma.means.detach().cpu().numpy(), quats=ma.quats.detach().cpu().numpy(), scales=ma.scales.detach().cpu().numpy(),
              opacities=ma.opacities.detach().cpu().numpy(), viewmats=data["w2c"].cpu().numpy()[None], Ks=data["K"].cpu().numpy()[None], width=W, height=H)
    rz = DR.razor(sc)[0]
    assert rz.mean() < 0.05, rz.mean()
    mask = torch.from_numpy(rz.astype(np.float32)).to(dev)
    lc = LossComputer(0.2, clamp_input=True)
    lam = float(np.float32(0.05))
    # the eager autograd loop
    out = ma(data, clamp=False, depth="ED")
    loss = lc.get_loss_dict(out["render_img"], gt, mask)
    dl = depth_loss(out["render_depth"], tg, mask, mode=mode)
    total = loss["total"] + lam * dl
    total.backward()
    g_eager = ma.means.grad.clone()
    # the captured step
    r = TrainStepGraph(mb, ob, lc, data, gt, mask, fuse_adam=False, depth=DepthSupervision(lam, mode), gt_depth=tg)
    so = r.step(data, gt, mask, gt_depth=tg)
    r.finish()
    assert _same_bits(so["render_img"], out["render_img"]) and _same_bits(so["render_depth"], out["render_depth"][..., 0])
    assert _same_bits(so["depth_loss"], dl) and _same_bits(so["loss3"][2], total) and _same_bits(so["loss3"][0], loss["l1"])
    assert float(dl) > 0
    b1 = ob.defaults["betas"][0]
    g_step = ob.moments_of(mb.means)[0].double().cpu() / (1.0 - b1)
    g_ref = _oracle_means_grad(ma, data, gt, mask, tg, mode, lam)
    scale = g_ref.abs().max().item()
    rel_step = ((g_step - g_ref).abs().max() / scale).item()
    rel_eager = ((g_eager.double().cpu() - g_ref).abs().max() / scale).item()
    # (how much of it is the depth term's: the same oracle without it)
    g_rgb = _oracle_means_grad(ma, data, gt, mask, tg, mode, 0.0)
    share = ((g_ref - g_rgb).abs().max() / scale).item()
    print(f"{mode}: v_means rel err: step {rel_step:.3g}, eager loop {rel_eager:.3g}; the depth term's share of the largest entry {share:.3g}")
    assert share > 10 * GRAD_RTOL   # the depth term is well above the bound: a step without it would fail
    assert rel_step <= GRAD_RTOL and rel_eager <= GRAD_RTOL, (rel_step, rel_eager)


def test_zero_weight_leaves_the_rgb_step_alone():
    dev, make, datas, gts = TGT._setup()
    tg = _targets(make, datas, 1)
    lc = LossComputer(0.2, clamp_input=True)
    (ma, oa), (mb, ob) = make(), make()
    plain = TrainStepGraph(ma, oa, lc, datas[0], gts[0], check_every=2)
    zero = TrainStepGraph(mb, ob, lc, datas[0], gts[0], check_every=2, depth=DepthSupervision(0.0, "disparity"), gt_depth=tg[0])
    a, b = plain.step(datas[0], gts[0]), zero.step(datas[0], gts[0], gt_depth=tg[0])
    plain.finish(); zero.finish()
    assert _same_bits(a["render_img"], b["render_img"]) and _same_bits(a["loss3"][:2], b["loss3"][:2])
    assert _same_bits(a["loss3"][2], b["loss3"][2]) and float(b["depth_loss"]) > 0   # (0 * value adds an exact zero)
    for k in ma.param_names:   # 3- against 4-channel gradient rows: test_depth_modes_leave_the_rgb_render_alone's bound
        x, y = getattr(ma, k).detach(), getattr(mb, k).detach()
        rel = ((x - y).abs().max() / (x.abs().max() + 1e-30)).item()
        assert rel <= 1e-6, (k, rel)


@pytest.mark.parametrize("with_grids", [False, True])
def test_overflow_replays_the_voided_step_once_with_its_own_target(with_grids):
    """`with_grids`: the same with `bilagrid=` beside `depth=` -- the recovery re-points both at the first skipped step's own inputs
    (its view, step count and rate; its depth target and weight)."""
    dev, make, datas, gts = TGT._setup(n=30000, n_views=3, dist=4.0)
    far = dict(datas[0])
    w2c = far["w2c"].clone()
    w2c[2, 3] += 14.0   # camera pulled back: splats shrink, few intersections
    far["w2c"] = w2c
    tg = _targets(make, datas, 2, sigma=0.05)
    tg[1] = (tg[1] * 1.5).contiguous()   # two targets that pull apart
    seq = [(far, 0), (datas[1], 1), (datas[2], 2), (far, 0), (datas[0], 0), (datas[1], 1)]
    lc = LossComputer(0.2, clamp_input=True)

    def run(first, view, margin, shift):
        m, o = make()
        kw = dict(bilagrid=BilateralGrids(3, 8, 8, 4).to(dev), bilagrid_lr=2e-3) if with_grids else {}
        r = TrainStepGraph(m, o, lc, {**first, "view_index": view} if with_grids else first, gts[0], margin=margin, check_every=4,
                           depth=DepthSupervision(LAM, "disparity"), gt_depth=tg[shift % 2], **kw)
        for it, (d, v) in enumerate(seq):   # no finish() in between: the host keeps enqueueing behind the overflow
            r.lambda_depth = LAM * 0.8 ** it   # schedules: every pending step keeps the weight and the rate it was issued with
            if with_grids:
                r.bilagrid_lr = 2e-3 * 0.8 ** it
            r.step(d, gts[it % 3], gt_depth=tg[(it + shift) % 2], **(dict(view_index=v) if with_grids else {}))
        r.finish()
        return m, o, r

    (mt, ot, rt), (ma, oa, ra) = run(far, 0, 1.02, 0), run(datas[1], 1, 4.0, 0)
    rep = rt.report()
    print(f"[depth step, grids={with_grids}] margin 1.02 overflowed {rep['overflows']} x and replayed {rep['replayed_steps']} steps; "
          f"margin 4 overflowed {ra.report()['overflows']} x")
    # every step applied exactly once: the applied-step count and Adam's step count are the sequence's length, and an overflow replays
    # at most the steps behind the first (whose own view sized the capacities), once each
    assert rep["overflows"] >= 1 and 1 <= rep["replayed_steps"] <= rep["overflows"] * (len(seq) - 1)
    assert rep["steps"] == len(seq) and ot._step == len(seq)
    assert ra.report()["overflows"] == 0 and ra.report()["steps"] == len(seq)
    TGT._assert_same(mt, ot, ma, oa, "replayed != never overflowed")
    if with_grids:
        assert torch.equal(rt.bilagrid.grids.detach(), ra.bilagrid.grids.detach())
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(rt.bilagrid_state, name), getattr(ra.bilagrid_state, name)), name
        assert rt.bilagrid_state.step == ra.bilagrid_state.step == len(seq)
    # ... and the targets matter: the same sequence with the two targets swapped ends elsewhere
    m, _, _ = run(datas[1], 1, 4.0, 1)
    assert not torch.equal(m.means.detach(), ma.means.detach())


@pytest.mark.parametrize("combo", ["mcmc", "scale_reg", "exposure", "bilagrid", "copy_targets"])
def test_combinations_captured_equals_eager_form(combo):
    dev, make, datas, gts = TGT._setup()
    tg = _targets(make, datas, 3)
    runs = []
    for use_graph in (True, False):
        m, o = make()
        kw, lc, view = {}, LossComputer(0.2, clamp_input=True), {}
        if combo == "mcmc":
            kw = dict(mcmc=M.MCMCStrategy(m, cap_max=m.nbr_gaussians, noise_lr=5e4, refine_start=10 ** 9, refine_stop=10 ** 9, refine_every=1,
                                          generator=torch.Generator(device=dev).manual_seed(5), noise="counter", seed=2 ** 63 + 12345),
                      mcmc_reg=(0.01, 0.01))
        elif combo == "scale_reg":
            m.USE_SCALE_REGULARIZATION, m.MAX_SCALE_RATIO = True, 2.0
            lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05)
        elif combo == "exposure":
            kw = dict(exposure=ExposureTable(3).to(dev), exposure_lr=1e-2)
        elif combo == "bilagrid":
            kw = dict(bilagrid=BilateralGrids(3, 8, 8, 4).to(dev), bilagrid_lr=2e-3)
        elif combo == "copy_targets":
            kw = dict(copy_targets=True)
        r = TrainStepGraph(m, o, lc, datas[0], gts[0], _mask(), use_graph=use_graph, check_every=2, depth=DepthSupervision(LAM, "disparity"),
                           gt_depth=tg[0], **kw)
        outs = []
        staging = tg[0].clone()   # (copy_targets: one recycled buffer, overwritten right after the step is issued)
        for it in range(4):
            v = it % 3
            m.update_learning_rate(it)
            if combo in ("exposure", "bilagrid"):
                view = dict(view_index=v)
            target = tg[v]
            if combo == "copy_targets":
                staging.copy_(tg[v])
                target = staging
            out = r.step(datas[v], gts[v], _mask(), gt_depth=target, **view)
            if combo == "copy_targets":
                staging.fill_(float("nan"))
            r.finish()
            outs.append({k: out[k].clone() for k in ("loss3", "render_img", "render_depth", "depth_loss")})
        runs.append((m, o, r, outs))
    for it in range(4):
        _same_outputs(runs[0][3][it], runs[1][3][it], f"{combo} step {it}")
        assert float(runs[0][3][it]["depth_loss"]) > 0 and bool(torch.isfinite(runs[0][3][it]["loss3"]).all())
    TGT._assert_same(runs[0][0], runs[0][1], runs[1][0], runs[1][1], combo)
    if combo == "exposure":
        assert torch.equal(runs[0][2].exposure.affine.detach(), runs[1][2].exposure.affine.detach())
        assert not torch.equal(runs[0][2].exposure.affine.detach()[0, :, :3], torch.eye(3, device=dev))
    if combo == "bilagrid":
        assert torch.equal(runs[0][2].bilagrid.grids.detach(), runs[1][2].bilagrid.grids.detach())


def test_forty_steps_pull_the_depth_loss_down():
    """Means pushed along their view rays: the image barely moves, the depth map does.  Forty captured steps with lambda_depth > 0 end
    below where they started and below the same run at lambda_depth = 0 -- two runs compared, no threshold."""
    dev, make, datas, gts = TGT._setup(n_views=1)
    data = datas[0]
    lc = LossComputer(0.2, clamp_input=True)
    m0, _ = make()
    with torch.no_grad():
        clean = m0(data, clamp=False, depth="ED")
        gt, tg = clean["render_img"].clamp(0, 1).contiguous().clone(), clean["render_depth"][..., 0].contiguous().clone()
    cam = torch.linalg.inv(data["w2c"])[:3, 3]
    final = {}
    for lam in (1.0, 0.0):
        m, o = make()
        with torch.no_grad():
            ray = m.means - cam
            g = torch.Generator().manual_seed(17)
            m.means.add_(ray * (0.05 * torch.randn((ray.shape[0], 1), generator=g)).to(dev))
        r = TrainStepGraph(m, o, lc, data, gt, depth=DepthSupervision(lam, "depth"), gt_depth=tg)
        first = None
        for it in range(40):
            out = r.step(data, gt, gt_depth=tg)
            if it == 0:
                r.finish()
                first = float(out["depth_loss"])
        r.finish()
        final[lam] = (first, float(out["depth_loss"]))
    print(f"depth_loss first -> last: lambda 1: {final[1.0]}, lambda 0: {final[0.0]}")
    assert final[1.0][0] == final[0.0][0] > 0     # the same start
    assert final[1.0][1] < final[1.0][0]          # supervised: below where it started
    assert final[1.0][1] < final[0.0][1]          # ... and below the unsupervised run


def test_runner_refusals_on_the_device():
    dev, make, datas, gts = TGT._setup(n=3000, n_views=1)
    tg = _targets(make, datas, 1)[0]
    lc = LossComputer(0.2, clamp_input=True)
    sup = DepthSupervision(LAM, "disparity")
    m, o = make()
    with pytest.raises(ValueError, match="gt_depth"):
        TrainStepGraph(m, o, lc, datas[0], gts[0], depth=sup)
    with pytest.raises(ValueError, match="gt_depth of shape"):
        TrainStepGraph(m, o, lc, datas[0], gts[0], depth=sup, gt_depth=tg.T.contiguous())
    with pytest.raises(ValueError, match="rounds='on'"):
        TrainStepGraph(m, o, lc, datas[0], gts[0], depth=sup, gt_depth=tg, rounds="on")
    r = TrainStepGraph(m, o, lc, datas[0], gts[0], depth=sup, gt_depth=tg)
    assert r.rounds_mode == "off" and not r.report()["rounds"]
    with pytest.raises(ValueError, match="shape"):
        r.step(datas[0], gts[0], gt_depth=tg[:, :-1])
    with pytest.raises(NotImplementedError, match="depth"):
        HostFeed(r)
    applied = r.report()["steps"]
    r.step(datas[0], gts[0], gt_depth=tg.double())   # another dtype is converted, like gt_img
    r.finish()
    assert r.report()["steps"] == applied + 1
    plain = TrainStepGraph(*make(), lc, datas[0], gts[0])
    with pytest.raises(ValueError, match="without `depth`"):
        plain.step(datas[0], gts[0], gt_depth=tg)
    out = plain.step(datas[0], gts[0])
    assert "render_depth" not in out and "depth_loss" not in out
