"""Fused HIP L1 + (1-SSIM) loss (csrc/gs_loss.hip).

The first three tests hold it to the plain-torch restatement of loss.py in fp64, at the project's fixed bounds.  The rest hold
it to the independent fp64 reference of tests/loss_ref.py (direct 11 x 11 window), at edge shapes, around the eight-way XCD
deal of the blocks, in the image regimes training produces, and to the contracts the kernels' comments state: deterministic
sums, every in-image word written, nothing stale read, the slots entries equal to the pointer entries.

Criteria of a case (`_judge`): the fixed bounds (values to 2e-5 * max(1, |ref|), gradient to 1e-3 of its largest entry) AND,
per metric, e_hip <= F * max(e32, floor) where e32 is the error an fp32 evaluation of the restatement leaves on the same
inputs against the same reference, and the floor is the fp32 rounding floor of the computation (loss_ref.VALUE_FLOOR,
loss_ref.GRAD_FLOOR).  The F's below were calibrated once on an MI355X: profiles/loss_parity.json.

Not tested: byte offsets beyond 2^31, which need an image of more than 179 M pixels (the entry points refuse H * W > 2^28).
"""
import os

import numpy as np
import pytest
import torch

import loss_ref as LR
import parity_log
from easy_gaussian_splatting_amd.loss import LossComputer

pytestmark = pytest.mark.gpu

# e_hip <= F * max(e32, floor), one F per metric for all regimes: twice the worst ratio measured over every case of this module
# (profiles/loss_parity.json), rounded up to a power of two, never below 2.  Measured worst ratios beside them.
F_BOUND = {
    "l1": 2.0,         # worst measured 0.024 (test_randomised_loss_configurations[22]): the floor, not e32, is what binds
    "ssim": 8.0,       # worst measured 2.49 (test_regimes_and_options[bright_flat-0.2-binary-True-shape13])
    "total": 8.0,      # worst measured 2.44 (the same case)
    "grad_max": 4.0,   # worst measured 1.77 (test_tile_counts_around_the_xcd_deal[20-24])
    "grad_l2": 16.0,   # worst measured 6.79 (test_edge_shapes_match_fp64_reference[11-300-white_bg-binary]): where render == gt == 1
                       # the true gradient is 0 and the kernel's three maps (each ~1e3) cancel to rounding noise on every flat pixel;
                       # all ratios above 2.3 are white_bg cases, and they grow with the flat share of the image
}


# (129 x 257: 5 x 9 = 45 tiles, not a multiple of the eight XCD runs the blocks are dealt over; 200 x 333: ragged right and bottom tiles)
@pytest.mark.parametrize("H,W,use_mask", [(75, 100, False), (64, 96, True), (33, 45, True), (129, 257, True), (200, 333, False),
                                          (1080, 1920, False), (1080, 1920, True)])
def test_fused_loss_matches_torch(H, W, use_mask):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H * W)
    lowres = torch.rand(H // 4 + 1, W // 4 + 1, 3, generator=g, dtype=torch.float64)
    up = lambda t: torch.nn.functional.interpolate(t.permute(2, 0, 1)[None], size=(H, W), mode="bilinear")[0].permute(1, 2, 0)
    gt = up(lowres).contiguous()
    render = (gt + 0.15 * torch.randn(H, W, 3, generator=g, dtype=torch.float64)).clamp(0, 1).contiguous()
    mask = (torch.rand(H, W, generator=g, dtype=torch.float64) > 0.8).double() if use_mask else None
    # reference: plain torch, fp64, CPU
    r64 = render.clone().requires_grad_(True)
    ref = LossComputer(0.2, fused=False).get_loss_dict(r64, gt, mask)
    (ref["total"] * 1.7).backward()
    # HIP
    r32 = render.float().to(dev).requires_grad_(True)
    out = LossComputer(0.2, fused=True).get_loss_dict(r32, gt.float().to(dev), None if mask is None else mask.float().to(dev))
    (out["total"] * 1.7).backward()
    for k in ("l1", "ssim", "total"):
        assert abs(out[k].item() - ref[k].item()) <= 2e-5 * max(1.0, abs(ref[k].item())), k
    gref = r64.grad.numpy()
    err = np.abs(r32.grad.cpu().numpy() - gref).max()
    assert err <= 1e-3 * np.abs(gref).max(), err


@pytest.mark.parametrize("shape", [(37, 53, 3), (1, 5), (1080, 1920, 3)])
def test_clamp01_matches_torch_clamp(shape):
    from easy_gaussian_splatting_amd.model import clamp01
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(shape, generator=g) * 1.6 - 0.3)
    x.view(-1)[::7] = 0.0   # exact boundaries: aten's clamp passes the gradient at x == 0 and x == 1
    x.view(-1)[3::11] = 1.0
    v = torch.randn(shape, generator=g)
    a = x.clone().to(dev).requires_grad_(True)
    b = x.clone().to(dev).requires_grad_(True)
    ya, yb = clamp01(a), torch.clamp(b, min=0.0, max=1.0)
    assert torch.equal(ya, yb)
    ya.backward(v.to(dev)); yb.backward(v.to(dev))
    assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("use_mask", [False, True])
def test_loss_with_folded_clamp_equals_clamp_then_loss(use_mask):
    """LossComputer(clamp_input=True) on the un-clamped image == torch.clamp(., 0, 1) followed by the loss,
    values and gradient (aten's clamp passes the gradient at exactly 0 and 1)."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    H, W = 70, 93
    gt = torch.rand(H, W, 3, generator=g)
    x = gt + 0.5 * torch.randn(H, W, 3, generator=g)          # a good part lies outside [0, 1]
    x.view(-1)[::13] = 0.0; x.view(-1)[5::17] = 1.0
    mask = (torch.rand(H, W, generator=g) > 0.7).float().to(dev) if use_mask else None
    a = x.clone().to(dev).requires_grad_(True)
    b = x.clone().to(dev).requires_grad_(True)
    la = LossComputer(0.2, clamp_input=True).get_loss_dict(a, gt.to(dev), mask)
    lb = LossComputer(0.2).get_loss_dict(torch.clamp(b, min=0.0, max=1.0), gt.to(dev), mask)
    for k in ("l1", "ssim", "total"):
        assert abs(la[k].item() - lb[k].item()) <= 1e-6 * max(1.0, abs(lb[k].item())), k
    (la["total"] * 1.3).backward(); (lb["total"] * 1.3).backward()
    assert float((a.grad - b.grad).abs().max()) <= 1e-6 * float(b.grad.abs().max())
    outside = (x < 0) | (x > 1)
    assert float(a.grad.cpu()[outside].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# against the independent fp64 reference (tests/loss_ref.py)

_REF_CACHE = {}


def _reference(regime, H, W, seed, mask, lam, clamp, scale):
    """Inputs, fp64 reference and the fp32 restatement's error of a case: computed once on the CPU and left unchanged."""
    key = (regime, H, W, seed, mask, lam, clamp, scale)
    if key not in _REF_CACHE:
        render, gt, m = LR.make_case(regime, H, W, seed, mask)
        ref = LR.ref64(render, gt, m, lam, clamp, scale)
        o32, g32 = LR.restatement32(render, gt, m, lam, clamp, scale)
        _REF_CACHE[key] = (render, gt, m, ref, LR.errors(o32, g32, ref))
    return _REF_CACHE[key]


def _fused(render, gt, m, lam, clamp, scale):
    dev = torch.device("cuda:0")
    r = render.to(dev).requires_grad_(True)
    out = LossComputer(lam, clamp_input=clamp).get_loss_dict(r, gt.to(dev), None if m is None else m.to(dev))
    (out["total"] * scale).backward()
    return {k: out[k].item() for k in ("l1", "ssim", "total")}, r.grad


def _judge(e_hip, e32, ref):
    floor = LR.floors(ref)
    ratio = {k: e_hip[k] / max(e32[k], floor[k]) for k in e_hip}
    parity_log.record(loss_parity={"e_hip": e_hip, "e32": e32, "ratio": ratio})
    print("loss parity:", {k: "%.3g / %.3g = %.3g" % (e_hip[k], e32[k], ratio[k]) for k in e_hip})
    for k in ("l1", "ssim", "total"):
        assert e_hip[k] <= 2e-5 * max(1.0, abs(ref[k])), (k, e_hip[k])
    assert e_hip["grad_max"] <= 1e-3, e_hip["grad_max"]
    for k in e_hip:
        assert ratio[k] <= F_BOUND[k], (k, e_hip[k], e32[k], ratio[k])


def _check(regime, H, W, seed, mask, lam=0.2, clamp=False, scale=1.0):
    render, gt, m, ref, e32 = _reference(regime, H, W, seed, mask, lam, clamp, scale)
    out, grad = _fused(render, gt, m, lam, clamp, scale)
    assert bool(torch.isfinite(grad).all())
    _judge(LR.errors(out, grad, ref), e32, ref)
    return ref, grad


def _check_pure_l1(ref, grad):
    """lambda_ssim = 0: every element is +-(1 - m) v / (3 H W), or exactly 0 where render == gt, where the clamp cuts and where
    the mask is 1.  (Under a fractional mask the sign of a rounded composite within 2^-22 of gt is any of the three: loss_ref.)"""
    g = grad.double().cpu()
    unit, amb = ref["l1_unit"], ref["ambiguous"]
    exp = ref["sign"] * unit
    zero = (exp == 0) & ~amb
    assert bool((g[zero] == 0).all()), "an element that must be exactly zero is not"
    nz = (exp != 0) & ~amb
    assert bool(((g[nz] - exp[nz]).abs() <= 1e-6 * exp[nz].abs()).all())
    if bool(amb.any()):
        d = torch.stack([(g - s * unit).abs() for s in (-1.0, 0.0, 1.0)]).min(0).values
        assert bool((d[amb] <= 1e-6 * unit[amb].abs()).all())


_EDGE_SHAPES = [(11, 11), (11, 12), (12, 11), (16, 16), (32, 32), (33, 33), (37, 37), (38, 38), (42, 43), (43, 33), (64, 64), (65, 96),
                (11, 300), (300, 11)]


@pytest.mark.parametrize("mask", ["none", "binary"])
@pytest.mark.parametrize("regime", ["noisy", "white_bg"])
@pytest.mark.parametrize("H,W", _EDGE_SHAPES)
def test_edge_shapes_match_fp64_reference(H, W, regime, mask):
    """The minimum image (one interior pixel, cnt = 3), last tiles of 1..5 columns or rows (wholly outside the interior), 38 (the
    last tile holds exactly one interior column), one to ten tiles in a row or column."""
    _check(regime, H, W, 100 + H * 7 + W, mask, lam=0.2, scale=1.7)


# the blocks are dealt over eight XCD runs of ceil(nt / 8) tiles: tile counts below, at and above one and two runs' worth, and
# (70 rows) three tile rows
@pytest.mark.parametrize("H,nt", [(20, n) for n in (1, 2, 7, 8, 9, 15, 16, 17, 24, 25)] + [(70, 4), (70, 5)])
def test_tile_counts_around_the_xcd_deal(H, nt):
    _check("noisy", H, 32 * nt - 7, 200 + nt, "frac", lam=0.2, scale=1.7)


# regime, lambda_ssim, mask, clamp_input, (H, W): every pair of options at least once (the first 18 rows are a pairwise cover;
# `unclamped` exists with clamp_input only), then the training configuration of every regime at both sizes and the
# combinations where the kernel has the least room: pure L1 on exact zeros, the converged and flat regimes under masks
_S, _B = (38, 45), (96, 131)
_TABLE = [
    ("white_bg", 0.0, "binary", False, _S), ("noisy", 0.2, "binary", True, _B), ("converged", 1.0, "none", False, _B),
    ("bright_flat", 1.0, "frac", True, _S), ("dark_flat", 0.0, "frac", False, _B), ("dark_flat", 0.2, "none", True, _S),
    ("unclamped", 0.0, "none", True, _S), ("white_bg", 0.2, "frac", False, _B), ("converged", 0.2, "binary", True, _S),
    ("bright_flat", 0.0, "none", False, _B), ("noisy", 1.0, "frac", False, _S), ("unclamped", 1.0, "binary", True, _B),
    ("white_bg", 1.0, "none", True, _B), ("bright_flat", 0.2, "binary", True, _S), ("noisy", 0.0, "none", True, _S),
    ("dark_flat", 1.0, "binary", False, _S), ("converged", 0.0, "frac", True, _S), ("unclamped", 0.2, "frac", True, _S),
    ("noisy", 0.2, "none", True, _S), ("white_bg", 0.2, "none", True, _S), ("converged", 0.2, "none", True, _B),
    ("bright_flat", 0.2, "none", True, _B), ("dark_flat", 0.2, "none", True, _B), ("unclamped", 0.2, "none", True, _B),
    ("noisy", 0.2, "frac", False, _B), ("white_bg", 0.2, "binary", True, _S), ("converged", 0.2, "frac", False, _B),
    ("bright_flat", 0.2, "frac", False, _S), ("dark_flat", 0.2, "binary", False, _B), ("unclamped", 0.2, "binary", True, _S),
    ("white_bg", 0.0, "none", True, _B), ("white_bg", 0.0, "frac", True, _S), ("unclamped", 0.0, "binary", True, _B),
    ("unclamped", 0.0, "frac", True, _B), ("converged", 0.0, "binary", False, _B), ("noisy", 0.0, "frac", True, _B),
    ("white_bg", 1.0, "binary", False, _S), ("converged", 1.0, "frac", True, _S), ("bright_flat", 1.0, "none", False, _S),
    ("dark_flat", 1.0, "frac", True, _B),
]


@pytest.mark.parametrize("regime,lam,mask,clamp,shape", _TABLE)
def test_regimes_and_options(regime, lam, mask, clamp, shape):
    ref, grad = _check(regime, shape[0], shape[1], 300 + shape[0], mask, lam=lam, clamp=clamp, scale=1.7)
    if lam == 0.0:
        _check_pure_l1(ref, grad)


@pytest.mark.parametrize("scale", [1.7, -3.0, 1e4, 0.0])
def test_upstream_gradient(scale):
    if scale != 0.0:
        _check("noisy", 38, 45, 400, "frac", lam=0.2, clamp=True, scale=scale)
        return
    render, gt, m = LR.make_case("noisy", 38, 45, 400, "frac")
    _, grad = _fused(render, gt, m, 0.2, True, 0.0)
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) == 0.0


def fuzz_loss_case(case):
    rs = np.random.RandomState(9000 + case)
    H, W = int(rs.randint(11, 141)), int(rs.randint(11, 141))
    regime = LR.REGIMES[rs.randint(len(LR.REGIMES))]
    mask = LR.MASKS[rs.randint(3)]
    clamp = bool(rs.randint(2)) or regime == "unclamped"
    lam = (0.0, 0.05, 0.2, 0.5, 1.0)[rs.randint(5)]
    scale = float((-1.0) ** rs.randint(2) * 10.0 ** rs.uniform(-2, 4))
    return regime, H, W, 500 + case, mask, lam, clamp, scale


# GS_FUZZ_CASES=N widens the sweep (as tests/test_gpu_parity.py::test_randomised_configurations)
@pytest.mark.parametrize("case", range(int(os.environ.get("GS_FUZZ_CASES", "24"))))
def test_randomised_loss_configurations(case):
    regime, H, W, seed, mask, lam, clamp, scale = fuzz_loss_case(case)
    ref, grad = _check(regime, H, W, seed, mask, lam=lam, clamp=clamp, scale=scale)
    if lam == 0.0:
        _check_pure_l1(ref, grad)


@pytest.mark.parametrize("H,W", [(10, 40), (40, 10), (5, 7)])
def test_images_smaller_than_the_window_are_refused(H, W):
    dev = torch.device("cuda:0")
    r = torch.rand(H, W, 3, device=dev).requires_grad_(True)
    with pytest.raises(ValueError, match="larger than the 11x11 window"):
        LossComputer(0.2).get_loss_dict(r, torch.rand(H, W, 3, device=dev), None)


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries themselves

def _grid(H, W):
    nt = ((W + 31) // 32) * ((H + 31) // 32)
    return 8 * ((nt + 7) // 8)     # loss_grid() of csrc/gs_loss.hip


def _written_words(H, W):
    return 9 * H * W + 2 * _grid(H, W)   # the derivative maps and one (l1, ssim) pair per launched forward block


def _c_inputs(H, W, use_mask, seed):
    dev = torch.device("cuda:0")
    render, gt, m = LR.make_case("unclamped", H, W, seed, "frac" if use_mask else "none")
    vt = torch.tensor([1.3], device=dev)
    return render.to(dev), gt.to(dev), None if m is None else m.to(dev), vt


def _c_run(H, W, render, gt, m, vt, fill, lam=0.2, clamp=1, slots=None):
    """forward + backward through the C ABI with the workspace and v_render pre-filled with `fill` -> (out3, workspace, v_render)"""
    from easy_gaussian_splatting_amd import _native as nat
    L = nat.lib()
    dev = render.device
    n = int(L.gs_loss_workspace_floats(H, W))
    assert n >= _written_words(H, W)
    ws = torch.full((n,), fill, dtype=torch.float32, device=dev)
    out = torch.full((3,), fill, dtype=torch.float32, device=dev)
    v = torch.full((H, W, 3), fill, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    mp = None if m is None else m.data_ptr()
    if slots is None:
        nat.check(L.gs_l1_ssim_fwd(st, H, W, lam, render.data_ptr(), gt.data_ptr(), mp, clamp, ws.data_ptr(), out.data_ptr()), "gs_l1_ssim_fwd")
        nat.check(L.gs_l1_ssim_bwd(st, H, W, lam, render.data_ptr(), gt.data_ptr(), mp, clamp, ws.data_ptr(), vt.data_ptr(), v.data_ptr()),
                  "gs_l1_ssim_bwd")
    else:
        nat.check(L.gs_l1_ssim_fwd_slots(st, H, W, lam, render.data_ptr(), slots.data_ptr(), int(m is not None), clamp, ws.data_ptr(),
                                         out.data_ptr()), "gs_l1_ssim_fwd_slots")
        nat.check(L.gs_l1_ssim_bwd_slots(st, H, W, lam, render.data_ptr(), slots.data_ptr(), clamp, ws.data_ptr(), vt.data_ptr(), v.data_ptr()),
                  "gs_l1_ssim_bwd_slots")
    torch.cuda.synchronize(dev)
    return out, ws, v


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,W", [(38, 45), (129, 257)])
def test_loss_entries_are_bit_reproducible(H, W, use_mask):
    """"Deterministic reduction, no atomics": two calls on the same inputs give the same bits -- the three values, every word of
    the workspace the kernels write, the gradient."""
    args = _c_inputs(H, W, use_mask, 600 + H)
    out_a, ws_a, v_a = _c_run(H, W, *args, fill=0.0)
    out_b, ws_b, v_b = _c_run(H, W, *args, fill=0.0)
    n = _written_words(H, W)
    assert bool(torch.isfinite(out_a).all()) and bool(torch.isfinite(v_a).all()) and float(v_a.abs().max()) > 0
    assert torch.equal(_bits(out_a), _bits(out_b))
    assert torch.equal(_bits(ws_a[:n]), _bits(ws_b[:n]))
    assert torch.equal(_bits(v_a), _bits(v_b))


@pytest.mark.parametrize("H,W", [(11, 11), (33, 45), (38, 70), (20, 281)])
def test_loss_entries_read_nothing_stale_and_write_every_word(H, W):
    """The workspace comes from torch.empty: with it and v_render pre-filled with NaN the results are finite and bit-identical to
    a run on zeros, every in-image word of the three derivative maps of each channel is written, and so is the partial pair of
    every launched block (20 x 281: nine tiles on a grid of sixteen -- seven blocks lie past the end of their XCD's run)."""
    args = _c_inputs(H, W, True, 700 + W)
    out_z, ws_z, v_z = _c_run(H, W, *args, fill=0.0)
    out_n, ws_n, v_n = _c_run(H, W, *args, fill=float("nan"))
    n = _written_words(H, W)
    assert not bool(torch.isnan(ws_n[:9 * H * W]).any()), "a word of the derivative maps was left unwritten"
    assert not bool(torch.isnan(ws_n[9 * H * W:n]).any()), "a launched block's partial pair was left unwritten"
    assert bool(torch.isfinite(out_n).all()) and bool(torch.isfinite(v_n).all())
    assert torch.equal(_bits(out_n), _bits(out_z)) and torch.equal(_bits(v_n), _bits(v_z))
    assert torch.equal(_bits(ws_n[:n]), _bits(ws_z[:n]))


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,W", [(38, 45), (70, 93)])
def test_slots_entries_equal_pointer_entries(H, W, use_mask):
    """gs_l1_ssim_fwd_slots / gs_l1_ssim_bwd_slots read {gt, mask} from a device array (as the captured train step hands them
    over): bit for bit the pointer entries' results, with a mask (has_mask = 1) and without (a null slot, has_mask = 0)."""
    render, gt, m, vt = _c_inputs(H, W, use_mask, 800 + H)
    slots = torch.tensor([gt.data_ptr(), 0 if m is None else m.data_ptr()], dtype=torch.int64, device=render.device)
    out_p, ws_p, v_p = _c_run(H, W, render, gt, m, vt, fill=0.0)
    out_s, ws_s, v_s = _c_run(H, W, render, gt, m, vt, fill=0.0, slots=slots)
    n = _written_words(H, W)
    assert float(v_p.abs().max()) > 0
    assert torch.equal(_bits(out_p), _bits(out_s)) and torch.equal(_bits(ws_p[:n]), _bits(ws_s[:n])) and torch.equal(_bits(v_p), _bits(v_s))
    # and they are the loss: the same values as the autograd binding
    r = render.clone().requires_grad_(True)
    d = LossComputer(0.2, clamp_input=True).get_loss_dict(r, gt, m)
    (d["total"] * 1.3).backward()
    assert torch.equal(torch.stack([d["l1"], d["ssim"], d["total"]]), out_s) and torch.equal(r.grad, v_s)


# ---------------------------------------------------------------------------------------------------------------------------
# the binding's input decisions (loss._fused_inputs; its refusals are tested on the CPU in tests/test_loss_model.py)

@pytest.mark.parametrize("C", [4, 1])
def test_other_channel_counts_take_the_torch_path(C):
    """rasterization() hands out [H, W, D] images with D in 1..4; only D == 3 may reach the three-channel kernels."""
    dev = torch.device("cuda:0")
    H, W = 38, 45
    g = torch.Generator().manual_seed(40 + C)
    gt = torch.rand(H, W, C, generator=g)
    render = (gt + 0.15 * torch.randn(H, W, C, generator=g)).clamp(0, 1)
    m = LR.make_mask("frac", H, W, C)
    ref = LR.ref64(render, gt, m, 0.2, scale=1.7)
    r = render.to(dev).requires_grad_(True)
    out = LossComputer(0.2).get_loss_dict(r, gt.to(dev), m.to(dev))
    (out["total"] * 1.7).backward()
    assert r.grad.shape == (H, W, C)
    e = LR.errors({k: out[k].item() for k in ("l1", "ssim", "total")}, r.grad, ref)
    for k in ("l1", "ssim", "total"):
        assert e[k] <= 2e-5 * max(1.0, abs(ref[k])), (k, e[k])
    assert e["grad_max"] <= 1e-3, e


def test_float64_ground_truth_and_mask_are_cast():
    dev = torch.device("cuda:0")
    render, gt, m = (t.to(dev) for t in LR.make_case("noisy", 38, 45, 50, "frac"))
    res = []
    for g_in, m_in in ((gt, m), (gt.double(), m), (gt, m.double()), (gt.double(), m.double())):
        r = render.clone().requires_grad_(True)
        d = LossComputer(0.2).get_loss_dict(r, g_in, m_in)
        (d["total"] * 1.7).backward()
        res.append((torch.stack([d["l1"], d["ssim"], d["total"]]), r.grad))
    assert float(res[0][1].abs().max()) > 0
    for vals, grad in res[1:]:
        assert torch.equal(_bits(vals), _bits(res[0][0])) and torch.equal(_bits(grad), _bits(res[0][1]))
