"""Independent float64 statement of the L1 + (1 - SSIM) loss for the loss tests, written from the metric and not from
easy_gaussian_splatting_amd/loss.py: the 11 x 11 Gaussian window (sigma 1.5) applied directly as a NON-separable window over
every position where it lies inside the image, K1 = 0.01, K2 = 0.03, data_range = 1, the mean over the (H-10) x (W-10)
interior of all channels; in front of it `clamp(0, 1)` when asked and the mask composite `m * gt + (1 - m) * render`;
`F.l1_loss`; `total = (1 - lambda) l1 + lambda (1 - ssim)`; gradients by autograd.  Plain torch on the CPU.

Also: the seeded image regimes the loss is tested in (`make_case`), the three kinds of mask, and the error metrics.
Everything `make_case` returns is a float32 tensor: the inputs are rounded BEFORE either side sees them, so the reference
and the code under test compute on identical numbers.

The sign of the L1 term.  d|c - gt| / dc = sign(c - gt) jumps at c == gt.  Without a mask, or where the mask is 0 or 1,
c - gt is exact in every precision (c is the input itself, or gt itself), so the sign is not in doubt.  Where 0 < m < 1 the
composite is ROUNDED: in float32 it carries an error of up to four roundings of values in [0, 1] (1 - m, two products, a
sum), 4 * 2^-24, so where |c64 - gt| <= 2^-22 an exact float32 evaluation may see any of -1, 0, +1 -- and where
render == gt, m * gt + (1 - m) * gt need not give gt back in any precision, the reference's included.  `ref64` reports
these elements (`ambiguous`) together with the size of one sign step (`l1_unit`); `resolve_sign` then moves the reference
gradient, on those elements only, to the candidate sign nearest to the gradient under test.  They are a handful per image.
"""
import math

import torch
import torch.nn.functional as F

REGIMES = ("noisy", "white_bg", "converged", "bright_flat", "dark_flat", "unclamped")   # `unclamped`: with clamp_input=True only
MASKS = ("none", "binary", "frac")
SIGN_BAND = 2.0 ** -22
VALUE_FLOOR = 4.8e-7    # four ulps of 1.0: the rounding of per-pixel SSIM values near 1 (times max(1, |ref|))
GRAD_FLOOR = 1e-6       # two 11-tap passes forward and two backward of rounded FMAs: about 16 epsilons, relative


def window64():
    x = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-(x / 1.5) ** 2 / 2.0)
    g = g / g.sum()
    return g[:, None] * g[None, :]


def ssim64(x, y):
    """x, y: [H, W, C] float64 -> mean SSIM over the interior of all channels."""
    C = x.shape[2]
    w = window64()[None, None].expand(C, 1, 11, 11).contiguous()
    win = lambda t: F.conv2d(t.permute(2, 0, 1)[None], w, groups=C)   # no padding: exactly the windows that lie inside the image
    mu_x, mu_y = win(x), win(y)
    s_xx, s_yy, s_xy = win(x * x) - mu_x * mu_x, win(y * y) - mu_y * mu_y, win(x * y) - mu_x * mu_y
    c1, c2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    full = ((2.0 * mu_x * mu_y + c1) * (2.0 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_xx + s_yy + c2))
    assert full.shape[-2:] == (x.shape[0] - 10, x.shape[1] - 10)
    return full.mean()


def ref64(render, gt, mask=None, lambda_ssim=0.2, clamp_input=False, scale=1.0):
    """-> dict: `l1`, `ssim` (= 1 - mean SSIM, as `LossComputer` names it), `total` (floats), `grad` = d (scale * total) / d render,
    `l1_unit` = the size of one sign step of the L1 term per element, `ambiguous` (see the module docstring); float64 tensors."""
    r0 = render.detach().double().requires_grad_(True)
    g = gt.detach().double()
    r = r0.clamp(0.0, 1.0) if clamp_input else r0
    keep = torch.ones_like(g)
    if clamp_input:
        keep = ((r0.detach() >= 0.0) & (r0.detach() <= 1.0)).double()
    if mask is not None:
        m = mask.detach().double().unsqueeze(2)
        r = m * g + (1.0 - m) * r
        keep = keep * (1.0 - m)
        frac = ((m > 0.0) & (m < 1.0)).expand_as(g)
    else:
        frac = torch.zeros_like(g, dtype=torch.bool)
    l1 = F.l1_loss(r, g)
    ssim_loss = 1.0 - ssim64(r, g)
    total = (1.0 - lambda_ssim) * l1 + lambda_ssim * ssim_loss
    (total * scale).backward()
    return {"l1": l1.item(), "ssim": ssim_loss.item(), "total": total.item(), "grad": r0.grad.detach(),
            "l1_unit": keep * (scale * (1.0 - lambda_ssim) / g.numel()), "sign": torch.sign((r - g).detach()),
            "ambiguous": frac & ((r - g).detach().abs() <= SIGN_BAND) & (keep != 0.0)}


def resolve_sign(ref, grad):
    """The reference gradient with, on the `ambiguous` elements only, the sign of the L1 term (-1, 0 or +1) that lies nearest to `grad`."""
    amb = ref["ambiguous"]
    if not bool(amb.any()):
        return ref["grad"]
    g = grad.detach().double().cpu()
    base = ref["grad"] - ref["sign"] * ref["l1_unit"]
    cands = torch.stack([base + s * ref["l1_unit"] for s in (-1.0, 0.0, 1.0)])
    best = cands.gather(0, (cands - g).abs().argmin(0, keepdim=True))[0]
    return torch.where(amb, best, ref["grad"])


def errors(out, grad, ref):
    """Absolute error of each value; gradient max-norm relative to the largest reference entry; gradient relative L2.
    `out`: dict of floats; `grad`: tensor of any float dtype / device."""
    gref = resolve_sign(ref, grad)
    d = grad.detach().double().cpu() - gref
    gmax, gl2 = float(gref.abs().max()), float(gref.norm())
    e = {k: abs(float(out[k]) - ref[k]) for k in ("l1", "ssim", "total")}
    e["grad_max"] = float(d.abs().max()) / gmax if gmax > 0 else float(d.abs().max())
    e["grad_l2"] = float(d.norm()) / gl2 if gl2 > 0 else float(d.norm())
    return e


def floors(ref):
    f = {k: VALUE_FLOOR * max(1.0, abs(ref[k])) for k in ("l1", "ssim", "total")}
    f["grad_max"] = f["grad_l2"] = GRAD_FLOOR
    return f


def restatement32(render, gt, mask=None, lambda_ssim=0.2, clamp_input=False, scale=1.0):
    """The project's plain-torch restatement (`LossComputer(fused=False)`) evaluated in float32 on the CPU: what an fp32
    evaluation of the same metric leaves against `ref64`.  -> (dict of floats, gradient)."""
    from easy_gaussian_splatting_amd.loss import LossComputer
    r = render.detach().float().clone().requires_grad_(True)
    out = LossComputer(lambda_ssim, fused=False, clamp_input=clamp_input).get_loss_dict(r, gt.float(), None if mask is None else mask.float())
    (out["total"] * scale).backward()
    return {k: out[k].item() for k in ("l1", "ssim", "total")}, r.grad


def _texture(H, W, g):
    low = torch.rand(H // 4 + 1, W // 4 + 1, 3, generator=g, dtype=torch.float64)
    return F.interpolate(low.permute(2, 0, 1)[None], size=(H, W), mode="bilinear")[0].permute(1, 2, 0).contiguous()


def make_mask(kind, H, W, seed):
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(1000003 * seed + 17)
    u = torch.rand(H, W, generator=g, dtype=torch.float64)
    if kind == "binary":
        return (u > 0.8).float()                       # 20 % ones
    assert kind == "frac", kind
    pick = torch.rand(H, W, generator=g, dtype=torch.float64)
    u[pick < 0.1] = 0.0                                # a tenth exactly 0, a tenth exactly 1, the rest uniform in [0, 1]
    u[pick > 0.9] = 1.0
    return u.float()


def make_case(regime, H, W, seed, mask="none"):
    """-> (render, gt, mask) float32 CPU tensors [H,W,3], [H,W,3], [H,W] or None."""
    g = torch.Generator().manual_seed(seed)
    N = lambda: torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    U = lambda: torch.rand(H, W, 3, generator=g, dtype=torch.float64)
    if regime == "noisy":
        gt = _texture(H, W, g)
        render = (gt + 0.15 * N()).clamp(0, 1)
    elif regime == "white_bg":           # a Blender frame: the object inside a centred disc, render == gt == 1.0 exactly around it
        tex = _texture(H, W, g)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        inside = (((yy - (H - 1) / 2.0) ** 2 + (xx - (W - 1) / 2.0) ** 2) <= (min(H, W) / 3.0) ** 2)[..., None]
        gt = torch.where(inside, tex, torch.ones_like(tex))
        render = torch.where(inside, (gt + 0.05 * N()).clamp(0, 1), gt)
    elif regime == "converged":
        gt = _texture(H, W, g)
        render = (gt + 1e-3 * N()).clamp(0, 1)
    elif regime == "bright_flat":
        gt = 0.97 + 0.002 * N()
        render = (gt + 0.002 * N()).clamp(0, 1)
    elif regime == "dark_flat":
        gt = 0.004 * U()
        render = gt + 0.004 * U()
    elif regime == "unclamped":
        gt = U()
        render = gt + 0.5 * N()          # a good part lies outside [0, 1]
        render.view(-1)[::13] = 0.0      # exact boundaries: aten's clamp passes the gradient at 0 and at 1
        render.view(-1)[5::17] = 1.0
    else:
        raise ValueError(regime)
    gt = gt.float()
    render = render.float()
    if regime == "white_bg":
        render = torch.where(inside, render, gt)   # (still exactly gt outside after the rounding)
    return render.contiguous(), gt.contiguous(), make_mask(mask, H, W, seed)


def next_pow2(x):
    return 2.0 ** math.ceil(math.log2(x))
