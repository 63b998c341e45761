"""Torch-side helpers of the refinement tests (tests/test_refine_ref_host.py on the CPU, tests/test_gpu_refine_ref.py on the
device): a model + optimizer that hold exactly the arrays of `refine_ref.make_inputs`, and their state read back."""
import numpy as np
import torch

import refine_ref as RR
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers

LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
STEP = 3   # Adam steps the optimizer has behind it


def draw_noise(inp, device, seed):
    """The split noise exactly as `GaussianModel._split_noise` draws it from a generator seeded with `seed`, put into `inp`
    for the reference; returns the generator to hand to `densify_and_prune`."""
    S, n = inp["num_splits"], len(inp["counts"])
    inp["noise"] = torch.randn((S, n, 3), device=device, generator=torch.Generator(device=device).manual_seed(seed)).cpu().numpy()
    return torch.Generator(device=device).manual_seed(seed)


def build_model(inp, device="cpu", fused=None):
    """A model + optimizer holding exactly `inp`: parameters, both Adam moments (STEP steps behind them), statistics."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())
    th, P = inp["thresholds"], inp["params"]
    m = GaussianModel(**{k: T(P[k]) for k in RR.PARAM_NAMES}, sh_degree=int(round(inp["K"] ** 0.5)) - 1,
                      densify_grad_thresh=th["densify_grad"], densify_scale_thresh=th["densify_scale"], num_splits=inp["num_splits"],
                      prune_radii_ratio_thresh=th["prune_radii"], prune_scale_thresh=th["prune_scale"], min_opacity=th["min_opacity"]).to(device)
    opt = build_optimizers(m, *LRS, fused=fused)
    for name in RR.PARAM_NAMES:
        p = getattr(m, name)
        assert np.array_equal(p.detach().cpu().numpy().view(np.uint32), P[name].view(np.uint32))
        if fused == "hip":
            mom = opt.moments_of(p)
            mom[0].copy_(T(inp["exp_avg"][name])); mom[1].copy_(T(inp["exp_avg_sq"][name]))
        else:
            opt.state[p] = {"step": torch.tensor(float(STEP)), "exp_avg": T(inp["exp_avg"][name]).to(device),
                            "exp_avg_sq": T(inp["exp_avg_sq"][name]).to(device)}
    if fused == "hip":
        opt._step = STEP
    m.grad_norm_accum, m.collecting_counts, m.max_radii = (T(inp[k]).to(device) for k in ("grad_norm_accum", "counts", "max_radii"))
    return m, opt


def state_of(m, info=None, flags=None, counters=None):
    """What compare_refine takes, read from a model."""
    N = lambda t: t.detach().cpu().numpy()
    out = {"params": {k: N(getattr(m, k)) for k in RR.PARAM_NAMES}, "exp_avg": {}, "exp_avg_sq": {}, "tb_info": info,
           "flags": flags, "counters": counters}
    for k in RR.PARAM_NAMES:
        a, b = m._moments(k)
        out["exp_avg"][k], out["exp_avg_sq"][k] = N(a), N(b)
    return out
