#!/usr/bin/env python3
"""Times the three parts of mcmc.MCMCStrategy (inject_noise, relocate, grow) on the device at 1 M Gaussians, SH degree 3, next
to a plain-torch restatement of the same maths written here (float64 where the kernels use it, torch.multinomial / bincount /
boolean indexing with the host reads they need).

Per part: HIP events around one call, three warm calls of each version first, then `--calls` timed calls with the two versions
taking turns; the median, the least and the largest are reported.  relocate and grow change the model, so every call starts from
the same saved state, restored outside the timed window (the population has `--dead` of its Gaussians below min_opacity).
One process, no file read outside the repository, nothing asserted about speed.  Run it under a time limit of its own:

    timeout -k 10 600 python tools/mcmc_time.py --out profiles/mcmc_time.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_RATIO = 51
NAMES = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")


# ---- the plain-torch restatement ----

def torch_rotmat(quats):
    w, x, y, z = torch.nn.functional.normalize(quats, dim=-1).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def torch_noise(p, strength, z):
    """means += strength g(o) R diag(s^2) R^T z, in float64 as the kernel"""
    R = torch_rotmat(p["quats"].double())
    s2 = torch.exp(p["log_scales"].double()) ** 2
    o = torch.sigmoid(p["logit_opacities"].double())
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    y = s2 * torch.einsum("nji,nj->ni", R, z.double())
    p["means"].copy_((p["means"].double() + (strength * gate)[:, None] * torch.einsum("nij,nj->ni", R, y)).float())


def relocation_table(device):
    """T[R, k] = C(R, k+1) (-1)^k / sqrt(k+1): D = sum_k T[R, k] o'^(k+1)"""
    T = torch.zeros((MAX_RATIO + 1, MAX_RATIO), dtype=torch.float64)
    for r in range(1, MAX_RATIO + 1):
        for k in range(r):
            T[r, k] = math.comb(r, k + 1) * (-1.0) ** k / math.sqrt(k + 1)
    return T.to(device)


def torch_relocation_values(o, s, ratio, table):
    r = ratio.clamp(1, MAX_RATIO)
    on = -torch.expm1(torch.log1p(-o) / r.double())
    powers = on[:, None] ** torch.arange(1, MAX_RATIO + 1, device=o.device, dtype=torch.float64)[None, :]
    D = (table[r] * powers).sum(dim=1)
    return on, s * (o / D)[:, None]


def torch_share_out(p, m, v, sampled, counts, min_opacity, table):
    """new opacity / scales of the drawn Gaussians; their moments to zero"""
    src = torch.nonzero(counts).squeeze(1)                                    # host read
    o = torch.sigmoid(p["logit_opacities"][src].double())
    on, sn = torch_relocation_values(o, torch.exp(p["log_scales"][src].double()), counts[src] + 1, table)
    on = on.clamp(min_opacity, 1.0 - 2.0 ** -23)
    p["logit_opacities"][src] = torch.log(on / (1.0 - on)).float()
    p["log_scales"][src] = torch.log(sn).float()
    for name in NAMES:
        m[name][src] = 0
        v[name][src] = 0


def torch_relocate(p, m, v, min_opacity, table, generator):
    o = torch.sigmoid(p["logit_opacities"].double())
    dead = o <= min_opacity
    dead_idx, alive_idx = torch.nonzero(dead).squeeze(1), torch.nonzero(~dead).squeeze(1)   # host reads
    if dead_idx.numel() == 0 or alive_idx.numel() == 0:
        return 0
    sampled = alive_idx[torch.multinomial(o[alive_idx].float(), dead_idx.numel(), replacement=True, generator=generator)]
    counts = torch.bincount(sampled, minlength=o.numel())
    torch_share_out(p, m, v, sampled, counts, min_opacity, table)
    for name in NAMES:
        p[name][dead_idx] = p[name][sampled]
        m[name][dead_idx] = 0
        v[name][dead_idx] = 0
    return dead_idx.numel()


def torch_grow(p, m, v, n_new, min_opacity, table, generator):
    o = torch.sigmoid(p["logit_opacities"].double())
    sampled = torch.multinomial(o.float(), n_new, replacement=True, generator=generator)
    counts = torch.bincount(sampled, minlength=o.numel())
    torch_share_out(p, m, v, sampled, counts, min_opacity, table)
    out = []
    for d in (p, m, v):
        out.append({name: torch.cat([d[name], d[name][sampled] if d is p else torch.zeros_like(d[name][sampled])]) for name in NAMES})
    return out


# ---- the measurement ----

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_time.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=11, help="timed calls per part and version (>= 10)")
    ap.add_argument("--dead", type=float, default=0.05, help="share of Gaussians below min_opacity")
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls: at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_time.py measures on the GPU and found none: nothing measured")
    from easy_gaussian_splatting_amd.mcmc import MCMCStrategy
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
    dev = torch.device("cuda", torch.cuda.current_device())
    n, K, min_opacity = args.n, 16, 0.005
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    logits = r(n) * 2.0
    logits[torch.rand(n, device=dev, generator=g) < args.dead] = -7.0
    saved = {"means": r(n, 3), "log_scales": torch.log(torch.rand(n, 3, device=dev, generator=g) * 0.03 + 0.003), "quats": r(n, 4),
             "sh_0": r(n, 1, 3), "sh_rest": r(n, K - 1, 3) * 0.1, "logit_opacities": logits}
    lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)

    def fresh_strategy():
        model = GaussianModel(**{k: t.clone() for k, t in saved.items()}, sh_degree=3).to(dev)
        opt = build_optimizers(model, *lrs, fused="hip")
        opt.exp_avg.fill_(0.5)
        opt.exp_avg_sq.fill_(0.25)
        return MCMCStrategy(model, cap_max=2 * n, generator=torch.Generator(device=dev).manual_seed(1))

    def fresh_torch():
        p = {k: t.clone() for k, t in saved.items()}
        return p, {k: torch.full_like(t, 0.5) for k, t in p.items()}, {k: torch.full_like(t, 0.25) for k, t in p.items()}

    table = relocation_table(dev)
    tg = torch.Generator(device=dev).manual_seed(2)
    n_new = int(1.05 * n) - n
    res = {"tool": "tools/mcmc_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
           "n": n, "K": K, "calls": args.calls, "dead_share": args.dead, "n_new": n_new, "parts": {}}

    def device_call(part):
        st = fresh_strategy()
        torch.cuda.synchronize(dev)
        return timed({"inject_noise": lambda: st.inject_noise(1e-4), "relocate": st.relocate, "grow": st.grow}[part])

    def torch_call(part):
        p, m, v = fresh_torch()
        torch.cuda.synchronize(dev)
        return timed({"inject_noise": lambda: torch_noise(p, 50.0, torch.randn((n, 3), device=dev, generator=tg)),
                      "relocate": lambda: torch_relocate(p, m, v, min_opacity, table, tg),
                      "grow": lambda: torch_grow(p, m, v, n_new, min_opacity, table, tg)}[part])

    for part in ("inject_noise", "relocate", "grow"):
        for _ in range(3):   # warm: code objects, the allocator
            device_call(part)
            torch_call(part)
        a, b = [], []
        for _ in range(args.calls):   # the two versions take turns
            a.append(device_call(part))
            b.append(torch_call(part))
        row = {"device": summary(a), "torch": summary(b)}
        res["parts"][part] = row
        print(json.dumps({part: row}), flush=True)
    res["note"] = ("every part includes its random draws on both sides (normals; random bits / torch.multinomial); grow includes "
                   "filling the new buffers")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
