#!/usr/bin/env python3
"""Times the normal-consistency regulariser (normals.py, csrc/gs_normals.hip) against its plain-torch form on the same buffers.

One process, runs alternating, `--repeats` (3) repeats, HIP events around warm calls (`--calls` (20) back-to-back calls per window
for the sub-millisecond native kernels and `gs_clamp01`), the median reported with min and max.

  gaussians  `gs_gauss_normals_fwd` / `_bwd` at `--gaussians` (1 M) under one camera, next to the torch form: normalise, gather the
             rotation's column along the smallest scale, rotate, flip by the sign of a dot product; its backward by autograd.
  image      `gs_normal_loss_fwd` (+ finish) and `gs_normal_loss_bwd` on a 1080p `RGB+ED` render of `synthetic.make_scene` whose
             colours are the Gaussians' normals, next to `normal_consistency_loss(fused=False)` forward and its autograd backward.
             The bytes the native passes must move (forward: 20 per pixel read; backward: 20 read, 16 written) per second, beside
             what `gs_clamp01` reaches on the same [H, W, 4] image in the same run.
  step       an eager training step (model forward, L1 + SSIM, backward, statistics, fused Adam) at `--step-gaussians` and
             `--step-size`, plain and with the regulariser (the second, normal render included).

Nothing is asserted about speed.  Run it under a time limit of its own:

    timeout -k 10 600 python tools/normals_time.py --out profiles/normals_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, calls=1):
    """ms per call: `calls` back-to-back calls between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def alternate(fns, repeats, calls):
    """{name: stats} of the named calls, run in turn `repeats` times; calls[name] back-to-back calls per window"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn, calls.get(k, 1)))
    return {k: stats(v) for k, v in ms.items()}


def torch_gaussian_normals(means, quats, scales, viewmat):
    """What a caller would write in torch: [N, 3] camera-space normals under one camera, differentiable in quats"""
    q = quats / quats.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    k = scales.argmin(dim=1)
    nw = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1))[..., 0]
    nc = nw @ viewmat[:3, :3].T
    pc = means @ viewmat[:3, :3].T + viewmat[:3, 3]
    return torch.where(((nc * pc).sum(1) > 0)[:, None], -nc, nc)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_time.json"))
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--render-gaussians", type=int, default=200_000)
    ap.add_argument("--step-gaussians", type=int, default=100_000)
    ap.add_argument("--step-size", type=int, nargs=2, default=[800, 800], metavar=("W", "H"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_time.py measures on the GPU and found none: nothing measured")
    from easy_gaussian_splatting_amd import _native as nat
    from easy_gaussian_splatting_amd import normals as NM
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers, clamp01
    from easy_gaussian_splatting_amd.rendering import rasterization
    from easy_gaussian_splatting_amd.synthetic import make_scene
    dev = torch.device("cuda", torch.cuda.current_device())
    L = nat.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    res = {"tool": "tools/normals_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
           "repeats": args.repeats, "calls_per_window": args.calls}

    # ---- the per-Gaussian kernels ----
    N = args.gaussians
    sc = make_scene(N, 64, 64, sh_degree=0, n_views=1, seed=7)
    t = lambda k: torch.from_numpy(sc[k]).to(dev)
    means, quats, scales, vms = t("means"), t("quats"), torch.log(t("scales")), t("viewmats")
    normals, v_normals, v_quats = torch.empty((1, N, 3), device=dev), torch.randn((1, N, 3), device=dev), torch.empty((N, 4), device=dev)
    ptr = lambda x: x.data_ptr()
    qg = quats.clone().requires_grad_(True)
    state = {}

    def torch_fwd():
        state["n"] = torch_gaussian_normals(means, qg, scales, vms[0])

    def torch_bwd():
        qg.grad = None
        state["n"].backward(v_normals[0], retain_graph=True)
    fns = {"fwd_hip": lambda: nat.check(L.gs_gauss_normals_fwd(st, N, 1, ptr(means), ptr(quats), ptr(scales), ptr(vms), ptr(normals)), "fwd"),
           "fwd_torch": torch_fwd,
           "bwd_hip": lambda: nat.check(L.gs_gauss_normals_bwd(st, N, 1, ptr(means), ptr(quats), ptr(scales), ptr(vms), ptr(v_normals), ptr(v_quats)), "bwd"),
           "bwd_torch": torch_bwd}
    g = alternate(fns, args.repeats, {"fwd_hip": args.calls, "bwd_hip": args.calls})
    agree = float((normals[0] - state["n"].detach()).abs().max())
    res["gaussians"] = {"N": N, **g, "fwd_speedup": round(g["fwd_torch"]["ms"] / g["fwd_hip"]["ms"], 2),
                        "bwd_speedup": round(g["bwd_torch"]["ms"] / g["bwd_hip"]["ms"], 2),
                        "fwd_min_bytes_moved": 52 * N, "fwd_gbytes_per_s": round(52 * N / (g["fwd_hip"]["ms"] * 1e-3) / 1e9, 1),
                        "bwd_min_bytes_moved": 68 * N, "bwd_gbytes_per_s": round(68 * N / (g["bwd_hip"]["ms"] * 1e-3) / 1e9, 1),
                        "max_abs_diff_hip_torch": agree}
    print(json.dumps({"gaussians": res["gaussians"]}), flush=True)
    del sc, means, quats, scales, normals, v_normals, v_quats, qg, state

    # ---- the image passes at 1080p ----
    W, H = 1920, 1080
    sc = make_scene(args.render_gaussians, W, H, sh_degree=0, n_views=1, seed=7, scale_range=(0.01, 0.05))
    t = lambda k: torch.from_numpy(sc[k]).to(dev)
    with torch.no_grad():
        nrm = NM.gaussian_normals(t("means"), t("quats"), t("scales"), t("viewmats"))
        img, alphas, _ = rasterization(means=t("means"), quats=t("quats"), scales=t("scales"), opacities=t("opacities"), colors=nrm, sh_degree=None,
                                       viewmats=t("viewmats"), Ks=t("Ks"), width=W, height=H, backgrounds=None, packed=False, render_mode="RGB+ED")
    render4, alphas, K = img[0].contiguous(), alphas[0, ..., 0].contiguous(), t("Ks")[0].contiguous()
    rec = torch.zeros((nat.GS_NORMAL_REC_FLOATS,), device=dev)
    partials = torch.empty((int(L.gs_normal_loss_partials_doubles(H, W)),), dtype=torch.float64, device=dev)
    v_loss, v_render4 = torch.ones((1,), device=dev), torch.empty_like(render4)
    rg = render4.clone().requires_grad_(True)
    state = {}

    def torch_fwd_img():
        state["loss"] = NM.normal_consistency_loss(rg, alphas, K, fused=False)

    def torch_bwd_img():
        rg.grad = None
        state["loss"].backward(retain_graph=True)
    buf = render4.clone()
    fns = {"fwd_hip": lambda: nat.check(L.gs_normal_loss_fwd(st, H, W, ptr(K), 0.5, ptr(render4), ptr(alphas), None, ptr(rec), ptr(partials), None), "fwd"),
           "fwd_torch": torch_fwd_img,
           "bwd_hip": lambda: nat.check(L.gs_normal_loss_bwd(st, H, W, ptr(K), 0.5, 0, ptr(render4), ptr(alphas), None, ptr(rec), ptr(v_loss), ptr(v_render4)), "bwd"),
           "bwd_torch": torch_bwd_img,
           "clamp01": lambda: clamp01(buf)}
    g = alternate(fns, args.repeats, {"fwd_hip": args.calls, "bwd_hip": args.calls, "clamp01": args.calls})
    px = H * W
    rate = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)
    res["image"] = {"view": [H, W], "gaussians": args.render_gaussians, "valid_share": round(float(rec[1]) and 1.0 / float(rec[1]) / px, 4),
                    **g, "fwd_speedup": round(g["fwd_torch"]["ms"] / g["fwd_hip"]["ms"], 2), "bwd_speedup": round(g["bwd_torch"]["ms"] / g["bwd_hip"]["ms"], 2),
                    "fwd_min_bytes_moved": 20 * px, "fwd_gbytes_per_s": rate(20 * px, g["fwd_hip"]["ms"]),
                    "bwd_min_bytes_moved": 36 * px, "bwd_gbytes_per_s": rate(36 * px, g["bwd_hip"]["ms"]),
                    "clamp01_gbytes_per_s": rate(8 * buf.numel(), g["clamp01"]["ms"]),
                    "value_hip": float(rec[0]), "value_torch": float(state["loss"]),
                    "v_render4_max_abs_diff": float((v_render4 - rg.grad).abs().max()), "v_render4_max_abs": float(rg.grad.abs().max())}
    print(json.dumps({"image": res["image"]}), flush=True)
    del sc, render4, alphas, rg, state, buf, v_render4, img, nrm

    # ---- the eager step, plain and regularised ----
    W, H = args.step_size
    sc = make_scene(args.step_gaussians, W, H, sh_degree=3, n_views=1, seed=3, scale_range=(0.01, 0.05))
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    model = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=T(sc["shs"][:, :1].copy()),
                          sh_rest=T(sc["shs"][:, 1:].copy()), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                          white_background=True).to(dev)
    opt = build_optimizers(model, 1e-5, 1e-4, 1e-5, 1e-4, 1e-5, 1e-4, fused="hip")
    lc = LossComputer(0.2, clamp_input=True)
    data = {"w2c": T(sc["viewmats"][0]).to(dev), "K": T(sc["Ks"][0]).to(dev), "width": W, "height": H}
    with torch.no_grad():
        gt = model(data)["render_img"].clone()
    one = torch.ones((), device=dev)

    def step(lam):
        out = model(data, clamp=False)
        total = lc.get_loss_dict(out["render_img"], gt, None)["total"]
        if lam > 0:
            rn = NM.render_normals(model, data)
            total = total + lam * NM.normal_consistency_loss(rn["render4"], rn["alphas"], data["K"])
        total.backward(gradient=one)
        model.update_statistics(data, out)
        opt.step(); opt.zero_grad()
    g = alternate({"plain": lambda: step(0.0), "regularised": lambda: step(0.05)}, args.repeats, {"plain": 5, "regularised": 5})
    res["step"] = {"gaussians": args.step_gaussians, "view": [H, W], "lambda_normal": 0.05, **g,
                   "ratio": round(g["regularised"]["ms"] / g["plain"]["ms"], 3)}
    print(json.dumps({"step": res["step"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
