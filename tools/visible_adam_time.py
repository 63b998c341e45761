#!/usr/bin/env python3
"""What updating only the visible Gaussians costs and returns: `tools/visible_adam_time.py [steps] [warmup] [--reps R] [--calls N]
[--out FILE]`, one process, dense and selective alternating.

1. the stand-alone kernel: gs_adam_step against gs_adam_step_visible (`FusedAdam.step(visible=...)`) at 1 M Gaussians, SH3 (59 floats
   per Gaussian), visible share 100 / 50 / 25 / 10 / 0 %, the visible rows scattered at random and as one contiguous range -- HIP events
   around `--calls` calls enqueued back to back, median / least / largest over seven windows;
2. the fused kernel: gs_project_bwd_adam against gs_project_bwd_selective on the buffers a finished captured step left (one depth
   round), on the bench scene (`config_bench_1m`) and on `synthetic.config_heavy`, with the visible share of that step's view;
3. the captured step (TrainStepGraph defaults, hipGraph replay, 8 shuffled views) without and with `visible_adam=True` on both scenes,
   `--reps` times each, each from a fresh model of the same seed -- wall clock per step between synchronisations, like bench.py.  The
   runs without it are the unchanged step: their spread is the yardstick.  The visible share: the mean over the 8 views.

Prints one JSON line; `--out FILE` also writes it to FILE.  Nothing is asserted about speed."""
import ctypes as ct
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import build_optimizers
from easy_gaussian_splatting_amd.optim import FusedAdam
from easy_gaussian_splatting_amd.synthetic import config_bench_1m, config_heavy
from easy_gaussian_splatting_amd.train_graph import EPS2D, FAR_PLANE, NEAR_PLANE, TrainStepGraph, _p

args = sys.argv[1:]
out_path, calls, reps = None, 20, 3
for flag in ("--out", "--calls", "--reps"):
    if flag in args:
        i = args.index(flag)
        if flag == "--out":
            out_path = args[i + 1]
        elif flag == "--calls":
            calls = int(args[i + 1])
        else:
            reps = int(args[i + 1])
        del args[i:i + 2]
steps = int(args[0]) if len(args) > 0 else 200
warmup = int(args[1]) if len(args) > 1 else 50
dev = torch.device("cuda:0")
n_views, N = 8, 1_000_000
lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
NAMES = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")


def note(msg):
    print(f"[visible_adam_time] {msg}", file=sys.stderr, flush=True)


def queued(fn, n):
    """n calls enqueued back to back, none waited for: device ms per call by events around all of them"""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def summary(ms):
    return {"median_us": round(1e3 * statistics.median(ms), 2), "min_us": round(1e3 * min(ms), 2), "max_us": round(1e3 * max(ms), 2)}


def alternate(forms):
    """{name: summary}: one warm window of every form, then seven windows of each, the forms taking turns."""
    ms = {k: [] for k in forms}
    for w in range(1 + 7):
        for k, fn in forms.items():
            t = queued(fn, calls)
            if w:
                ms[k].append(t)
    return {k: summary(v) for k, v in ms.items()}


def standalone():
    g = torch.Generator().manual_seed(0)
    shapes = [(N, 3), (N, 3), (N, 4), (N, 1, 3), (N, 15, 3), (N,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    opt = FusedAdam([{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(ps, lrs, NAMES)])
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
    out = {"floats_per_gaussian": sum(p.numel() for p in ps) // N, "bytes_per_dense_step": 28 * sum(p.numel() for p in ps), "rows": []}
    for share in (100, 50, 25, 10, 0):
        for layout in ("scattered", "contiguous"):
            if layout == "scattered":
                seen = torch.rand(N, generator=g) < share / 100.0 if 0 < share < 100 else torch.full((N,), share == 100)
            else:
                seen = torch.zeros(N, dtype=torch.bool)
                count = N * share // 100
                seen[(N - count) // 2:(N - count) // 2 + count] = True   # (the middle of the model)
            radii = seen.to(torch.int32).to(dev)
            r = alternate({"gs_adam_step": lambda: opt.step(), "gs_adam_step_visible": lambda: opt.step(visible=radii)})
            note(f"stand-alone {share} % {layout}: {r}")
            out["rows"].append({"visible_percent": share, "layout": layout, "visible_share": round(float(seen.float().mean()), 4), **r,
                                "selective_over_dense": round(r["gs_adam_step_visible"]["median_us"] / r["gs_adam_step"]["median_us"], 4)})
    del opt, ps
    torch.cuda.empty_cache()
    return out


def scene_inputs(sc):
    W, H = sc["width"], sc["height"]
    datas = [{"w2c": torch.from_numpy(sc["viewmats"][v]).to(dev), "K": torch.from_numpy(sc["Ks"][v]).to(dev), "width": W, "height": H}
             for v in range(n_views)]
    targets = [bench.smooth_target(H, W, 1234 + v, dev) for v in range(n_views)]
    return datas, targets


def make_runner(sc, datas, targets, **kw):
    model = bench.model_from_scene(sc, dev)
    opt = build_optimizers(model, *lrs, fused="hip")
    return model, opt, TrainStepGraph(model, opt, LossComputer(lambda_ssim=0.2, clamp_input=True), datas[0], targets[0], **kw)


def fused_kernels(sc, datas, targets):
    """The two fused entries on the buffers of a finished step (they update in place: the parameters drift by a few learning rates over
    the windows, the gradient rows stay the step's)."""
    model, opt, r = make_runner(sc, datas, targets, rounds="off")
    for v in range(3):
        r.step(datas[v], targets[v])
    r.finish()
    torch.cuda.synchronize()
    L, b, m = nat.lib(), r.buf, model
    W, H = r.W, r.H
    b1, b2 = opt.defaults["betas"]
    offs = (ct.c_int64 * 6)(*opt._offs)
    share = float((b["radii"] > 0).float().mean())

    def call(selective):
        st = torch.cuda.current_stream(dev).cuda_stream
        row_args = (st, r.N, r.K, int(m.active_sh_degree), _p(opt.flat_param), _p(opt.exp_avg), _p(opt.exp_avg_sq), offs,
                    _p(b["viewmats"]), _p(b["Ks"]), W, H, EPS2D, NEAR_PLANE, FAR_PLANE, _p(b["radii"]), _p(b["colors_post"]),
                    r._tpg(), _p(b["cum_tiles"]), _p(b["rows"]), _p(b["row_base"]), _p(b["qmask"]), _p(b["v_abs"]), float(b1),
                    float(b2), float(opt.defaults["eps"]), _p(b["hyper"]), _p(b["applied"]), _p(m.max_radii),
                    _p(m.grad_norm_accum), _p(m.collecting_counts), _p(b["sh_jac"]))
        if selective:
            nat.check(L.gs_project_bwd_selective(*row_args, 0, 0.0, 0.0), "gs_project_bwd_selective")
        else:
            nat.check(L.gs_project_bwd_adam(*row_args), "gs_project_bwd_adam")
    res = alternate({"gs_project_bwd_adam": lambda: call(False), "gs_project_bwd_selective": lambda: call(True)})
    res["visible_share"] = round(share, 4)
    note(f"fused kernels at visible share {share:.4f}: {res}")
    res["selective_over_dense"] = round(res["gs_project_bwd_selective"]["median_us"] / res["gs_project_bwd_adam"]["median_us"], 4)
    del r, model, opt
    torch.cuda.empty_cache()
    return res


def run_captured(sc, datas, targets, visible):
    model, opt, runner = make_runner(sc, datas, targets, **({"visible_adam": True} if visible else {}))
    sched = bench.ViewSchedule(n_views, seed=0)
    seen, last = [], {}

    def one(note=False):
        v = sched.next()
        last["out"] = runner.step(datas[v], targets[v])
        model.update_learning_rate(sched.step)
        if note:
            seen.append(float((last["out"]["batch_radii"] > 0).float().mean()))
    for it in range(warmup):
        one(note=it < n_views)
    runner.finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    runner.finish()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    rep = runner.report()
    out = {"ms_per_step": round(ms, 4), "overflows": rep["overflows"], "rebuilds": rep["rebuilds"], "rounds": rep["rounds"],
           "visible_share": round(statistics.mean(seen), 4), "loss_total": float(last["out"]["loss3"][2])}
    note(f"captured, visible_adam={visible}: {out}")
    del runner, model, opt
    torch.cuda.empty_cache()
    return out


res = {"tool": "tools/visible_adam_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
       "steps": steps, "warmup": warmup, "calls_per_window": calls, "standalone_1m_sh3": standalone(), "scenes": {}}
for name, sc in (("bench (config_bench_1m)", config_bench_1m(seed=42, n=N, n_views=n_views)),
                 ("config_heavy", config_heavy(seed=42, n=N, n_views=n_views))):
    datas, targets = scene_inputs(sc)
    row = {"workload": f"{N} Gaussians, {sc['width']}x{sc['height']}, SH3, {n_views} views", "fused_kernel": fused_kernels(sc, datas, targets),
           "captured_dense": [], "captured_visible": []}
    for rep in range(reps):
        row["captured_dense"].append(run_captured(sc, datas, targets, False))
        row["captured_visible"].append(run_captured(sc, datas, targets, True))
    off = [x["ms_per_step"] for x in row["captured_dense"]]
    on = [x["ms_per_step"] for x in row["captured_visible"]]
    row["dense_ms"] = {"min": min(off), "median": statistics.median(off), "max": max(off)}   # the spread of the unchanged step
    row["visible_ms"] = {"min": min(on), "median": statistics.median(on), "max": max(on)}
    row["visible_minus_dense_us"] = round(1e3 * (statistics.median(on) - statistics.median(off)), 1)
    row["dense_spread_us"] = round(1e3 * (max(off) - min(off)), 1)
    row["visible_share"] = row["captured_visible"][0]["visible_share"]
    res["scenes"][name] = row
    del datas, targets
    torch.cuda.empty_cache()
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
