#!/usr/bin/env python3
"""What per-view exposure compensation adds to the captured step at the bench workload (1 M Gaussians, 1920x1080, SH3, 8 shuffled
views, tight lists, fused Adam): `tools/exposure_time.py [steps] [warmup] [--reps R] [--calls N] [--out FILE]`, one process.

* the captured step (TrainStepGraph, hipGraph replay) without and with `exposure=ExposureTable(n_views)`, alternately, `--reps`
  times each, each time from a fresh model of the same seed -- wall clock per step between synchronisations, like bench.py.  The
  runs without a table are the parent's step: their spread is the yardstick for "nothing changes with exposure=None";
* the launches exposure adds -- gs_exposure_step_inputs, gs_exposure_apply, gs_exposure_bwd (two kernels: the streaming pass and the
  pass over its per-block partials), gs_exposure_adam -- each on the buffers a finished step left, HIP events around `--calls` calls
  enqueued back to back (the queue never empty, as inside the graph): device time per call, median / least / largest over seven
  windows;
* in the same run, the rate a plain streaming kernel of the library reaches on the same image: gs_clamp01 over H*W*3 floats (one read,
  one write: 8 B per float), and from it what the 60 B per pixel of the two image kernels (apply: 12 read + 12 written; backward:
  12 + 12 read, 12 written) would take at that rate.

Prints one JSON line; `--out FILE` also writes it to FILE.  Nothing is asserted about speed."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.exposure import ExposureTable
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph, _p

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
n_views = 8
sc, _ = bench.build_workload(1_000_000, n_views, dev)
W, H = sc["width"], sc["height"]
datas = [{"w2c": torch.from_numpy(sc["viewmats"][v]).to(dev), "K": torch.from_numpy(sc["Ks"][v]).to(dev), "width": W, "height": H}
         for v in range(n_views)]
targets = [bench.smooth_target(H, W, 1234 + v, dev) for v in range(n_views)]
lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def make_runner(with_table: bool):
    model = bench.model_from_scene(sc, dev)
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    table = ExposureTable(n_views).to(dev) if with_table else None
    return model, TrainStepGraph(model, opt, lc, datas[0], targets[0], exposure=table)


def run_captured(with_table: bool):
    model, runner = make_runner(with_table)
    sched = bench.ViewSchedule(n_views, seed=0)

    def one():
        v = sched.next()
        runner.step(datas[v], targets[v], view_index=v if with_table else None)
        model.update_learning_rate(sched.step)
    for _ in range(warmup):
        one()
    runner.finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    runner.finish()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    rep = runner.report()
    out = {"ms_per_step": round(ms, 4), "overflows": rep["overflows"], "rebuilds": rep["rebuilds"], "rounds": rep["rounds"]}
    if with_table:
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).to(dev)
        out["max_abs_affine_minus_identity"] = float((runner.exposure.affine.detach() - eye).abs().max())
    del runner, model
    torch.cuda.empty_cache()
    return out


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


def added_launches():
    """Each launch exposure adds, on the buffers of a finished step (copies of the table, its moments and the gradient image: nothing
    trains here), and gs_clamp01 over the same image."""
    model, r = make_runner(True)
    for v in range(3):
        r.step(datas[v], targets[v], view_index=v)
    r.finish()
    torch.cuda.synchronize()
    L, b = nat.lib(), r.buf
    st = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    table, ea, es = r.exposure.affine.detach().clone(), r.exposure_state.exp_avg.clone(), r.exposure_state.exp_avg_sq.clone()
    v_img, out_img = b["v_render"].clone(), torch.empty_like(b["exposed"])
    render = b["render_colors"]
    forms = {
        "gs_exposure_step_inputs": lambda: nat.check(L.gs_exposure_step_inputs(st(), 2, n_views, 1e-2, 0.9, 0.999, 3, _p(b["exposure_rec"])),
                                                     "gs_exposure_step_inputs"),
        "gs_exposure_apply": lambda: nat.check(L.gs_exposure_apply(st(), H, W, n_views, _p(b["exposure_rec"]), 0, _p(table), _p(render),
                                                                   _p(out_img)), "gs_exposure_apply"),
        # (in place on a copy of the gradient image: every call multiplies it by A^T again, the identity's neighbourhood here)
        "gs_exposure_bwd": lambda: nat.check(L.gs_exposure_bwd(st(), H, W, n_views, _p(b["exposure_rec"]), 0, _p(table), _p(render), _p(v_img),
                                                               _p(b["exposure_partials"]), _p(b["v_affine"])), "gs_exposure_bwd"),
        "gs_exposure_adam": lambda: nat.check(L.gs_exposure_adam(st(), n_views, _p(b["exposure_rec"]), _p(table), _p(ea), _p(es), _p(b["v_affine"]),
                                                                 0.9, 0.999, 1e-15), "gs_exposure_adam"),
        "gs_clamp01": lambda: nat.check(L.gs_clamp01(st(), render.numel(), _p(render), None, _p(out_img)), "gs_clamp01"),
    }
    out = {}
    for name, fn in forms.items():
        ms = [queued(fn, calls) for _ in range(1 + 7)][1:]   # one warm window, then seven
        out[name] = summary(ms)
    del r, model
    torch.cuda.empty_cache()
    return out


res = {"tool": "tools/exposure_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
       "workload": "1M Gaussians, 1920x1080, SH3, 8 views, TrainStepGraph defaults", "steps": steps, "warmup": warmup,
       "captured_without_exposure": [], "captured_with_exposure": []}
for rep in range(reps):
    res["captured_without_exposure"].append(run_captured(False))
    res["captured_with_exposure"].append(run_captured(True))
off = [x["ms_per_step"] for x in res["captured_without_exposure"]]
on = [x["ms_per_step"] for x in res["captured_with_exposure"]]
res["without_ms"] = {"min": min(off), "median": statistics.median(off), "max": max(off)}   # the spread of the parent's own step
res["with_ms"] = {"min": min(on), "median": statistics.median(on), "max": max(on)}
res["exposure_cost_us"] = round(1e3 * (min(on) - min(off)), 1)
res["launches"] = added_launches()
added = ("gs_exposure_step_inputs", "gs_exposure_apply", "gs_exposure_bwd", "gs_exposure_adam")
res["added_launches_us"] = round(sum(res["launches"][k]["median_us"] for k in added), 1)
clamp_us = res["launches"]["gs_clamp01"]["median_us"]
res["stream_rate_GBps"] = round(8.0 * 3 * H * W / (1e3 * clamp_us), 1)              # gs_clamp01: 8 B per float over H*W*3 floats
res["image_kernels_bytes"] = 60 * H * W
res["image_kernels_at_stream_rate_us"] = round(60.0 * H * W / (8.0 * 3 * H * W) * clamp_us, 1)
res["calls_per_window"] = calls
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
