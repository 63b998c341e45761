#!/usr/bin/env python3
"""What per-view bilateral grids add to the captured step at the bench workload (1 M Gaussians, 1920x1080, SH3, 8 shuffled views,
tight lists, fused Adam): `tools/bilagrid_time.py [steps] [warmup] [--reps R] [--calls N] [--out FILE]`, one process.

* the captured step (TrainStepGraph, hipGraph replay) without and with `bilagrid=BilateralGrids(n_views)`, alternately, `--reps`
  times each, each time from a fresh model of the same seed -- wall clock per step between synchronisations, like bench.py.  The
  runs without grids are the parent's step: their spread is the yardstick for "nothing changes with bilagrid=None";
* the launches the grids add -- gs_bilagrid_step_inputs, gs_bilagrid_apply, gs_bilagrid_bwd (three kernels: the scatter into per-cell
  partials, the per-node sums, the in-place pass over the gradient image), gs_bilagrid_tv (two kernels), gs_bilagrid_adam -- each on
  the buffers a finished step left, HIP events around `--calls` calls enqueued back to back (the queue never empty, as inside the
  graph): device time per call, median / least / largest over seven windows;
* in the same run, the rate a plain streaming kernel of the library reaches on the same image: gs_clamp01 over H*W*3 floats (one read,
  one write: 8 B per float), and from it what the 60 B per pixel the image passes must move (apply: 12 read + 12 written; backward:
  12 + 12 read, 12 written) would take at that rate;
* the dense part, gs_bilagrid_tv + gs_bilagrid_adam, at n_views = 100, 300 and 1000 with its bytes (TV: 4 read + 4 written per
  element; Adam: 16 read + 12 written), since its traffic grows with the table.

Prints one JSON line; `--out FILE` also writes it to FILE.  Nothing is asserted about speed."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.bilagrid import BilateralGrids
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
GX, GY, GL = 16, 16, 8
sc, _ = bench.build_workload(1_000_000, n_views, dev)
W, H = sc["width"], sc["height"]
datas = [{"w2c": torch.from_numpy(sc["viewmats"][v]).to(dev), "K": torch.from_numpy(sc["Ks"][v]).to(dev), "width": W, "height": H}
         for v in range(n_views)]
targets = [bench.smooth_target(H, W, 1234 + v, dev) for v in range(n_views)]
lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
st = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731


def make_runner(with_grids: bool):
    model = bench.model_from_scene(sc, dev)
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    grids = BilateralGrids(n_views, GX, GY, GL).to(dev) if with_grids else None
    return model, TrainStepGraph(model, opt, lc, datas[0], targets[0], bilagrid=grids)


def run_captured(with_grids: bool):
    model, runner = make_runner(with_grids)
    sched = bench.ViewSchedule(n_views, seed=0)

    def one():
        v = sched.next()
        runner.step(datas[v], targets[v], view_index=v if with_grids else None)
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
    if with_grids:
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12).to(dev)[None, :, None, None, None]
        out["max_abs_grids_minus_identity"] = float((runner.bilagrid.grids.detach() - eye).abs().max())
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


def windows(fn):
    return summary([queued(fn, calls) for _ in range(1 + 7)][1:])   # one warm window, then seven


def dense_forms(L, n, grids, ea, es, v_grids, rec, v_slab, tv_out, ws):
    """gs_bilagrid_tv and gs_bilagrid_adam over n views' grids (copies: nothing trains here)."""
    return {
        "gs_bilagrid_tv": lambda: nat.check(L.gs_bilagrid_tv(st(), n, GX, GY, GL, _p(grids), 10.0, _p(rec), 0, _p(v_slab), None, _p(tv_out),
                                                             _p(v_grids), _p(ws)), "gs_bilagrid_tv"),
        "gs_bilagrid_adam": lambda: nat.check(L.gs_bilagrid_adam(st(), grids.numel(), _p(rec), _p(grids), _p(ea), _p(es), _p(v_grids), 0.9, 0.999,
                                                                 1e-15), "gs_bilagrid_adam"),
    }


def added_launches():
    """Each launch the grids add, on the buffers of a finished step (copies of the grids, their moments and the gradient image), and
    gs_clamp01 over the same image."""
    model, r = make_runner(True)
    for v in range(3):
        r.step(datas[v], targets[v], view_index=v)
    r.finish()
    torch.cuda.synchronize()
    L, b = nat.lib(), r.buf
    grids, ea, es = r.bilagrid.grids.detach().clone(), r.bilagrid_state.exp_avg.clone(), r.bilagrid_state.exp_avg_sq.clone()
    v_img, out_img = b["v_render"].clone(), torch.empty_like(b["exposed"])
    render, rec = b["render_colors"], b["bilagrid_rec"]
    forms = {
        "gs_bilagrid_step_inputs": lambda: nat.check(L.gs_bilagrid_step_inputs(st(), 2, n_views, 2e-3, 0.9, 0.999, 3, _p(rec)), "gs_bilagrid_step_inputs"),
        "gs_bilagrid_apply": lambda: nat.check(L.gs_bilagrid_apply(st(), H, W, n_views, GX, GY, GL, _p(rec), 0, _p(grids), _p(render), _p(out_img)),
                                               "gs_bilagrid_apply"),
        # (in place on a copy of the gradient image: every call applies the transpose again, the identity's neighbourhood here)
        "gs_bilagrid_bwd": lambda: nat.check(L.gs_bilagrid_bwd(st(), H, W, n_views, GX, GY, GL, _p(rec), 0, _p(grids), _p(render), _p(v_img),
                                                               _p(b["bilagrid_partials"]), _p(b["v_slab"])), "gs_bilagrid_bwd"),
        **dense_forms(L, n_views, grids, ea, es, b["v_grids"], rec, b["v_slab"], b["bilagrid_tv"], b["bilagrid_tv_ws"]),
        "gs_clamp01": lambda: nat.check(L.gs_clamp01(st(), render.numel(), _p(render), None, _p(out_img)), "gs_clamp01"),
    }
    out = {name: windows(fn) for name, fn in forms.items()}
    dense = {}
    for n in (100, 300, 1000):
        big = BilateralGrids(n, GX, GY, GL).to(dev).grids.detach()
        bufs = [torch.zeros_like(big) for _ in range(3)]
        row = {name: windows(fn) for name, fn in dense_forms(L, n, big, bufs[0], bufs[1], bufs[2], rec, b["v_slab"], b["bilagrid_tv"],
                                                               b["bilagrid_tv_ws"]).items()}
        row["elements"] = big.numel()
        row["tv_bytes"], row["adam_bytes"] = 8 * big.numel(), 28 * big.numel()
        row["tv_GBps"] = round(row["tv_bytes"] / (1e3 * row["gs_bilagrid_tv"]["median_us"]), 1)
        row["adam_GBps"] = round(row["adam_bytes"] / (1e3 * row["gs_bilagrid_adam"]["median_us"]), 1)
        dense[str(n)] = row
        del big, bufs
        torch.cuda.empty_cache()
    del r, model
    torch.cuda.empty_cache()
    return out, dense


res = {"tool": "tools/bilagrid_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
       "workload": "1M Gaussians, 1920x1080, SH3, 8 views, TrainStepGraph defaults, grids 16 x 16 x 8", "steps": steps, "warmup": warmup,
       "captured_without_bilagrid": [], "captured_with_bilagrid": []}
for rep in range(reps):
    res["captured_without_bilagrid"].append(run_captured(False))
    res["captured_with_bilagrid"].append(run_captured(True))
off = [x["ms_per_step"] for x in res["captured_without_bilagrid"]]
on = [x["ms_per_step"] for x in res["captured_with_bilagrid"]]
res["without_ms"] = {"min": min(off), "median": statistics.median(off), "max": max(off)}   # the spread of the parent's own step
res["with_ms"] = {"min": min(on), "median": statistics.median(on), "max": max(on)}
res["bilagrid_cost_us"] = round(1e3 * (min(on) - min(off)), 1)
res["launches"], res["dense_by_n_views"] = added_launches()
added = ("gs_bilagrid_step_inputs", "gs_bilagrid_apply", "gs_bilagrid_bwd", "gs_bilagrid_tv", "gs_bilagrid_adam")
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
