#!/usr/bin/env python3
"""What depth supervision adds to the captured step at the bench workload (1 M Gaussians, 1920x1080, SH3, 8 shuffled views, tight
lists, fused Adam): `tools/depth_step_time.py [steps] [warmup] [--reps R] [--calls N] [--out FILE]`, one process.

* the captured step (TrainStepGraph, hipGraph replay) without and with `depth=DepthSupervision(...)`, alternately, `--reps` times
  each, each time from a fresh model of the same seed -- wall clock per step between synchronisations, like bench.py.  The runs
  without depth are the parent's step: their spread is the yardstick for "nothing changes with depth=None".  The targets: the
  initial model's own expected depth per view, scaled by 1.05, with a hole of zeros;
* the launches depth adds around the image loss -- gs_depth_step_inputs, gs_depth_loss_split (the one pass over the [H,W,4] blend),
  gs_depth_loss_finish, gs_depth_loss_join (the one pass in front of the blend backward), gs_rec_depth, gs_depth_grads_z -- each on
  the buffers a finished step left, HIP events around `--calls` calls enqueued back to back (the queue never empty, as inside the
  graph): device time per call, median / least / largest over seven windows;
* in the same run, the rate a plain streaming kernel of the library reaches on the same image: gs_clamp01 over H*W*3 floats (one read,
  one write: 8 B per float), and from it what the two image passes (split: 16 + 4 + 4 B per pixel read, 12 + 4 written = 40, + the
  mask's 4 when there is one; join: 16 + 4 + 4 + 4 + 12 read, 16 + 4 written = 60) would take at that rate;
* the blend forward and backward at 3 against 4 channels: the eager model (`model(data, clamp=False)` against `depth="ED"`) under
  `rendering.profile_stages` with the two blend stages repeated ten times inside their events, as bench.py isolates them.

Prints one JSON line; `--out FILE` also writes it to FILE.  Nothing is asserted about speed."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import rendering
from easy_gaussian_splatting_amd.depth_loss import DepthSupervision
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
LAMBDA, MODE = 0.01, "disparity"
sc, _ = bench.build_workload(1_000_000, n_views, dev)
W, H = sc["width"], sc["height"]
datas = [{"w2c": torch.from_numpy(sc["viewmats"][v]).to(dev), "K": torch.from_numpy(sc["Ks"][v]).to(dev), "width": W, "height": H}
         for v in range(n_views)]
targets = [bench.smooth_target(H, W, 1234 + v, dev) for v in range(n_views)]
lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def depth_targets():
    model = bench.model_from_scene(sc, dev)
    out = []
    with torch.no_grad():
        for v in range(n_views):
            t = (model(datas[v], clamp=False, depth="ED")["render_depth"][..., 0] * 1.05).contiguous()
            t[H // 3:H // 2, W // 4:W // 2] = 0.0
            out.append(t)
    del model
    torch.cuda.empty_cache()
    return out


gt_depths = depth_targets()


def make_runner(with_depth: bool):
    model = bench.model_from_scene(sc, dev)
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    kw = dict(depth=DepthSupervision(LAMBDA, MODE), gt_depth=gt_depths[0]) if with_depth else {}
    return model, TrainStepGraph(model, opt, lc, datas[0], targets[0], **kw)


def run_captured(with_depth: bool):
    model, runner = make_runner(with_depth)
    sched = bench.ViewSchedule(n_views, seed=0)
    last = {}

    def one():
        v = sched.next()
        last["out"] = runner.step(datas[v], targets[v], gt_depth=gt_depths[v]) if with_depth else runner.step(datas[v], targets[v])
        model.update_learning_rate(sched.step)
    for _ in range(warmup):
        one()
    runner.finish()
    torch.cuda.synchronize()
    first = float(last["out"]["depth_loss"]) if with_depth else None
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    runner.finish()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    rep = runner.report()
    out = {"ms_per_step": round(ms, 4), "overflows": rep["overflows"], "rebuilds": rep["rebuilds"], "rounds": rep["rounds"]}
    if with_depth:
        out["depth_loss_after_warmup"], out["depth_loss_at_end"] = first, float(last["out"]["depth_loss"])
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
    """Each launch depth adds around the loss, on the buffers of a finished step (outputs into copies: nothing trains here), and
    gs_clamp01 over the same image."""
    model, r = make_runner(True)
    for v in range(3):
        r.step(datas[v], targets[v], gt_depth=gt_depths[v])
    r.finish()
    torch.cuda.synchronize()
    L, b = nat.lib(), r.buf
    st = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    rec, img3, depth = b["depth_rec"].clone(), torch.empty_like(b["render_colors"]), torch.empty_like(b["render_depth"])
    v4, va, vz = torch.empty_like(b["v_colors4"]), torch.empty_like(b["v_alphas"]), torch.empty_like(b["v_depths"])
    rec_copy = b["rec"].clone()
    c4, al, part = b["render_colors4"], b["render_alphas"], b["depth_partials"]
    forms = {
        "gs_depth_step_inputs": lambda: nat.check(L.gs_depth_step_inputs(st(), LAMBDA, 1, _p(gt_depths[2]), _p(rec)), "gs_depth_step_inputs"),
        "gs_rec_depth": lambda: nat.check(L.gs_rec_depth(st(), 1, r.N, 3, _p(b["depths"]), _p(b["radii"]), _p(rec_copy)), "gs_rec_depth"),
        "gs_depth_loss_split": lambda: nat.check(L.gs_depth_loss_split(st(), H, W, _p(rec), 0.0, 0, None, None, None, _p(c4), _p(al), _p(img3),
                                                                       _p(depth), _p(part)), "gs_depth_loss_split"),
        "gs_depth_loss_finish": lambda: nat.check(L.gs_depth_loss_finish(st(), H, W, _p(rec), 0.0, 1, _p(part), None), "gs_depth_loss_finish"),
        "gs_depth_loss_join": lambda: nat.check(L.gs_depth_loss_join(st(), H, W, _p(rec), 0.0, 0, None, None, None, _p(c4), _p(al),
                                                                     _p(b["render_depth"]), _p(b["v_render"]), _p(v4), _p(va)), "gs_depth_loss_join"),
        "gs_depth_grads_z": lambda: nat.check(L.gs_depth_grads_z(st(), 1, r.N, 3, _p(b["radii"]), r._tpg(), _p(b["cum_tiles"]), _p(b["rows"]),
                                                                 _p(b["row_base"]), _p(b["qmask"]), _p(vz)), "gs_depth_grads_z"),
        "gs_clamp01": lambda: nat.check(L.gs_clamp01(st(), img3.numel(), _p(b["render_colors"]), None, _p(img3)), "gs_clamp01"),
    }
    out = {}
    for name, fn in forms.items():
        ms = [queued(fn, calls) for _ in range(1 + 7)][1:]   # one warm window, then seven
        out[name] = summary(ms)
    del r, model
    torch.cuda.empty_cache()
    return out


def blend_stages():
    """gs_blend_fwd / gs_blend_bwd of the eager model at 3 channels and at 4 (depth="ED"), each repeated ten times inside its events."""
    model = bench.model_from_scene(sc, dev)
    out = {}
    for name, depth in (("ch3", None), ("ch4", "ED")):
        ms = {"gs_blend_fwd": [], "gs_blend_bwd": []}
        for it in range(1 + 3):   # one warm pass, then three views
            rendering.profile_stages(True, repeat={"gs_blend_fwd": 10, "gs_blend_bwd": 10})
            o = model(datas[it], clamp=False, depth=depth)
            loss = (o["render_img"] - targets[it]).abs().mean()
            if depth is not None:
                loss = loss + 0.01 * (o["render_depth"][..., 0] - gt_depths[it]).abs().mean()
            loss.backward()
            prof = rendering.profile_stages(False)
            for p in model.parameters():
                p.grad = None
            if it > 0:
                for k in ms:
                    ms[k].extend(prof.get(k, []))
        out[name] = {k: round(1e3 * statistics.mean(v), 1) for k, v in ms.items() if v}
    del model
    torch.cuda.empty_cache()
    return out


res = {"tool": "tools/depth_step_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
       "workload": "1M Gaussians, 1920x1080, SH3, 8 views, TrainStepGraph defaults", "steps": steps, "warmup": warmup,
       "lambda_depth": LAMBDA, "mode": MODE, "captured_without_depth": [], "captured_with_depth": []}
for rep in range(reps):
    res["captured_without_depth"].append(run_captured(False))
    res["captured_with_depth"].append(run_captured(True))
off = [x["ms_per_step"] for x in res["captured_without_depth"]]
on = [x["ms_per_step"] for x in res["captured_with_depth"]]
res["without_ms"] = {"min": min(off), "median": statistics.median(off), "max": max(off)}   # the spread of the parent's own step
res["with_ms"] = {"min": min(on), "median": statistics.median(on), "max": max(on)}
res["depth_cost_us"] = round(1e3 * (min(on) - min(off)), 1)
res["launches"] = added_launches()
added = [k for k in res["launches"] if k != "gs_clamp01"]
res["added_launches_us"] = round(sum(res["launches"][k]["median_us"] for k in added), 1)
clamp_us = res["launches"]["gs_clamp01"]["median_us"]
res["stream_rate_GBps"] = round(8.0 * 3 * H * W / (1e3 * clamp_us), 1)              # gs_clamp01: 8 B per float over H*W*3 floats
res["image_pass_bytes"] = {"gs_depth_loss_split": 40 * H * W, "gs_depth_loss_join": 60 * H * W}
res["image_passes_at_stream_rate_us"] = {k: round(v / (8.0 * 3 * H * W) * clamp_us, 1) for k, v in res["image_pass_bytes"].items()}
res["blend_us"] = blend_stages()
res["blend_added_us"] = {k: round(res["blend_us"]["ch4"][k] - res["blend_us"]["ch3"][k], 1) for k in res["blend_us"]["ch3"]}
res["calls_per_window"] = calls
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
