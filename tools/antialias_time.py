#!/usr/bin/env python3
"""What the antialiased rasterize mode costs in the projection, at the bench workload (1 M Gaussians, 1920x1080, 8 shuffled views, tight
lists, fused Adam, hipGraph replay): `tools/antialias_time.py [steps] [warmup] [--out FILE]`.
For "classic" and "antialiased" in turn, twice, each from a fresh model on the same scene: the captured step
(`TrainStepGraph(rasterize_mode=...)`, wall clock per step between synchronisations, like bench.py), then -- on the buffers the last step
left -- the forward projection launch alone (gs_project_fwd / gs_project_fwd_aa) and the launches behind the blend backward alone (the
fused projection backward + Adam, gs_project_bwd_adam / gs_project_bwd_adam_aa, and the step's status launch), each between two events
over `reps` repetitions.  The antialiased step multiplies every opacity by rho < 1, so its tight lists are shorter and its blend does
less: the list lengths are reported next to the times, and only the two projection figures compare like with like.
Prints one JSON line (per mode the minimum of its runs, and the spread of the classic runs); `--out FILE` also writes it to FILE."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph

args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
steps = int(args[0]) if len(args) > 0 else 100
warmup = int(args[1]) if len(args) > 1 else 30
reps = 20
dev = torch.device("cuda:0")
n_views = 8
sc, _ = bench.build_workload(1_000_000, n_views, dev)
W, H = sc["width"], sc["height"]
targets = [bench.smooth_target(H, W, 1234 + v, dev) for v in range(n_views)]
mask = torch.zeros((H, W), device=dev)
lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
datas = [{"w2c": torch.from_numpy(sc["viewmats"][v]).to(dev), "K": torch.from_numpy(sc["Ks"][v]).to(dev), "width": W, "height": H}
         for v in range(n_views)]


def events_ms(fn, stream):
    with torch.cuda.stream(stream):
        fn()   # (once untimed)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(reps):
            fn()
        t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def run(mode: str):
    model = bench.model_from_scene(sc, dev)
    model.rasterize_mode = mode
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    runner = TrainStepGraph(model, opt, lc, datas[0], targets[0], mask, rounds="off", rasterize_mode=mode)
    sched = bench.ViewSchedule(n_views, seed=0)

    def one():
        v = sched.next()
        runner.step(datas[v], targets[v], mask)
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
    visible = int((runner.buf["radii"] > 0).sum())
    # the two projection stages on their own, on what the last step left (the runner is discarded afterwards: the repeated fused
    # backward moves the parameters and the step counter)
    fwd_ms = events_ms(runner._project, runner.stream)
    bwd_ms = events_ms(lambda: runner._enqueue_rest(runner._st()), runner.stream)
    out = {"rasterize_mode": mode, "ms_per_step": round(ms, 4), "project_fwd_ms": round(fwd_ms, 4), "project_bwd_adam_ms": round(bwd_ms, 4),
           "visible_last_view": visible, "isects_seen": int(rep.get("seen_isects", runner.seen_isects)), "overflows": rep["overflows"],
           "rebuilds": rep["rebuilds"]}
    del runner, opt, model
    torch.cuda.empty_cache()
    return out


KEYS = ("ms_per_step", "project_fwd_ms", "project_bwd_adam_ms")
res = {"workload": "1M Gaussians, 1920x1080, 8 views, TrainStepGraph(rounds='off')", "steps": steps, "warmup": warmup, "reps": reps, "runs": []}
for _ in range(2):
    for name in ("classic", "antialiased"):
        res["runs"].append(run(name))
for name in ("classic", "antialiased"):
    mine = [r for r in res["runs"] if r["rasterize_mode"] == name]
    res[name] = {k: min(r[k] for r in mine) for k in KEYS}
    res[name]["isects_seen"] = mine[0]["isects_seen"]
classic = [r for r in res["runs"] if r["rasterize_mode"] == "classic"]
res["classic_spread"] = {k: round(max(r[k] for r in classic) - min(r[k] for r in classic), 4) for k in KEYS}
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
