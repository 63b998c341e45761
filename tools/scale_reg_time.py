#!/usr/bin/env python3
"""Cost of the scale-ratio regulariser in the captured step at the bench workload (1 M Gaussians, 1920x1080, SH3, 8 shuffled views,
tight lists, fused Adam, hipGraph replay): `tools/scale_reg_time.py [steps] [warmup] [--out FILE]`.
Times TrainStepGraph with use_scale_regularization off and on (max_scale_ratio 10, lambda_scale 0.1 as the reference's
configs name them), alternately, each time from a fresh model of the same seed -- wall clock per step between synchronisations,
like bench.py -- and gs_scale_reg alone (HIP events).  Prints one JSON line; `--out FILE` also writes it to FILE."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph

args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
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
mask = torch.zeros((H, W), device=dev)
lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def run(reg: bool):
    model = bench.model_from_scene(sc, dev)
    model.USE_SCALE_REGULARIZATION, model.MAX_SCALE_RATIO = reg, 10.0
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True, model=model, lambda_scale=0.1)
    runner = TrainStepGraph(model, opt, lc, datas[0], targets[0], mask)
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
    out = {"ms_per_step": round(ms, 4), "overflows": rep["overflows"], "rebuilds": rep["rebuilds"]}
    if reg:
        out["scale_reg"] = float(runner.buf["scale_reg"][0])
        out["share_above_ratio"] = float(((torch.exp(model.log_scales).amax(1) / torch.exp(model.log_scales).amin(1)) >= 10.0).float().mean())
    del runner, opt, model
    torch.cuda.empty_cache()
    return out


res = {"workload": "1M Gaussians, 1920x1080, SH3, 8 views, TrainStepGraph defaults", "steps": steps, "warmup": warmup,
       "off": [], "on": []}
for rep in range(2):
    res["off"].append(run(False))
    res["on"].append(run(True))
# the value + gradient pass alone (the form the unfused and view-parallel steps use) and the value pass alone
L = nat.lib()
m = bench.model_from_scene(sc, dev)
N = m.means.shape[0]
ls = m.log_scales.detach()
ws = torch.zeros((int(L.gs_scale_reg_workspace_floats(N)),), device=dev)
v = torch.zeros_like(ls)
loss3 = torch.zeros((3,), device=dev)
st = torch.cuda.current_stream(dev).cuda_stream
for name, vp in (("value_pass_us", None), ("value_and_grad_pass_us", v.data_ptr())):
    for _ in range(20):
        nat.check(L.gs_scale_reg(st, N, ls.data_ptr(), 10.0, 0.1, loss3.data_ptr(), ws.data_ptr(), vp), "gs_scale_reg")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        nat.check(L.gs_scale_reg(st, N, ls.data_ptr(), 10.0, 0.1, loss3.data_ptr(), ws.data_ptr(), vp), "gs_scale_reg")
    e1.record()
    torch.cuda.synchronize()
    res[name] = round(1e3 * e0.elapsed_time(e1) / 200, 2)
off = min(r["ms_per_step"] for r in res["off"])
on = min(r["ms_per_step"] for r in res["on"])
res["best_off_ms"], res["best_on_ms"], res["delta_us"] = off, on, round(1e3 * (on - off), 1)
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
