#!/usr/bin/env python3
"""Cost of SH degree 4 in the captured step at the bench workload (1 M Gaussians, 1920x1080, 8 shuffled views, tight lists,
fused Adam, hipGraph replay): `tools/sh_degree_time.py [steps] [warmup] [--out FILE]`.
Times TrainStepGraph at SH3 / K = 16 (the bench model) and at SH4 / K = 25 (the same scene, 9 more coefficients per colour
channel drawn at the scale of the third band), alternately, each time from a fresh model -- wall clock per step between
synchronisations, like bench.py.  Per-kernel times (project_fwd_kernel<4, 0>, project_bwd_kernel<4, true> against their
degree-3 forms): run this tool under `rocprofv3 --kernel-trace --stats`.
Prints one JSON line; `--out FILE` also writes it to FILE."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
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


def make(deg: int):
    m3 = bench.model_from_scene(sc, dev)
    if deg == 3:
        return m3
    rest = m3.sh_rest.detach()
    g = torch.Generator(device=dev).manual_seed(4)
    band4 = torch.randn((rest.shape[0], 9, 3), generator=g, device=dev) * rest[:, 8:].std()
    return GaussianModel(means=m3.means.detach(), log_scales=m3.log_scales.detach(), quats=m3.quats.detach(),
                         sh_0=m3.sh_0.detach(), sh_rest=torch.cat([rest, band4], 1).contiguous(),
                         logit_opacities=m3.logit_opacities.detach(), sh_degree=4, sh_degree_interval=0,
                         white_background=bool(sc["backgrounds"][0, 0] > 0.5)).to(dev)


def run(deg: int):
    model = make(deg)
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
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
    out = {"sh_degree": deg, "K": 1 + model.sh_rest.shape[1], "ms_per_step": round(ms, 4), "overflows": rep["overflows"],
           "rebuilds": rep["rebuilds"]}
    del runner, opt, model
    torch.cuda.empty_cache()
    return out


res = {"workload": "1M Gaussians, 1920x1080, 8 views, TrainStepGraph defaults", "steps": steps, "warmup": warmup,
       "sh3": [], "sh4": []}
for rep in range(2):
    res["sh3"].append(run(3))
    res["sh4"].append(run(4))
s3 = min(r["ms_per_step"] for r in res["sh3"])
s4 = min(r["ms_per_step"] for r in res["sh4"])
res["best_sh3_ms"], res["best_sh4_ms"], res["delta_pct"] = s3, s4, round(100.0 * (s4 - s3) / s3, 2)
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
