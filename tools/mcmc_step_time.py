#!/usr/bin/env python3
"""Training under a Gaussian budget at the bench workload (1 M Gaussians, 1920x1080, SH3, 8 shuffled views, tight lists, fused Adam):
`tools/mcmc_step_time.py [steps] [warmup] [--calls N] [--noise-only] [--out FILE]`, one process.

* the captured step (TrainStepGraph, hipGraph replay) without and with `mcmc=MCMCStrategy(..., noise="counter")`, alternately, each
  time from a fresh model of the same seed -- wall clock per step between synchronisations, like bench.py;
* the eager budget loop (model forward, LossComputer, `regularization(fused=True)`, backward, FusedAdam, `after_step`) the same way,
  over a fifth of the steps: what the captured step is an alternative to;
* the noise alone, HIP events around one call, the two forms taking turns: `inject_noise` with noise="counter" (gs_mcmc_step_inputs +
  gs_mcmc_noise_step) against noise="torch" (torch.randn + gs_mcmc_noise), median / least / largest of `--calls` calls; and the
  same two forms with 50 calls enqueued back to back per window (the queue never empty, as in a train loop): device time per call.
  Kernel times on their own: run `--noise-only` under `rocprofv3 --kernel-trace --stats` (profiles/mcmc_noise_kernel_stats.csv).

No refinement falls into the timed windows (refine_start beyond them).  Prints one JSON line; `--out FILE` also writes it to FILE.
Nothing is asserted about speed; `fused_noise_not_slower` (isolated calls) and `fused_noise_not_slower_queued` record how the two
noise forms compared in this run."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.mcmc import MCMCStrategy
from easy_gaussian_splatting_amd.model import build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph

args = sys.argv[1:]
out_path, calls = None, 21
for flag in ("--out", "--calls"):
    if flag in args:
        i = args.index(flag)
        if flag == "--out":
            out_path = args[i + 1]
        else:
            calls = int(args[i + 1])
        del args[i:i + 2]
noise_only = "--noise-only" in args   # the last part alone
if noise_only:
    args.remove("--noise-only")
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
REG = (0.01, 0.01)
NEVER = 10 ** 9


def fresh(noise="counter"):
    model = bench.model_from_scene(sc, dev)
    opt = build_optimizers(model, *lrs, fused="hip")
    st = MCMCStrategy(model, cap_max=model.nbr_gaussians, refine_start=NEVER, refine_stop=NEVER, noise=noise, seed=7,
                      generator=torch.Generator(device=dev).manual_seed(1))
    return model, opt, st


def timed_loop(one, finish, n_warm, n_steps):
    for _ in range(n_warm):
        one()
    finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        one()
    finish()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n_steps


def run_captured(mcmc: bool):
    model, opt, st = fresh()
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    runner = TrainStepGraph(model, opt, lc, datas[0], targets[0], mcmc=st if mcmc else None, mcmc_reg=REG)
    sched = bench.ViewSchedule(n_views, seed=0)

    def one():
        v = sched.next()
        runner.step(datas[v], targets[v])
        if mcmc:
            st.after_step(sched.step, runner)
        model.update_learning_rate(sched.step)
    ms = timed_loop(one, runner.finish, warmup, steps)
    rep = runner.report()
    out = {"ms_per_step": round(ms, 4), "overflows": rep["overflows"], "rebuilds": rep["rebuilds"]}
    if mcmc:
        out["mcmc_reg"] = float(runner.buf["mcmc_reg"][0])
    del runner, opt, model, st
    torch.cuda.empty_cache()
    return out


def run_eager():
    model, opt, st = fresh()
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    sched = bench.ViewSchedule(n_views, seed=0)

    def one():
        v = sched.next()
        out = model(datas[v], clamp=False)
        loss = lc.get_loss_dict(out["render_img"], targets[v])
        (loss["total"] + st.regularization(*REG, fused=True)).backward()
        model.update_statistics(datas[v], out)
        opt.step()
        opt.zero_grad()
        st.after_step(sched.step)
        model.update_learning_rate(sched.step)
    ms = timed_loop(one, lambda: None, max(warmup // 5, 3), max(steps // 5, 10))
    del opt, model, st
    torch.cuda.empty_cache()
    return {"ms_per_step": round(ms, 4)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


res = {"tool": "tools/mcmc_step_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
       "workload": "1M Gaussians, 1920x1080, SH3, 8 views, TrainStepGraph defaults", "steps": steps, "warmup": warmup, "mcmc_reg": REG,
       "captured_without_mcmc": [], "captured_with_mcmc": []}
for rep in range(0 if noise_only else 2):
    res["captured_without_mcmc"].append(run_captured(False))
    res["captured_with_mcmc"].append(run_captured(True))
if not noise_only:
    res["eager_budget_loop"] = run_eager()
    off = min(r["ms_per_step"] for r in res["captured_without_mcmc"])
    on = min(r["ms_per_step"] for r in res["captured_with_mcmc"])
    res["best_without_ms"], res["best_with_ms"], res["budget_cost_us"] = off, on, round(1e3 * (on - off), 1)
    res["captured_over_eager_budget_loop"] = round(res["eager_budget_loop"]["ms_per_step"] / on, 3)

# the noise alone: both forms on models of the same state (the means drift apart by their draws, nothing the timing sees)
(_, _, st_counter), (_, _, st_torch) = fresh("counter"), fresh("torch")
means_lr = 1.6e-4
a, b = [], []
for k in range(3 + calls):   # three warm calls of each (code objects, the allocator), then the two forms take turns
    torch.cuda.synchronize(dev)
    ta = timed(lambda: st_counter.inject_noise(means_lr, k + 1))
    tb = timed(lambda: st_torch.inject_noise(means_lr))
    if k >= 3:
        a.append(ta)
        b.append(tb)
res["noise"] = {"calls": calls, "counter_fused": summary(a), "torch_randn_plus_noise": summary(b)}
res["fused_noise_not_slower"] = bool(statistics.median(a) <= statistics.median(b))


def queued(fn, n):
    """n calls enqueued back to back, none waited for: (device ms per call by events around all of them, host ms per call to enqueue)"""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    host = 1e3 * (time.perf_counter() - t0) / n
    e1.synchronize()
    return e0.elapsed_time(e1) / n, host


# ... and the way a train loop meets it, the queue never empty: QUEUE calls back to back per window, the two forms taking turns.  An
# isolated call (above) also times the device idling between its two launches, whichever is the shorter first kernel.
QUEUE, qa, qb, ha, hb = 50, [], [], [], []
for k in range(1 + 7):   # one warm window of each, then seven
    da, xa = queued(lambda i: st_counter.inject_noise(means_lr, 1000 + QUEUE * k + i), QUEUE)
    db, xb = queued(lambda i: st_torch.inject_noise(means_lr), QUEUE)
    if k >= 1:
        qa.append(da); qb.append(db); ha.append(xa); hb.append(xb)
res["noise_queued"] = {"calls_per_window": QUEUE, "windows": len(qa), "counter_fused": summary(qa), "torch_randn_plus_noise": summary(qb),
                       "host_enqueue_ms_per_call": {"counter_fused": round(statistics.median(ha), 4), "torch_randn_plus_noise": round(statistics.median(hb), 4)}}
res["fused_noise_not_slower_queued"] = bool(statistics.median(qa) <= statistics.median(qb))
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
