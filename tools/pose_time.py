#!/usr/bin/env python3
"""What pose refinement adds to the captured step at the bench workload (1 M Gaussians, 1920x1080, SH3, 8 shuffled views, tight
lists, fused Adam): `tools/pose_time.py [steps] [warmup] [--calls N] [--out FILE]`, one process.

* the captured step (TrainStepGraph, hipGraph replay) without and with `poses=CameraDeltas(n_views)`, alternately, each time from a
  fresh model of the same seed -- wall clock per step between synchronisations, like bench.py;
* the launches poses add -- gs_pose_step_inputs, gs_pose_compose, gs_row_sums (the step's ONE walk over the gradient rows: with poses
  the fused projection backward + Adam reads the sums it leaves, gs_project_bwd_adam_sums, in place of walking the rows itself),
  gs_cam_grad_sums (project_cam_kernel + cam_sum_kernel), gs_pose_adam -- each on the buffers a finished step left, HIP events
  around `--calls` calls enqueued back to back (the queue never empty, as inside the graph): device time per call, median / least /
  largest over seven windows; and the fused kernel in its two forms, rows against sums, on throw-away copies of the parameters.

Prints one JSON line; `--out FILE` also writes it to FILE.  Nothing is asserted about speed."""
import ctypes as ct
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
import bench
from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import build_optimizers
from easy_gaussian_splatting_amd.pose import CameraDeltas
from easy_gaussian_splatting_amd.train_graph import EPS2D, FAR_PLANE, NEAR_PLANE, TrainStepGraph, _p

args = sys.argv[1:]
out_path, calls = None, 20
for flag in ("--out", "--calls"):
    if flag in args:
        i = args.index(flag)
        if flag == "--out":
            out_path = args[i + 1]
        else:
            calls = int(args[i + 1])
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


def make_runner(with_poses: bool):
    model = bench.model_from_scene(sc, dev)
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    poses = CameraDeltas(n_views).to(dev) if with_poses else None
    return model, TrainStepGraph(model, opt, lc, datas[0], targets[0], poses=poses)


def run_captured(with_poses: bool):
    model, runner = make_runner(with_poses)
    sched = bench.ViewSchedule(n_views, seed=0)

    def one():
        v = sched.next()
        runner.step(datas[v], targets[v], view_index=v if with_poses else None)
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
    if with_poses:
        out["max_abs_delta"] = float(runner.poses.deltas.detach().abs().max())
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
    """Each launch poses add, on the buffers of a finished step (copies of the corrections and their moments: nothing trains here)."""
    model, r = make_runner(True)
    for v in range(3):
        r.step(datas[v], targets[v], view_index=v)
    r.finish()
    torch.cuda.synchronize()
    L, b, m, N = nat.lib(), r.buf, model, r.N
    st = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    deltas, ea, es = r.poses.deltas.detach().clone(), r.pose_state.exp_avg.clone(), r.pose_state.exp_avg_sq.clone()
    vm = torch.empty((16,), dtype=torch.float32, device=dev)
    forms = {
        "gs_pose_step_inputs": lambda: nat.check(L.gs_pose_step_inputs(st(), 2, n_views, _p(datas[2]["w2c"]), None, 1e-3, 0.9, 0.999, 3, _p(b["pose_rec"])),
                                                 "gs_pose_step_inputs"),
        "gs_pose_compose": lambda: nat.check(L.gs_pose_compose(st(), n_views, _p(b["pose_rec"]), _p(deltas), _p(vm)), "gs_pose_compose"),
        "gs_row_sums": lambda: nat.check(L.gs_row_sums(st(), 1, N, _p(b["radii"]), _p(b["colors_post"]), r._tpg(), _p(b["cum_tiles"]), _p(b["rows"]),
                                                        _p(b["row_base"]), _p(b["qmask"]), _p(b["pose_row_sums"]), _p(b["pose_v_pre"]), None,
                                                        float(max(H, W)), None, None), "gs_row_sums"),
        "gs_cam_grad_sums": lambda: nat.check(L.gs_cam_grad_sums(st(), N, r.K, int(m.active_sh_degree), _p(m.means), _p(m.quats), _p(m.log_scales),
                                                                  _p(m.sh_rest) if r.K > 1 else None, _p(b["viewmats"]), _p(b["Ks"]), W, H, EPS2D,
                                                                  NEAR_PLANE, FAR_PLANE, _p(b["radii"]), _p(b["colors_post"]), 1, _p(b["sh_jac"]),
                                                                  _p(b["pose_row_sums"]), _p(b["cam_partials"]), _p(b["v_viewmats"]),
                                                                  _p(b["v_campos"])), "gs_cam_grad_sums"),
        "gs_pose_adam": lambda: nat.check(L.gs_pose_adam(st(), n_views, _p(b["pose_rec"]), _p(deltas), _p(ea), _p(es), _p(b["v_viewmats"]),
                                                         _p(b["v_campos"]), _p(b["v_delta"]), 0.9, 0.999, 1e-15), "gs_pose_adam"),
    }
    # the fused projection backward + Adam, walking the rows itself (the step without poses) against reading the sums (with poses)
    opt = r.opt
    fp, fm, fv = opt.flat_param.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    stats = [x.clone() for x in (m.max_radii, m.grad_norm_accum, m.collecting_counts)]
    applied, v_abs = torch.zeros((1,), dtype=torch.int64, device=dev), torch.empty_like(b["v_abs"])
    offs = (ct.c_int64 * 6)(*opt._offs)
    b1, b2 = opt.defaults["betas"]
    head = (N, r.K, int(m.active_sh_degree), _p(fp), _p(fm), _p(fv), offs, _p(b["viewmats"]), _p(b["Ks"]), W, H, EPS2D, NEAR_PLANE, FAR_PLANE,
            _p(b["radii"]), _p(b["colors_post"]), r._tpg(), _p(b["cum_tiles"]))
    tail = (_p(v_abs), float(b1), float(b2), float(opt.defaults["eps"]), _p(b["hyper"]), _p(applied), _p(stats[0]), _p(stats[1]), _p(stats[2]),
            _p(b["sh_jac"]))
    forms["gs_project_bwd_adam (walks the rows)"] = lambda: nat.check(
        L.gs_project_bwd_adam(st(), *head, _p(b["rows"]), _p(b["row_base"]), _p(b["qmask"]), *tail), "gs_project_bwd_adam")
    forms["gs_project_bwd_adam_sums (reads the sums)"] = lambda: nat.check(
        L.gs_project_bwd_adam_sums(st(), *head, _p(b["pose_row_sums"]), *tail, 0, 0.0, 0.0, 0, 0.0, 0.0), "gs_project_bwd_adam_sums")
    out = {}
    if r.rounds_on:   # (the rows of a step in two depth rounds are two ranges: gs_row_sums reads the rounds context)
        r._rounds_phase(3)
    try:
        for name, fn in forms.items():
            ms = [queued(fn, calls) for _ in range(1 + 7)][1:]   # one warm window, then seven
            out[name] = summary(ms)
    finally:
        r._rounds_phase(0)
    out["rows_walked"] = int(r.status[6])
    del r, model
    torch.cuda.empty_cache()
    return out


res = {"tool": "tools/pose_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
       "workload": "1M Gaussians, 1920x1080, SH3, 8 views, TrainStepGraph defaults", "steps": steps, "warmup": warmup,
       "captured_without_poses": [], "captured_with_poses": []}
for rep in range(2):
    res["captured_without_poses"].append(run_captured(False))
    res["captured_with_poses"].append(run_captured(True))
off = min(x["ms_per_step"] for x in res["captured_without_poses"])
on = min(x["ms_per_step"] for x in res["captured_with_poses"])
res["best_without_ms"], res["best_with_ms"], res["pose_cost_us"] = off, on, round(1e3 * (on - off), 1)
res["launches"] = added_launches()
added = ("gs_pose_step_inputs", "gs_pose_compose", "gs_row_sums", "gs_cam_grad_sums", "gs_pose_adam")
fused_rows, fused_sums = (res["launches"][k]["median_us"] for k in ("gs_project_bwd_adam (walks the rows)", "gs_project_bwd_adam_sums (reads the sums)"))
res["added_launches_us"] = round(sum(res["launches"][k]["median_us"] for k in added), 1)
res["fused_kernel_saves_us"] = round(fused_rows - fused_sums, 1)   # what reading the sums saves the fused kernel: the walk happens once
res["calls_per_window"] = calls
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
