#!/usr/bin/env python3
"""Benchmark of the rasterization hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

A "step" is one training iteration of the reference's loop around the seam
(/root/reference/train.py:93-157 without DataLoader / TensorBoard): activations ->
rasterization forward -> clamp -> L1 + (1-SSIM) -> backward -> update_statistics ->
[gradient exchange over RCCL when N>1] -> Adam step -> zero grads,
on the workload BASELINE.json quotes its metric on: 1 M Gaussians, 1920x1080, SH degree 3
(synthetic generator of SURVEY.md section 8d; there is no dataset in this environment).
One rank per GPU, one view per rank per step (weak scaling); `value` = view-iterations/s of the
whole job.  Forward-only render fps of the same workload is reported next to it.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process stays GPU-free, starts N
fresh rank processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set), waits for them and exits with
the first non-zero status.  Under `torch.distributed.run` (WORLD_SIZE set) it is one of the ranks.

Extra objects: `roofline` for the dominant blend kernel (algorithmic bytes of SURVEY.md 8d for the
intersections the launch actually processed, over its HIP-event duration on the launch stream),
`roofline_compute` (the same kernel against the VALU issue rate, the limiter it actually has) and
`cpu_baseline` (the C/OpenMP oracle timed on the host cores on a bounded sample; rank 0, N=1 only).

A plain run sets up, warms up, times the K steps and prints the headline line (`metric`, `value`, `unit`,
`ms_per_step`, `step_ms`, `config`, ...).  Everything else -- static view, hand-back and host-fed loops, forward fps,
per-stage times, rooflines, extras, captured-step configs, `cpu_baseline`, `per_rank` -- runs with `--full` only
(`--no-extras`, `--no-configs`, `--no-cpu-baseline` trim a `--full` run).

`--dump-outputs DIR`: after the timed steps, what the last timed step handed its caller -- the rendered image,
the three loss terms, and the Gaussians' parameters after the optimizer step plus the step's radii and
absolute 2-D mean gradients on a fixed seeded sample of 65536 Gaussians -- as float32 / float64 DIR/<name>.npy.
The workload, the targets and the view schedule are seeded: the same arguments give the same inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0    # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
N_SIMD = 1024            # 256 CUs x 4 SIMD-32
VALU_CYCLES_PER_WAVE_INST = 2.0   # wave64 on a SIMD-32 (same guide, cycle-constants table)
CLOCK_HZ_NOMINAL = 2.4e9
# blend_bwd's main loop, one systolic step of four (pixel, entry) pairs per lane, counted in the ISA hipcc emits
# (hipcc -S of csrc/gs_blend.hip, loop .LBB1_24): 208 VALU = 160 fma / mul / add / sub / min / DPP moves, 21 v_cmp, 19 v_cndmask,
# 8 transcendentals (4 v_exp_f32 + 4 v_rcp_f32); 24 SALU and 2 LDS reads ride along
BWD_LOOP_MIX = {"simple": 160, "cmp_cndmask": 40, "transcendental": 8}
PROFILE_TAGS = ("r06", "r05", "r04", "r03", "r02", "r01")     # committed rocprofv3 summaries under profiles/, newest first


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--cpu-sample", type=int, default=1_000_000)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary timings (gsplat-list mode, drop-in loop, long lists)")
    ap.add_argument("--no-configs", action="store_true", help="skip the captured-step figures on the long-list / S3 / S5 workloads")
    ap.add_argument("--torch-adam", action="store_true", help="torch.optim.Adam(fused=True) instead of the HIP Adam")
    ap.add_argument("--no-graph", action="store_true", help="enqueue every step from Python instead of replaying the captured hipGraph")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement (static view, host-fed, forward fps, stage times, rooflines, extras, "
                         "configs, CPU baseline); off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32 / float64, <= 64 MB)")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------ launcher
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int, argv) -> int:
    """Parent of an N-rank run: never touches the GPU (no torch.cuda / HIP call happens in this process),
    starts N fresh interpreters on this file, one per GPU, and returns the first non-zero exit status."""
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for rank in range(n):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool (RCCL needs it)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    deadline = None
    while procs:
        for p in list(procs):
            r = p.poll()
            if r is None:
                continue
            procs.remove(p)
            if r != 0 and rc == 0:
                rc = r
                deadline = time.time() + 30.0   # a failed rank leaves the others stuck in a collective
        if deadline is not None and time.time() > deadline:
            for p in procs:
                p.kill()
        time.sleep(0.05)
    return rc


# ------------------------------------------------------------------------------------------------ helpers
def _percentiles(ms):
    import numpy as np
    a = np.asarray(ms, dtype=np.float64)
    return {"median": round(float(np.median(a)), 4), "p10": round(float(np.percentile(a, 10)), 4),
            "p90": round(float(np.percentile(a, 90)), 4), "mean": round(float(a.mean()), 4), "n": int(a.size)}


def _profile_json(name: str):
    for tag in PROFILE_TAGS:
        path = os.path.join(ROOT, "profiles", f"{tag}_{name}")
        try:
            with open(path) as f:
                return json.load(f), f"profiles/{tag}_{name}"
        except (OSError, ValueError):
            continue
    return None, None


def pmc_traffic(kernel_prefix: str):
    """HBM bytes per launch of the kernel whose name starts with `kernel_prefix`, from the committed rocprofv3
    --pmc passes of this same command (profiles/rNN_pmc_traffic.json, produced by tools/pmc_summary.py with the
    gfx950 FETCH_SIZE x2 correction of MI355X_MICROARCH.md); None when no such profile is committed."""
    data, src = _profile_json("pmc_traffic.json")
    if not data:
        return None, None
    for k, v in data.items():
        if k.startswith(kernel_prefix) and v.get("traffic_bytes_per_launch") is not None:
            # [lower, upper]: FETCH_SIZE raw + writes (what a gather-dominated kernel moves: gathers are counted in full at their
            # 64-byte sector) and 2 x FETCH_SIZE + writes (the guide's correction, exact for coalesced streams) --
            # profiles/r03_traffic_calibration.json; the blend kernels' reads are record gathers: near the lower end
            lo = v.get("traffic_bytes_per_launch_lower")
            return ([lo, v["traffic_bytes_per_launch"]] if lo is not None else v["traffic_bytes_per_launch"]), src
    return None, src


def sq_counters(kernel_prefix: str):
    data, src = _profile_json("sq_counters.json")
    if not data:
        return None, None
    for k, v in data.items():
        if k.startswith(kernel_prefix):
            return v, src
    return None, src


DUMP_SAMPLE = 65536            # Gaussians in the seeded sample of --dump-outputs
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, model, render_img, loss3, radii, absgrad) -> int:
    """--dump-outputs: the last timed step's image and loss terms in full, the parameters after its optimizer step and its
    radii / absolute 2-D mean gradients on a fixed sample of Gaussians (seed 0, sorted indices, the same for the same
    model size).  Returns the bytes written."""
    import numpy as np
    import torch
    n = int(model.means.shape[0])
    idx = np.sort(np.random.default_rng(0).choice(n, size=min(n, DUMP_SAMPLE), replace=False))
    sel = torch.from_numpy(idx).to(model.means.device)
    rows = lambda t: t.detach().reshape((n,) + tuple(t.shape[2:])).index_select(0, sel)   # [1, N, ...] -> [sample, ...]
    arrays = {"render_img": render_img.detach(), "loss3": loss3.detach().reshape(-1), "gaussian_sample_index": idx.astype(np.float64),
              "radii": rows(radii), "absgrad": rows(absgrad)}
    for name in ("means", "quats", "log_scales", "logit_opacities", "sh_0", "sh_rest"):
        arrays[name] = getattr(model, name).detach().index_select(0, sel)
    arrays = {k: np.ascontiguousarray(v.float().cpu().numpy() if torch.is_tensor(v) else v) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs would write {total} bytes"
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)
    return total


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sc, sample_n: int, reps: int):
    """Oracle (C + OpenMP, all host cores) on the first `sample_n` Gaussians of the same workload: rasterization
    forward + backward, one warm-up (spins the OpenMP pool up, pages the arrays in) + `reps` timed repetitions.
    Plus the S1 leg of BASELINE.md section 3: the pure-PyTorch restatement on configs[0] (10 k Gaussians, 256x256,
    SH0), forward and forward+backward.  Reported baselines only."""
    import numpy as np
    from oracle import c_oracle as CO
    CO.build()
    cores = os.cpu_count() or 1
    os.environ.setdefault("OMP_NUM_THREADS", str(cores))
    n = min(sample_n, sc["means"].shape[0])
    W, H = sc["width"], sc["height"]
    vc = None
    times, n_isects = [], 0
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fw = CO.render(sc["means"][:n], sc["quats"][:n], sc["scales"][:n], sc["opacities"][:n], sc["shs"][:n],
                       sc["viewmats"][:1], sc["Ks"][:1], W, H, sh_degree=sc["sh_degree"],
                       backgrounds=sc["backgrounds"][:1], dtype=np.float32)
        if vc is None:
            vc = (np.random.default_rng(0).standard_normal(fw["render_colors"].shape) / (W * H)).astype(np.float32)
        CO.backward(fw, vc)
        if rep > 0:
            times.append(time.perf_counter() - t0)
        n_isects = fw["n_isects"]
    med = float(np.median(times))
    out = {"value": round(1.0 / med, 4), "unit": "iters/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(),
           "reps_s": [round(t, 3) for t in times],
           "sample": f"oracle/c (C+OpenMP) rasterization fwd+bwd, first {n} of the workload's Gaussians at {W}x{H} "
                     f"SH{sc['sh_degree']}, I={n_isects} (gsplat lists), median of {reps} repetitions after 1 warm-up"}
    # S1 leg: pure-PyTorch restatement (oracle/torch_oracle.py) in its own process, bounded by a hard timeout.  (In
    # this process the C oracle's OpenMP pool is still spinning; torch's own pool at the box's full core count on
    # top of it crawls.)  Small tensors: more than 16 threads only add synchronisation.
    threads = min(cores, 16)
    code = (
        "import sys, time, json, torch; sys.path.insert(0, %r)\n"
        "from easy_gaussian_splatting_amd.synthetic import config_s1\n"
        "from oracle import torch_oracle as TO\n"
        "torch.set_num_threads(%d)\n"
        "s1 = config_s1(); T = lambda k: torch.from_numpy(s1[k]).double()\n"
        "ins = [T(k).requires_grad_(True) for k in ('means', 'quats', 'scales', 'opacities', 'shs')]\n"
        "def run(bwd):\n"
        "    t0 = time.perf_counter()\n"
        "    img, alpha, _ = TO.rasterization(*ins, T('viewmats'), T('Ks'), 256, 256, sh_degree=0, packed=False, backgrounds=T('backgrounds'))\n"
        "    if bwd: torch.autograd.grad(img.sum(), ins)\n"
        "    return time.perf_counter() - t0\n"
        "run(False); f = min(run(False) for _ in range(2)); fb = min(run(True) for _ in range(2))\n"
        "print(json.dumps({'fwd_ms': round(1e3 * f, 1), 'fwd_bwd_ms': round(1e3 * fb, 1)}))\n" % (ROOT, threads))
    try:
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_WAIT_POLICY="passive")
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=90)
        s1 = json.loads(p.stdout.strip().splitlines()[-1])
        s1["workload"] = ("configs[0]: 10k Gaussians, 256x256, SH0, oracle/torch_oracle.py (fp64, autograd), "
                          f"{threads} threads, best of 2")
        out["s1_torch"] = s1
    except Exception as e:   # the S1 leg must never cost the bench line
        out["s1_torch"] = {"error": repr(e)[:200]}
    return out


def model_from_scene(sc, device):
    import numpy as np
    import torch
    from easy_gaussian_splatting_amd.model import GaussianModel
    t = lambda a: torch.from_numpy(a).to(device)
    shs = t(sc["shs"])
    op = np.clip(sc["opacities"], 1e-6, 1 - 1e-6)
    model = GaussianModel(means=t(sc["means"]), log_scales=torch.log(t(sc["scales"])), quats=t(sc["quats"]),
                          sh_0=shs[:, :1].contiguous(), sh_rest=shs[:, 1:].contiguous(),
                          logit_opacities=t(np.log(op / (1 - op)).astype(np.float32)),
                          sh_degree=sc["sh_degree"], sh_degree_interval=0,
                          white_background=bool(sc["backgrounds"][0, 0] > 0.5)).to(device)
    return model


def build_workload(n_gauss: int, n_views: int, device):
    from easy_gaussian_splatting_amd.synthetic import config_bench_1m
    sc = config_bench_1m(seed=42, n=n_gauss, n_views=max(n_views, 1))
    return sc, model_from_scene(sc, device)


def smooth_target(H: int, W: int, seed: int, device):
    """A band-limited random image (bilinear up-sampling of H/8 x W/8 noise): the synthetic ground truth."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    gt = torch.rand((max(H // 8, 1), max(W // 8, 1), 3), generator=g).to(device)
    return torch.nn.functional.interpolate(gt.permute(2, 0, 1)[None], size=(H, W), mode="bilinear",
                                           align_corners=False)[0].permute(1, 2, 0).contiguous()


class ViewSchedule:
    """`shuffle=True` of the reference's DataLoader (/root/reference/train.py:36-43): a fresh seeded permutation of the
    views per epoch; rank r of `world` takes draws r, r + world, ... of the common stream (one view per GPU per step)."""

    def __init__(self, n_views: int, world: int = 1, rank: int = 0, seed: int = 0):
        import numpy as np
        self.n, self.world, self.rank = n_views, world, rank
        self.rng = np.random.RandomState(seed)
        self.queue = []
        self.step = 0          # 1-based iteration count after the first next(): what update_learning_rate receives

    def next(self) -> int:
        self.step += 1
        picks = []
        for _ in range(self.world):
            if not self.queue:
                self.queue = list(self.rng.permutation(self.n))
            picks.append(int(self.queue.pop(0)))
        return picks[self.rank]


def real_loop(sc, device, lrs, datas, targets, mask, steps: int, refine_every: int, reset_at: int, captured: bool,
              max_growth: float = 3.0):
    """The reference's loop END TO END on the bench workload (/root/reference/train.py:93-157): a shuffled view every step,
    update_statistics every step, `densify_and_prune` every `refine_every` steps (train.py:129-135; the reference's
    refine_every is 200), ONE `reset_opacities` (at step `reset_at`) instead of the densification of that step, the
    means-LR schedule every step -- wall clock from the first step to the last, re-builds / re-captures / overflow replays
    of the captured step INCLUDED.  `captured`: train_graph.TrainStepGraph, else the eager model step.  A fresh model from the
    same seed either way, so the two trajectories are comparable."""
    import numpy as np
    import torch
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.model import build_optimizers
    model = model_from_scene(sc, device)
    opt = build_optimizers(model, *lrs, fused="hip")
    lc = LossComputer(lambda_ssim=0.2, clamp_input=True)
    sched = ViewSchedule(len(datas), seed=1)
    gen = torch.Generator(device=device).manual_seed(7)   # split noise: the same stream in both modes
    n0 = model.nbr_gaussians
    runner = None
    if captured:
        from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
        runner = TrainStepGraph(model, opt, lc, datas[0], targets[0], mask)   # (class defaults: eager hand-back)
    one = torch.ones((), device=device)
    losses, traj, refine_s, drain_s = [], [n0], 0.0, 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, steps + 1):
        v = sched.next()
        if runner is not None:
            runner.step(datas[v], targets[v], mask)
        else:
            out = model(datas[v], clamp=False)
            loss3 = lc.get_loss_dict(out["render_img"], targets[v], mask)
            loss3["total"].backward(gradient=one)
            model.update_statistics(datas[v], out)
            opt.step()
            opt.zero_grad()
            losses.append(loss3["total"].detach())
        model.update_learning_rate(it)
        if it % refine_every == 0 and it < steps:
            td = time.perf_counter()
            if runner is not None:
                runner.finish()
            torch.cuda.synchronize()   # (the refinement's one host read would drain the queue anyway: counted apart)
            tr = time.perf_counter()
            drain_s += tr - td
            if it == reset_at:
                model.reset_opacities()
            elif model.nbr_gaussians <= max_growth * n0:
                model.densify_and_prune(generator=gen)
            traj.append(model.nbr_gaussians)
            torch.cuda.synchronize()
            refine_s += time.perf_counter() - tr
    if runner is not None:
        runner.finish()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if runner is not None:
        tail = runner.loss_history(50)[:, 2]
    else:
        tail = torch.stack(losses[-50:])
    out = {"train_iters_per_s": round(steps / wall, 2), "wall_s": round(wall, 3), "steps": steps,
           "refine_every": refine_every, "reset_opacities_at": reset_at, "n_gaussians": traj,
           "refine_wall_s": round(refine_s, 4), "queue_drain_wait_s": round(drain_s, 3), "loss_mean_last_50": round(float(tail.mean().item()), 6),
           "finite": bool(torch.isfinite(tail).all().item())}
    if runner is not None:
        rep = runner.report()
        out.update(captures=rep["captures"], overflows=rep["overflows"], replayed_steps=rep["replayed_steps"], rebuilds=rep["rebuilds"],
                   build_ms=rep.get("build_ms"), capture_ms=rep.get("capture_ms"))
    del runner, model, opt
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------ the reference's loop, restated
class DropInLoop:
    """What a maintainer of the reference gets from the ONE-LINE import change of INTEGRATION.md section 2 and nothing
    else: the reference's own loop body, restated line by line around `rasterization()` --
      forward             /root/reference/model/gaussian.py:351-374  (torch exp / sigmoid / cat, packed=False, absgrad=True,
                                                                      gsplat's tile lists, `[0]`, torch.clamp)
      loss                /root/reference/model/gaussian.py:422-453  (mask blend, F.l1_loss, SSIM as torchmetrics computes
                                                                      it: `loss.ssim`, a conv2d restatement -- torchmetrics is
                                                                      not installed here)
      three .item() reads /root/reference/train.py:103-105           (every step, right after backward)
      update_statistics   /root/reference/model/gaussian.py:188-197  (boolean-index form; the reference runs it for steps
                                                                      500..15000, i.e. half of a 30 k run: always on here)
      torch.optim.Adam    /root/reference/model/gaussian.py:389-412  (six groups, torch defaults: foreach, not fused)
      step / zero_grad    /root/reference/train.py:152-153
    No fused loss, no in-kernel activations, no split SH hand-over, no tight lists, no HIP Adam, no hipGraph."""

    def __init__(self, sc, device, lrs, loss: str = "torch", adam: str = "torch", size_check: str = "immediate"):
        """`loss="hip"` / `adam="hip"`: the next two one-line swaps of INTEGRATION.md section 2 (this package's LossComputer /
        build_optimizers(..., fused="hip")) on top of the import change -- the rest of the loop stays the reference's."""
        import torch
        self.torch = torch
        self.m = model_from_scene(sc, device)
        names = ["means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities"]
        if adam == "hip":
            from easy_gaussian_splatting_amd.model import build_optimizers
            self.opt = build_optimizers(self.m, *lrs, fused="hip")
        else:
            self.opt = torch.optim.Adam([{"params": [getattr(self.m, k)], "lr": lr, "name": k} for k, lr in zip(names, lrs)])
        self.lambda_ssim = 0.2
        self.size_check = size_check   # "deferred": rasterization(..., _size_check="deferred") -- the opt-in sync-free seam
        self.hip_loss = None
        if loss == "hip":
            from easy_gaussian_splatting_amd.loss import LossComputer
            self.hip_loss = LossComputer(lambda_ssim=0.2)

    def forward(self, data):
        from easy_gaussian_splatting_amd.rendering import rasterization   # <- the import the maintainer changes
        torch, m = self.torch, self.m
        w2c = data["w2c"]
        batch_render_imgs, _, meta = rasterization(
            means=m.means, quats=m.quats, scales=torch.exp(m.log_scales), opacities=torch.sigmoid(m.logit_opacities),
            colors=torch.cat([m.sh_0, m.sh_rest], dim=1), sh_degree=m.active_sh_degree, viewmats=w2c[None], Ks=data["K"][None],
            width=data["width"], height=data["height"], backgrounds=m.BACKGROUND[None], absgrad=True, packed=False,
            **({} if self.size_check == "immediate" else {"_size_check": self.size_check}))
        render_img = torch.clamp(batch_render_imgs[0], min=0.0, max=1.0)
        return {"render_img": render_img, "batch_xys": meta["means2d"], "batch_radii": meta["radii"]}

    def loss_dict(self, render_img, gt_img, mask):
        if self.hip_loss is not None:
            return self.hip_loss.get_loss_dict(render_img, gt_img, mask)
        import torch.nn.functional as F
        from easy_gaussian_splatting_amd.loss import ssim
        mask = mask.unsqueeze(2).repeat(1, 1, 3)
        render_img = mask * gt_img + (1.0 - mask) * render_img
        l1_loss = F.l1_loss(render_img, gt_img)
        ssim_loss = 1.0 - ssim(gt_img.permute(2, 0, 1)[None, ...], render_img.permute(2, 0, 1)[None, ...])
        return {"l1": l1_loss, "ssim": ssim_loss, "total": (1.0 - self.lambda_ssim) * l1_loss + self.lambda_ssim * ssim_loss}

    def update_statistics(self, data, model_output):
        torch, m = self.torch, self.m
        max_hw = max(data["height"], data["width"])
        radii = model_output["batch_radii"].detach()[0] / max_hw
        xys_absgrad = model_output["batch_xys"].absgrad.detach()[0]
        visible = radii > 0.0
        m.max_radii[visible] = torch.max(m.max_radii[visible], radii[visible])
        grads = torch.norm(xys_absgrad, dim=-1) * max_hw
        m.grad_norm_accum[visible] = m.grad_norm_accum[visible] + grads[visible]
        m.collecting_counts[visible] = m.collecting_counts[visible] + 1

    def step(self, data, gt_img, mask, item_reads: bool = True, phases=None):
        """`phases` (a dict): HIP events at the phase boundaries are appended to it (one extra pass of bench.py reports where
        the step's time goes: event-to-event time on the stream, host-induced gaps included)."""
        torch = self.torch

        def mark(name):
            if phases is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                phases.setdefault(name, []).append(e)

        mark("start")
        model_output = self.forward(data)
        mark("forward")
        loss_dict = self.loss_dict(model_output["render_img"], gt_img, mask)
        mark("loss")
        loss_dict["total"].backward()
        mark("backward")
        if item_reads:
            for _name, loss in loss_dict.items():
                loss.item()
        mark("item_reads")
        with torch.no_grad():
            self.update_statistics(data, model_output)
        mark("update_statistics")
        self.opt.step()
        self.opt.zero_grad()
        mark("adam")


# ------------------------------------------------------------------------------------------------ one rank
def run_rank(args) -> int:
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with --gpus equal to the number of ranks")
    backend = os.environ.get("GS_BENCH_BACKEND", "nccl")   # "nccl" is RCCL on ROCm
    import torch
    import torch.distributed as dist

    if os.environ.get("GS_BENCH_DRYRUN") == "1":
        # launcher self-test (tests/test_bench_launcher.py): rendezvous only, no GPU, no product code
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank)])
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"dryrun": True, "n_gpus": dist.get_world_size(), "rank_sum": float(t.item())}), flush=True)
        dist.barrier()
        dist.destroy_process_group()
        return 0

    import numpy as np
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback for the product path)")
    n_dev = torch.cuda.device_count()
    if world > 1 and backend == "nccl" and n_dev < world:
        raise SystemExit(f"bench.py: {world} ranks need {world} GPUs, this node shows {n_dev} "
                         "(RCCL refuses two ranks on one device; GS_BENCH_BACKEND=gloo exercises the code path only)")
    dev_index = local_rank % n_dev
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    # GS_BENCH_FORCE_DIST=1: initialise the process group and run the exchange path even with ONE rank (RCCL smoke on a 1-GPU box)
    force_dist = os.environ.get("GS_BENCH_FORCE_DIST") == "1"
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        # GS_BENCH_BACKEND=gloo only exists to exercise this code path with several ranks on a 1-GPU box; never used for numbers
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)

    from easy_gaussian_splatting_amd import rendering
    from easy_gaussian_splatting_amd.distributed import GradBucket, ViewParallelStep, all_reduce_param_grads
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.model import build_optimizers

    n_views = max(8, world)
    sc, model = build_workload(args.gaussians, n_views, device)
    W, H = sc["width"], sc["height"]
    # The reference's loop shape (/root/reference/train.py:36-43, 93-98): a DataLoader with shuffle=True hands the step a
    # DIFFERENT view every iteration -- camera, target image and mask change, and with them the visible set and every list
    # length.  The "dataset" is the 8 views of SURVEY.md 8d's generator, uploaded before the loop (the DataLoader itself
    # is outside the metric, 8d); rank r of an N-rank job takes every N-th draw of the same seeded permutation stream.
    datas = [{"w2c": torch.from_numpy(sc["viewmats"][v]).to(device), "K": torch.from_numpy(sc["Ks"][v]).to(device),
              "width": W, "height": H} for v in range(n_views)]
    targets = [smooth_target(H, W, 1234 + v, device) for v in range(n_views)]
    view = rank % n_views
    data, gt_img = datas[view], targets[view]      # the static-camera figures (`static_view`, forward fps, stage profile)
    mask = torch.zeros((H, W), device=device)
    sched = ViewSchedule(n_views, world, rank, seed=0)
    lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)   # /root/reference/configs/tandt_db.yaml
    if args.torch_adam:
        optimizer = build_optimizers(model, *lrs, fused=True)
        bucket = GradBucket(model.parameters())
    else:  # one HIP kernel per step over flat params/moments; gradients are autograd's own tensors
        optimizer = build_optimizers(model, *lrs, fused="hip")
        bucket = None
    loss_computer = LossComputer(lambda_ssim=0.2, clamp_input=True)   # the model's clamp(0,1) is applied inside the loss kernels
    # N > 1: factorised exchange (all-gather of colour gradients + all-reduce of the geometry
    # gradients, distributed.ViewParallelStep); GS_DP_EXCHANGE=allreduce selects the plain all-reduce
    exchange = "none" if (world == 1 and not force_dist) else os.environ.get("GS_DP_EXCHANGE", "factorised")
    # GS_VP_CAPTURE=1 (opt-in): the view-parallel step with everything in front of its first collective as one hipGraph
    # (train_graph.ViewParallelGraphStep); default: the step enqueued eagerly around its two collectives
    vp_capture = os.environ.get("GS_VP_CAPTURE") == "1"
    vp = ViewParallelStep(model, optimizer, force_exchange=force_dist, guard_words=vp_capture) if (exchange == "factorised" and bucket is None) else None
    if (world > 1 or force_dist) and vp is None:
        exchange = "allreduce"

    one = torch.ones((), device=device)   # root gradient, allocated once (backward() would fill a new one per step)
    last = {}   # what the latest step of the timed path handed back (--dump-outputs)

    def train_step(data=data, gt_img=gt_img):
        if vp is not None:
            vp.begin_step(data)
        out = model(data, clamp=False)
        if vp is not None:
            vp.after_forward(data, out)
        ld = loss_computer.get_loss_dict(out["render_img"], gt_img, mask)
        last["loss3"] = (ld["l1"], ld["ssim"], ld["total"])
        loss = ld["total"]
        loss.backward(gradient=one)
        if vp is not None:
            vp.step(data, out)
            return out
        model.update_statistics(data, out)
        if bucket is not None:
            bucket.all_reduce_mean(force=force_dist)
            optimizer.step()
            bucket.zero_()
        else:
            all_reduce_param_grads(model.parameters(), force=force_dist)
            optimizer.step()
            optimizer.zero_grad()
        return out

    # Single GPU, HIP Adam: the whole step is captured once into a hipGraph and replayed (train_graph.TrainStepGraph:
    # capacity-sized list buffers, no host read-back; a step whose lists outgrow the capacity is a device-side no-op
    # that the runner detects, re-captures with larger buffers and replays)
    graph_step = None
    if world == 1 and not force_dist and not args.no_graph and not args.torch_adam:
        try:
            from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
            # The headline runs the runner as a default user gets it: handback="eager" (every step orders the caller's stream
            # behind itself on return), `inputs_ready` off (every step waits for the caller's stream on entry) -- ADVICE r4.
            # The opt-in handback="lazy" (this loop reads nothing between steps, so the caller's stream could stay idle and
            # the entry wait would be free: round 4's headline) is timed right behind it and reported as `lazy_handback`.
            graph_step = TrainStepGraph(model, optimizer, loss_computer, data, gt_img, mask, margin=float(os.environ.get('GS_TG_MARGIN', '1.3')),
                                        handback=os.environ.get("GS_TG_HANDBACK", "eager"))
        except ImportError:
            graph_step = None
    elif vp is not None and vp_capture and vp.native and not args.no_graph:
        from easy_gaussian_splatting_amd.train_graph import ViewParallelGraphStep
        graph_step = ViewParallelGraphStep(model, optimizer, loss_computer, data, gt_img, mask, vp=vp, margin=float(os.environ.get('GS_TG_MARGIN', '1.3')),
                                           handback=os.environ.get("GS_TG_HANDBACK", "eager"))

    def loop_step():
        """One iteration of the reference's loop: the next shuffled view (camera + target), the step, the means-LR
        schedule (/root/reference/train.py:93-98, 140, 152-153)."""
        v = sched.next()
        if graph_step is not None:
            graph_step.step(datas[v], targets[v], mask)
        else:
            last["out"] = train_step(datas[v], targets[v])
        model.update_learning_rate(sched.step)

    step_fn = loop_step

    def barrier():
        if world > 1 or force_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_loop(fn, steps, warmup, finish=None, ev_stream=None, spin_up=None):
        """EXACTLY `steps` calls of fn between barrier+synchronize brackets (wall clock, the contract's number),
        with one HIP event per step boundary on the launch stream for the per-step distribution (`ev_stream`: the graph
        runner's own stream -- with a lazy hand-back the caller's stream carries nothing).  `finish` (the graph
        runner's deferred overflow check + replay of skipped steps) runs INSIDE the timed bracket."""
        for _ in range(warmup):
            fn()
        if finish is not None:
            finish()
        if spin_up is not None:
            spin_up()
        barrier()
        rendering.stats["sync_wait_ns"] = 0
        stream = ev_stream if ev_stream is not None else torch.cuda.current_stream(device)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        t0 = time.perf_counter()
        evs[0].record(stream)
        for i in range(steps):
            fn()
            evs[i + 1].record(stream)
        t_enq = time.perf_counter() - t0
        if finish is not None:
            finish()
        barrier()
        elapsed = time.perf_counter() - t0
        per_step = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
        return elapsed, t_enq, per_step, rendering.stats["sync_wait_ns"] * 1e-6 / max(steps, 1)

    def trace(msg):
        if os.environ.get("GS_BENCH_TRACE") == "1":
            torch.cuda.synchronize()
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    trace("setup done")
    # ---- train iterations (the timed region)
    g_stream = None if graph_step is None else graph_step.stream
    # The shader clock takes 10-15 training steps (~20 ms) to ramp after the idle GPU of the set-up phase: with the driver's 5
    # warm-up steps the first timed steps ran 1.53 -> 1.42 ms (693 against 705 it/s over 20 steps; 200 / 50 does not see it).
    # 60 ms of forward-only renders -- no training state touched, not a training step -- sit between the W warm-up steps and
    # the timed region; GS_BENCH_SPINUP_MS=0 switches them off.  Reported as `spin_up_ms`.
    spin_ms = float(os.environ.get("GS_BENCH_SPINUP_MS", "60"))

    def spin_up():
        """Forward-only renders (no training state touched) for `spin_ms` of wall clock right in front of the timed region."""
        t_end = time.perf_counter() + spin_ms * 1e-3
        with torch.no_grad():
            i = 0
            while time.perf_counter() < t_end:
                model(datas[i % n_views], clamp=False)
                i += 1
                if i % 16 == 0:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()

    elapsed, t_enqueued, step_ms, host_wait_ms = timed_loop(step_fn, args.steps, args.warmup,
                                                            finish=None if graph_step is None else graph_step.finish, ev_stream=g_stream,
                                                            spin_up=spin_up if spin_ms > 0 else None)
    trace("timed loop done")
    if os.environ.get("GS_BENCH_TRACE") == "1":
        print("[bench] step ms: " + " ".join(f"{x:.3f}" for x in step_ms[:64]), file=sys.stderr, flush=True)
    graph_report = None if graph_step is None else graph_step.report()   # (of the headline run: the extras re-capture the runner)
    if args.dump_outputs and rank == 0:
        if graph_step is not None:   # (finish() ran inside the bracket: the runner's buffers hold the last step's results)
            b = graph_step.buf
            res = (b["render_colors"][0], b["loss3"], b["radii"], b["v_abs"])
        else:
            o = last["out"]
            res = (o["render_img"], torch.stack(last["loss3"]), o["batch_radii"], o["batch_xys"].absgrad)
        dump_outputs(args.dump_outputs, model, *res)

    def headline_line(elapsed):
        """The result line's headline part: what a plain run prints (a --full run adds its figures to it)."""
        line = {
            "metric": "train iters/sec + forward render fps, 1M Gaussians @ 1080p",
            "value": round(world * args.steps / elapsed, 3), "unit": "iters/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "spin_up_ms": spin_ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "step_ms": _percentiles(step_ms),
            "config": {"workload": f"{args.gaussians} Gaussians, {W}x{H}, SH degree {sc['sh_degree']}, "
                                   "1 view per GPU per step, full train step (fwd + L1/SSIM + bwd + stats + Adam)",
                       "view_schedule": f"{n_views} views (camera + target image), a fresh seeded permutation per epoch "
                                        "(DataLoader shuffle=True, the reference's train.py:36-43), a different view every "
                                        "step, means-LR schedule updated every step (train.py:140); TrainStepGraph at its class defaults "
                                        "(handback='eager', inputs_ready off)",
                       "list_mode": "tight (model default; image, radii, means2d bitwise identical to the gsplat-list mode, gradients equal to rounding: "
                                    "<= 1e-4 of the tensor's largest entry)",
                       "parallelism": f"view-dp{world}", "exchange": exchange,
                       "dist_backend": dist.get_backend() if (world > 1 or force_dist) else None,
                       "dist_world_size": dist.get_world_size() if (world > 1 or force_dist) else 1,
                       "step_launch": ("hipGraph replay" if (world == 1 and not force_dist) else "hipGraph replay up to the first collective + 4 launches") if graph_step is not None else "eager",
                       "exchange_bytes_per_rank": None if (world == 1 and not force_dist) else (
                           {"all_gather_view_record": 16 * args.gaussians + 64, "all_reduce_geometry_stats": 4 * 13 * args.gaussians,
                            "collectives_per_step": 2} if vp is not None else
                           {"all_reduce_grads": 4 * 59 * args.gaussians, "all_reduce_stats": 12 * args.gaussians})},
            # host diagnostics: ms/step the host spent enqueueing, and blocked on the list-size read-back (0 when
            # the captured step is replayed: no read-back exists on that path)
            "host": {"enqueue_ms_per_step": round(1e3 * t_enqueued / args.steps, 4),
                     "blocked_on_readback_ms_per_step": round(host_wait_ms, 4)},
        }
        if graph_report is not None:
            line["host"]["graph"] = graph_report
            if graph_report["overflows"]:
                line["host"]["graph"]["note"] = "overflowed steps were replayed inside the timed bracket"
        return line

    if not args.full:   # the headline alone
        if world > 1:
            tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        if rank == 0:
            print(json.dumps(headline_line(elapsed)), flush=True)
        if world > 1 or force_dist:
            dist.barrier()
            dist.destroy_process_group()
        return 0

    lazy_handback = None
    if graph_step is not None and graph_step.handback == "eager" and not args.no_extras and world == 1 and not force_dist:
        graph_step.handback = "lazy"   # (read per step: no re-build)
        e_l, _, s_l, _ = timed_loop(step_fn, args.steps, 10, finish=graph_step.finish, ev_stream=g_stream)
        graph_step.fence()
        graph_step.handback = "eager"
        lazy_handback = {"train_iters_per_s": round(args.steps / e_l, 2), "train_ms": _percentiles(s_l),
                         "note": "the headline loop with TrainStepGraph(handback='lazy') -- opt-in: the caller's stream is ordered behind a step only "
                                 "when the caller touches the returned outputs or calls fence(); rounds 4's headline mode"}
    # ---- host_fed: the loop the way the reference FEEDS it (train.py:36-43 DataLoader(pin_memory=True), :97 data_to_device): camera,
    # target image and mask of every step come from page-locked host memory -- 33 MB per step at 1080p -- uploaded on a copy
    # stream into two recycled device slots, event-ordered in front of the replay (train_graph.HostFeed); with float32 targets
    # (what the reference's loader pins) and with uint8 targets (a third of the bytes, converted on the device with the loader's
    # own `/ 255`).  The headline above has the 8 targets resident in HBM, as the contract asks.
    host_fed = None
    if graph_step is not None and not args.no_extras and world == 1 and not force_dist:
        try:
            from easy_gaussian_splatting_amd.train_graph import HostFeed
            pin = lambda t: t.detach().cpu().contiguous().pin_memory()
            hm = pin(mask)
            host_fed = {}
            # what the link gives: one 64 MB pinned -> device copy on an otherwise idle GPU, best of 5 (HIP events)
            probe_h, probe_d = torch.empty((64 << 20,), dtype=torch.uint8).pin_memory(), torch.empty((64 << 20,), dtype=torch.uint8, device=device)
            best = 1e9
            for _ in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); probe_d.copy_(probe_h, non_blocking=True); e1.record(); e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
            h2d_peak = (64 << 20) / (best * 1e-3) / 1e9
            del probe_h, probe_d
            for kind in ("float32", "uint8"):
                imgs = [pin(t) if kind == "float32" else pin((t * 255.0).round().clamp(0, 255).to(torch.uint8)) for t in targets]
                batches = [{"w2c": pin(d["w2c"]), "K": pin(d["K"]), "width": W, "height": H, "image": imgs[v], "mask": hm} for v, d in enumerate(datas)]
                feed = HostFeed(graph_step, n_slots=2)

                def fed_step():
                    feed.step(batches[sched.next()])
                    model.update_learning_rate(sched.step)

                e_h, _, s_h, _ = timed_loop(fed_step, args.steps, 10, finish=graph_step.finish, ev_stream=g_stream)
                graph_step.fence()
                nbytes = sum(int(b["image"].numel() * b["image"].element_size() + b["mask"].numel() * 4 + 100) for b in batches) / len(batches)
                host_fed[kind] = {"train_iters_per_s": round(args.steps / e_h, 2), "train_ms": _percentiles(s_h),
                                  "slowest_steps_ms": [round(float(x), 3) for x in sorted(s_h)[-5:]],
                                  "host_bytes_per_step": int(nbytes), "h2d_GBps": round(nbytes * args.steps / e_h / 1e9, 2),
                                  "h2d_GBps_at_headline_rate": round(nbytes * (args.steps / elapsed) / 1e9, 2), "h2d_link_GBps_measured": round(h2d_peak, 2),
                                  "vs_headline": round((args.steps / e_h) / (args.steps / elapsed), 4)}
                del feed, batches, imgs
            host_fed["note"] = ("every step's camera, target image and mask uploaded from pinned host memory on a copy stream, double-buffered, "
                                "event-ordered in front of the hipGraph replay (train_graph.HostFeed); same runner, same schedule as the headline")
        except Exception as e:   # a secondary timing must never cost the bench line
            host_fed = {"error": repr(e)[:300]}
    # the round-1..3 headline, kept for comparison: ONE static camera and target, no LR change
    static_view = None
    if world == 1 and not force_dist:
        if graph_step is not None:
            graph_step.step(data, gt_img, mask)   # (argument-less steps re-use this view's camera and target)
        sfn = (lambda: graph_step.step()) if graph_step is not None else train_step
        e_s, _, s_s, _ = timed_loop(sfn, args.steps, 10, finish=None if graph_step is None else graph_step.finish, ev_stream=g_stream)
        static_view = {"train_iters_per_s": round(args.steps / e_s, 2), "train_ms": _percentiles(s_s),
                       "note": "the same step replayed on one static camera and target (rounds 1-3's headline)"}
    per_rank = None
    if world > 1 or force_dist:
        # every rank's own clock and step-time distribution, so that ONE multi-GPU run can be read without a second one:
        # [wall seconds of the timed loop, median / p10 / p90 / max step ms (HIP events on the rank's stream)], gathered to all ranks;
        # and the world size as the collective library itself sees it (an all-reduce of ones over the group)
        sm = np.asarray(step_ms, dtype=np.float64)
        mine = torch.tensor([elapsed, float(np.median(sm)), float(np.percentile(sm, 10)), float(np.percentile(sm, 90)), float(sm.max())],
                            device=device, dtype=torch.float64)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        ones = torch.ones((1,), device=device)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        rows_pr = [[round(float(x), 4) for x in t.tolist()] for t in allr]
        ms_pr = [1e3 * r[0] / args.steps for r in rows_pr]
        per_rank = {"columns": ["wall_s", "step_ms_median", "step_ms_p10", "step_ms_p90", "step_ms_max"], "ranks": rows_pr,
                    "ms_per_step_min": round(min(ms_pr), 4), "ms_per_step_median": round(float(np.median(ms_pr)), 4), "ms_per_step_max": round(max(ms_pr), 4),
                    "world_size_seen_by_collective": int(round(float(ones.item()))), "backend": dist.get_backend()}
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    # ---- forward-only render fps (eval path: /root/reference/eval.py:38-43, but synchronised)
    def fwd_only():
        with torch.no_grad():
            model(data)

    trace("graph finished")
    # (at least 30 untimed renders and the clock spin-up first -- a render is not a training step --: with the driver's 5 warm-up
    #  steps 20 timed renders read 2400 fps against 2700 at 200, every one of them 0.405 instead of 0.369 ms)
    fwd_elapsed, _, fwd_ms, _ = timed_loop(fwd_only, args.steps, max(30, args.warmup // 2), spin_up=spin_up if spin_ms > 0 else None)
    trace("forward loop done")

    extras = {}
    if force_dist:
        args.no_extras = args.no_cpu_baseline = True
    if world == 1 and not args.no_extras:
        # the same two numbers with the reference's own (3-sigma) tile lists, i.e. meta's list arrays bit-exact
        ne = min(args.steps, 50)
        # the reference's list mode.  "gsplat" (what rasterization() does by default): gsplat's exact list arrays in meta, built
        # when read, the render walks the short lists;  "gsplat_eager": the render pipeline itself walks gsplat's lists
        lm = {}
        for mode in ("gsplat", "gsplat_eager"):
            model.tile_culling = mode
            e2, q2, s2, w2 = timed_loop(train_step, ne, 10)
            f2, _, fm2, _ = timed_loop(fwd_only, ne, 5)
            lm[mode] = {"train_iters_per_s": round(ne / e2, 2), "train_ms": _percentiles(s2),
                        "forward_fps": round(ne / f2, 2), "forward_ms": _percentiles(fm2),
                        "host_enqueue_ms_per_step": round(1e3 * q2 / ne, 4), "blocked_on_readback_ms_per_step": round(w2, 4)}
            if graph_step is not None:   # the same list mode under the captured step (the runner re-captures on the mode change)
                try:
                    e3, _, s3, _ = timed_loop(graph_step.step, ne, 10, finish=graph_step.finish, ev_stream=g_stream)
                    lm[mode]["graph"] = {"train_iters_per_s": round(ne / e3, 2), "train_ms": _percentiles(s3), "runner": graph_step.report()}
                except Exception as e:
                    lm[mode]["graph"] = {"error": repr(e)[:200]}
        extras["gsplat_list_mode"] = dict(lm["gsplat"], lists_materialised_by_the_render=lm["gsplat_eager"],
                                          note="static view; eager steps (+ the captured step under `graph`) with _tile_culling='gsplat': meta's list "
                                               "arrays are gsplat's, built when read; 'lists_materialised_by_the_render' = 'gsplat_eager'")
        model.tile_culling = "tight"

        def eager_loop_step():
            v = sched.next()
            train_step(datas[v], targets[v])
            model.update_learning_rate(sched.step)

        e4, q4, s4, w4 = timed_loop(eager_loop_step, ne, 10)
        extras["eager_tight"] = {"train_iters_per_s": round(ne / e4, 2), "train_ms": _percentiles(s4),
                                 "host_enqueue_ms_per_step": round(1e3 * q4 / ne, 4), "blocked_on_readback_ms_per_step": round(w4, 4),
                                 "note": "the headline loop (shuffled views, per-step means-LR) enqueued step by step from Python (no hipGraph)"}

        # ---- real_loop: the reference's loop end to end (shuffled views, LR schedule, densify / reset), captured and eager
        try:
            n_rl = int(os.environ.get("GS_BENCH_REAL_LOOP_STEPS", "600"))
            rl = {}
            # (first use of the refinement kernels in this process -- code-object load, first allocations: 13 ms once -- on a
            #  throw-away model, so that neither mode pays it inside its bracket: tools/refine_in_loop.py)
            from easy_gaussian_splatting_amd.synthetic import make_scene
            wm = model_from_scene(make_scene(4096, 64, 64, sh_degree=sc["sh_degree"], seed=1), device)
            build_optimizers(wm, *lrs, fused="hip")
            wm.grad_norm_accum += 1.0
            wm.collecting_counts += 1.0
            wm.densify_and_prune()
            wm.reset_opacities()
            del wm
            for tag, cap in (("captured", True), ("eager", False)):
                rl[tag] = real_loop(sc, device, lrs, datas, targets, mask, steps=n_rl, refine_every=100, reset_at=400, captured=cap)
            rl["what"] = ("reference loop shape end to end at the bench workload: shuffled views, update_statistics + means-LR every "
                          "step, densify_and_prune every 100 steps (one reset_opacities at 400), wall clock INCLUDING re-captures, "
                          "refinement and overflow replays; same seeds in both modes")
            extras["real_loop"] = rl
        except Exception as e:   # a secondary timing must never cost the bench line
            extras["real_loop"] = {"error": repr(e)[:300]}

        # ---- e2e: the reference's acceptance test on a dataset that can be made here (tools/e2e_train.py): nerf_synthetic layout
        # on disk -> Scene -> generate_pointcloud -> from_pointcloud -> nerf_synthetic.yaml's schedule scaled to 3000 steps ->
        # held-out PSNR; the whole run's it/s (re-captures, refinements, resets included), captured and eager
        try:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
            import e2e_train
            e2 = e2e_train.run(3000, ("captured", "eager"))
            extras["e2e"] = {"dataset": e2["dataset"], **{m: {k: r[k] for k in ("train_iters_per_s", "wall_s", "psnr", "ssim", "eval_fps", "n_gaussians_initial",
                                                                                "n_gaussians_final", "active_sh_degree", "schedule", "runner")}
                                                         for m, r in e2["runs"].items()},
                             "what": "scene.Scene(blender) -> from_pointcloud(100 k random points) -> 3000 steps of /root/reference/configs/nerf_synthetic.yaml's "
                                     "schedule (densify every 100 in (100, 1500], reset every 1000, SH degree + 1 every 500, means-LR) -> PSNR on 8 held-out views"}
            rendering.reset_hints()
            torch.cuda.empty_cache()
        except Exception as e:   # a secondary timing must never cost the bench line
            extras["e2e"] = {"error": repr(e)[:300]}

        # ---- drop_in: the reference's own loop body behind the one-line import change (DropInLoop above)
        try:
            di = DropInLoop(sc, device, lrs)
            nd = min(args.steps, 30)
            ed, qd, sd, wd = timed_loop(lambda: di.step(data, gt_img, mask, item_reads=True), nd, 5)
            en, qn, sn, wn = timed_loop(lambda: di.step(data, gt_img, mask, item_reads=False), nd, 3)

            def di_fwd():
                with torch.no_grad():
                    di.forward(data)

            ef, _, sf, _ = timed_loop(di_fwd, nd, 3)
            ph = {}
            for _ in range(5):
                di.step(data, gt_img, mask, item_reads=True, phases=ph)
            torch.cuda.synchronize()
            order = ["start", "forward", "loss", "backward", "item_reads", "update_statistics", "adam"]
            phase_ms = {b: round(float(np.mean([x.elapsed_time(y) for x, y in zip(ph[a], ph[b])])), 3) for a, b in zip(order, order[1:])}
            extras["drop_in"] = {
                "train_iters_per_s": round(nd / ed, 2), "train_ms": _percentiles(sd),
                "forward_fps": round(nd / ef, 2), "forward_ms": _percentiles(sf),
                "host_enqueue_ms_per_step": round(1e3 * qd / nd, 4), "blocked_on_readback_ms_per_step": round(wd, 4),
                "phase_ms": phase_ms,
                "without_item_reads": {"train_iters_per_s": round(nd / en, 2), "train_ms": _percentiles(sn),
                                       "host_enqueue_ms_per_step": round(1e3 * qn / nd, 4)},
                "what": "reference loop body restated (train.py:93-157, model/gaussian.py:97-107,188-197,351-374,389-453) around "
                        "rasterization(): torch exp/sigmoid/cat, gsplat tile lists, torch.clamp, torch L1 + conv2d SSIM, three "
                        ".item() per step, boolean-index update_statistics, torch.optim.Adam (six groups, foreach), eager"}
            del di
            torch.cuda.empty_cache()
            # the next one-line swaps on top of it, the loop otherwise unchanged
            more = {}
            for tag, kw in (("plus_hip_loss", dict(loss="hip")), ("plus_hip_loss_and_adam", dict(loss="hip", adam="hip"))):
                dj = DropInLoop(sc, device, lrs, **kw)
                ej, _, sj, _ = timed_loop(lambda: dj.step(data, gt_img, mask, item_reads=True), nd, 5)
                more[tag] = {"train_iters_per_s": round(nd / ej, 2), "train_ms": _percentiles(sj)}
                del dj
                torch.cuda.empty_cache()
            extras["drop_in"].update(more)
            # the opt-in sync-free seam (`_size_check="deferred"`, SURVEY.md 8b "Sync"): the same loop, the size record read by the
            # call's own backward / the next forward instead of before the forward returns
            dk = DropInLoop(sc, device, lrs, size_check="deferred")
            ek, qk, sk, wk = timed_loop(lambda: dk.step(data, gt_img, mask, item_reads=True), nd, 5)

            def dk_fwd():
                with torch.no_grad():
                    dk.forward(data)

            efk, _, sfk, wfk = timed_loop(dk_fwd, nd, 3)
            rendering.flush_size_checks()
            extras["drop_in"]["deferred_size_check"] = {
                "train_iters_per_s": round(nd / ek, 2), "train_ms": _percentiles(sk), "blocked_on_readback_ms_per_step": round(wk, 4),
                "forward_fps": round(nd / efk, 2), "forward_ms": _percentiles(sfk), "forward_blocked_on_readback_ms": round(wfk, 4),
                "late_overflows": rendering.stats["late_overflows"],
                "note": "opt-in: an overflow found late is repaired in place, but consumers queued in between saw unwritten memory "
                        "(backward refuses) -- hence not the default"}
            del dk
            torch.cuda.empty_cache()
        except Exception as e:   # a secondary timing must never cost the bench line
            extras.setdefault("drop_in", {})["error"] = repr(e)[:300]

        # long lists (what real captures look like to the tile lists): 200 k heavy-tailed splats, mean list ~4.6 k
        try:
            from easy_gaussian_splatting_amd.synthetic import config_long_lists
            ll = config_long_lists(n=200_000, width=1920, height=1080)
            tt = {k: torch.from_numpy(v).to(device) for k, v in ll.items() if isinstance(v, np.ndarray)}
            ins = [tt[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")]
            sh0, shr = tt["shs"][:, :1].contiguous().requires_grad_(True), tt["shs"][:, 1:].contiguous().requires_grad_(True)
            vc = None

            def ll_step(mode):
                nonlocal vc
                img, _, meta = rendering.rasterization(*ins, (sh0, shr), tt["viewmats"], tt["Ks"], 1920, 1080, sh_degree=3, packed=False,
                                                       backgrounds=tt["backgrounds"], absgrad=True, _tile_culling=mode)
                if vc is None:
                    vc = torch.randn_like(img) / (1920 * 1080)
                (img * vc).sum().backward()
                return meta

            out_ll = {}
            for mode in ("gsplat_eager", "tight"):   # (the render pipeline walking gsplat's own lists / the short lists)
                meta_ll = ll_step(mode)
                rendering.profile_stages(True)
                e_ll, _, ms_ll, _ = timed_loop(lambda: ll_step(mode), 10, 2)
                st_ll = rendering.profile_stages(False) or {}
                n_ll = int(meta_ll["flatten_ids"].shape[0])
                out_ll[mode] = {"n_isects": n_ll, "mean_list": round(n_ll / (120 * 68), 1), "fwd_bwd_ms": _percentiles(ms_ll),
                                "binning": rendering.last_binning(device),
                                "stage_ms": {k[3:]: round(float(np.mean(v)), 4) for k, v in sorted(st_ll.items())}}
            extras["long_lists"] = dict(out_ll, workload="200000 heavy-tailed splats (scale 0.02-0.3), 1920x1080, SH3: rasterization fwd+bwd, eager")
            del tt, ins, sh0, shr, vc
            torch.cuda.empty_cache()
        except Exception as e:   # a secondary timing must never cost the bench line
            extras["long_lists"] = {"error": repr(e)[:200]}

    if world == 1 and not args.no_extras and graph_step is not None and not args.no_configs:
        # captured (hipGraph) train step on the real-capture-shaped workloads: heavy-tailed long lists, S3, S5
        from easy_gaussian_splatting_amd.synthetic import config_heavy, config_heavy_5m_4k, config_long_lists, config_s3, config_s5
        from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
        figs = {}
        for name, make, n_steps in (("long_lists_200k_1080p", lambda: config_long_lists(n=200_000, width=1920, height=1080), 30),
                                    ("S3_2M_1080p", lambda: config_s3(), 30), ("S5_5M_4K", lambda: config_s5(), 10),
                                    # the metric's N on a realistic footprint: gsplat's lists hold ~29 entries per Gaussian
                                    ("heavy_1M_1080p", lambda: config_heavy(n=1_000_000), 20),
                                    ("heavy_2M_1080p", lambda: config_heavy(n=2_000_000), 20),
                                    # configs[4] on a realistic footprint: ~28 entries per Gaussian at 4K, I ~ 140 M
                                    ("heavy_5M_4K", lambda: config_heavy_5m_4k(), 10)):
            try:
                t_build = time.perf_counter()
                scx = make()
                mx = model_from_scene(scx, device)
                ox = build_optimizers(mx, *lrs, fused="hip")
                Wx, Hx = scx["width"], scx["height"]
                dx = {"w2c": torch.from_numpy(scx["viewmats"][0]).to(device), "K": torch.from_numpy(scx["Ks"][0]).to(device),
                      "width": Wx, "height": Hx}
                gx = smooth_target(Hx, Wx, 77, device)
                outs = {}
                for mode in ("gsplat_eager", "tight"):   # (gsplat's own lists walked by the captured step / the short lists)
                    mx.tile_culling = mode
                    rendering.reset_hints()   # (the eager seam's idle workspaces of the configuration before: not this runner's memory)
                    torch.cuda.empty_cache()
                    torch.cuda.synchronize()
                    held = torch.cuda.memory_allocated(device)   # model, optimizer state, target: not the runner's either
                    torch.cuda.reset_peak_memory_stats(device)
                    runner = TrainStepGraph(mx, ox, LossComputer(lambda_ssim=0.2, clamp_input=True), dx, gx, None)
                    ex, _, sx, _ = timed_loop(runner.step, n_steps, 5, finish=runner.finish, ev_stream=runner.stream)
                    rep = runner.report()
                    torch.cuda.synchronize()
                    peak, listed = torch.cuda.max_memory_allocated(device), max(1, rep["probed_isects"])
                    outs[mode] = {"train_iters_per_s": round(n_steps / ex, 2), "train_ms": _percentiles(sx),
                                  "n_isects": rep["probed_isects"], "isects_per_gaussian": round(rep["probed_isects"] / max(1, scx["means"].shape[0]), 1),
                                  "longest_list": rep["probed_longest_list"], "binning": rep["binning"], "coarse_entries": rep["probed_coarse_entries"],
                                  "overflows": rep["overflows"], "captures": rep["captures"],
                                  "walked_work_units": rep["seen_work_units"], "gradient_rows": rep["seen_rows"],
                                  # peak of the process while the runner was built and stepped; of which the runner's own
                                  # workspace (everything beyond model + optimizer state + target), in bytes per LISTED intersection
                                  "peak_GiB": round(peak / 2 ** 30, 2), "runner_GiB": round((peak - held) / 2 ** 30, 2),
                                  "runner_bytes_per_listed_isect": round((peak - held) / listed, 1),
                                  # depth rounds (TrainStepGraph rounds="auto"): on where the frame lists several times what its blend walks
                                  "depth_rounds": bool(rep.get("rounds")), "round_fraction": rep.get("round_fraction"),
                                  "listed_per_step": int(runner.buf["info"][0])}
                    del runner
                    if outs[mode]["depth_rounds"]:   # ... and the same step with the list stages in ONE round, same box, same minute
                        runner = TrainStepGraph(mx, ox, LossComputer(lambda_ssim=0.2, clamp_input=True), dx, gx, None, rounds="off")
                        e1, _, s1, _ = timed_loop(runner.step, n_steps, 5, finish=runner.finish, ev_stream=runner.stream)
                        outs[mode]["one_round"] = {"train_iters_per_s": round(n_steps / e1, 2), "train_ms": _percentiles(s1),
                                                   "listed_per_step": int(runner.buf["info"][0])}
                        del runner
                # forward render fps on this workload (eval.py:38-43, 70: one synchronised render per frame through the model, short
                # lists), list stages in one round / in depth rounds (rendering.py GS_ROUNDS: "auto" turns them on from 4 M listed)
                try:
                    mx.tile_culling = "tight"
                    fps = {}
                    for variant in ("off", "auto"):
                        os.environ["GS_ROUNDS"] = variant
                        rendering.reset_hints()
                        with torch.no_grad():
                            for _ in range(4):
                                mx(dx)
                            torch.cuda.synchronize()
                            r0, t0 = rendering.stats["round_calls"], time.perf_counter()
                            for _ in range(30):
                                mx(dx)
                                torch.cuda.synchronize()
                            fps[variant] = {"fps": round(30 / (time.perf_counter() - t0), 1), "two_round_frames": rendering.stats["round_calls"] - r0}
                    outs["forward_fps"] = {"one_round": fps["off"]["fps"], "rounds_auto": fps["auto"]["fps"], "two_round_frames_of_30": fps["auto"]["two_round_frames"]}
                except Exception as e:
                    outs["forward_fps"] = {"error": repr(e)[:200]}
                finally:
                    os.environ.pop("GS_ROUNDS", None)
                    rendering.reset_hints()
                # roofline of the dominant kernel on THIS workload, priced on the entries the kernel actually walked (VERDICT r4
                # missing #4): a saturated tile abandons the rest of its list, so bytes per LISTED entry over the launch time would
                # exceed the HBM peak on the long-list scenes.  Eager steps (model mirror + HIP loss + fused Adam), HIP events
                # around every stage; the walked counts from the forward's own sublists.
                try:
                    lcx = LossComputer(lambda_ssim=0.2, clamp_input=True)
                    def eager_x():
                        o = mx(dx, clamp=False)
                        lcx.get_loss_dict(o["render_img"], gx, None)["total"].backward(gradient=one)
                        mx.update_statistics(dx, o)
                        ox.step(); ox.zero_grad()
                    for _ in range(3):
                        eager_x()
                    rendering.profile_stages(True)
                    for _ in range(5):
                        eager_x()
                    stx = rendering.profile_stages(False) or {}
                    dbgx = {}
                    insx = [p.detach().clone().requires_grad_(True) for p in (mx.means, mx.quats, mx.log_scales, mx.logit_opacities)]
                    _, _, metax = rendering.rasterization(insx[0], insx[1], insx[2], insx[3], (mx.sh_0, mx.sh_rest), dx["w2c"][None], dx["K"][None], Wx, Hx,
                                                          sh_degree=mx.active_sh_degree, packed=False, backgrounds=mx.BACKGROUND[None], absgrad=True,
                                                          _tile_culling="tight", _activations="exp_sigmoid", _debug=dbgx)
                    torch.cuda.synchronize()
                    walked = int(dbgx["walked_isects"])
                    t_b = float(np.mean(stx["gs_blend_bwd"]))
                    algx = 128 * walked + 24 * Hx * Wx
                    outs["roofline"] = {"bound": "hbm", "kernel": "blend_bwd_kernel", "list_mode": "tight", "unit": "walked intersections (those with gradient rows)",
                                        "n_isects_listed": int(metax["flatten_ids"].numel()), "walked_isects": walked,
                                        "walked_quadrant_pairs": int(dbgx["qcnt"].sum()), "algorithmic_bytes": algx,
                                        "avg_launch_ms": round(t_b, 4), "achieved": round(algx / t_b / 1e6, 1), "peak": HBM_PEAK_GBS, "unit_rate": "GB/s",
                                        "frac": round(algx / t_b / 1e6 / HBM_PEAK_GBS, 5),
                                        "eager_stage_ms": {k[3:]: round(float(np.mean(v)), 4) for k, v in sorted(stx.items())}}
                    # ... and of the list stages (SURVEY.md 8d's algorithmic bytes; VERDICT r5 weak #5: on realistic footprints binning is the
                    # largest stage and had no roofline): two-level -- coarse keys emitted (12 I'), sorted per bin (16 I'), refined into
                    # tile lists (24 I' read + 16 I written); per-tile -- 20 N + 12 I emitted, 16 I sorted in LDS, 8 I + 4 tiles of offsets
                    t_bin = float(np.mean(stx["gs_bin_count"])) + float(np.mean(stx["gs_bin_emit_sort"]))
                    n_listed, n_coarse = int(metax["flatten_ids"].numel()), int(outs["tight"].get("coarse_entries") or 0)
                    two_level = rendering.last_binning(device) == "bins"
                    alg_bin = (52 * n_coarse + 16 * n_listed) if two_level else (20 * int(scx["means"].shape[0]) + 36 * n_listed + 4 * (Wx // 16 + 1) * (Hx // 16 + 1))
                    outs["roofline_binning"] = {"bound": "hbm", "stage": "gs_bin_count + gs_bin_emit_sort (" + ("two-level" if two_level else "per-tile") + ")",
                                                "list_mode": "tight", "n_isects_listed": n_listed, "coarse_entries": n_coarse if two_level else None,
                                                "algorithmic_bytes": alg_bin, "stage_ms": round(t_bin, 4), "achieved": round(alg_bin / t_bin / 1e6, 1),
                                                "peak": HBM_PEAK_GBS, "unit_rate": "GB/s", "frac": round(alg_bin / t_bin / 1e6 / HBM_PEAK_GBS, 5),
                                                "share_of_eager_step": round(t_bin / max(1e-9, sum(float(np.mean(v)) for v in stx.values())), 3),
                                                "listed_per_walked": round(n_listed / max(1, walked), 1)}
                    del insx, metax, dbgx
                except Exception as e:
                    outs["roofline"] = {"error": repr(e)[:200]}
                outs["n_gaussians"] = int(scx["means"].shape[0])
                outs["image"] = f"{Wx}x{Hx}"
                outs["setup_s"] = round(time.perf_counter() - t_build, 1)
                figs[name] = outs
                del mx, ox, dx, gx, scx
                torch.cuda.empty_cache()
            except Exception as e:   # a secondary timing must never cost the bench line
                figs[name] = {"error": repr(e)[:300]}
        extras["captured_step_configs"] = dict(figs, note="full train step (fwd + L1/SSIM + bwd + stats + fused Adam) replayed as one "
                                               "hipGraph, same camera every step, synthetic stand-ins of SURVEY.md 8d")

    # ---- per-stage device times (HIP events on the launch stream), outside the timed region
    rendering.profile_stages(True)
    for _ in range(min(args.steps, 20)):
        train_step()
    stages = rendering.profile_stages(False) or {}
    stage_ms = {k: float(np.mean(v)) for k, v in stages.items()}
    # the two blend kernels again, each launched 10 times back to back inside its pair of events (no launch gap, but ten
    # VALU-saturating launches in a row also sit lower on the clock curve: reported next to the single launch, not instead)
    rendering.profile_stages(True, repeat={"gs_blend_fwd": 10, "gs_blend_bwd": 10})
    for _ in range(min(args.steps, 5)):
        train_step()
    iso = rendering.profile_stages(False) or {}
    kernel_ms = {k: float(np.mean(iso[k])) for k in ("gs_blend_fwd", "gs_blend_bwd") if k in iso}
    trace("stage profile done")

    rc = 0
    if rank == 0:
        dbg = {}
        ins = [p.detach().clone().requires_grad_(True) for p in (model.means, model.quats, model.log_scales, model.logit_opacities)]
        _, _, meta = rendering.rasterization(ins[0], ins[1], ins[2], ins[3], (model.sh_0, model.sh_rest),
                                             data["w2c"][None], data["K"][None], W, H,
                                             sh_degree=model.active_sh_degree, packed=False,
                                             backgrounds=model.BACKGROUND[None], absgrad=True, _tile_culling="tight",
                                             _activations="exp_sigmoid", _debug=dbg)
        with torch.no_grad():
            _, _, meta_ref = rendering.rasterization(model.means, model.quats, model.scales, model.opacities, model.shs,
                                                     data["w2c"][None], data["K"][None], W, H,
                                                     sh_degree=model.active_sh_degree, packed=False,
                                                     backgrounds=model.BACKGROUND[None], _tile_culling="gsplat")
        n_isects = int(meta["flatten_ids"].shape[0])          # what the timed launches walk (tight lists)
        n_isects_ref = int(meta_ref["flatten_ids"].shape[0])  # the reference's own lists (gsplat's 3-sigma rectangles)
        n_vis = int((meta["radii"] > 0).sum().item())
        # algorithmic bytes per launch: SURVEY.md section 8d, for the intersections the launch processed
        alg = {"gs_blend_fwd": 40 * n_isects + 20 * H * W,
               "gs_blend_bwd": 40 * n_isects + 24 * H * W + 88 * n_isects}
        kname = {"gs_blend_fwd": "blend_fwd_kernel", "gs_blend_bwd": "blend_bwd_kernel"}
        dom = max(alg, key=lambda k: stage_ms.get(k, 0.0))
        t_ms = stage_ms.get(dom, float("nan"))
        achieved = alg[dom] / (t_ms * 1e-3) / 1e9 if t_ms == t_ms and t_ms > 0 else None
        traffic, traffic_src = pmc_traffic(kname[dom])
        roofline = {"bound": "hbm", "kernel": kname[dom],
                    "achieved": None if achieved is None else round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": None if achieved is None else round(achieved / HBM_PEAK_GBS, 5),
                    "traffic": traffic, "traffic_source": traffic_src,
                    "traffic_note": "[lower, upper] bytes per launch: FETCH_SIZE raw / x2, + WRITE_SIZE (counter calibration per access shape: "
                                    "profiles/r03_traffic_calibration.json); this kernel's reads are 48-byte record gathers: near the lower bound",
                    "algorithmic_bytes": alg[dom], "n_isects_processed": n_isects,
                    "algorithmic_bytes_gsplat_lists": (40 + (88 if dom == "gs_blend_bwd" else 0)) * n_isects_ref + (24 if dom == "gs_blend_bwd" else 20) * H * W,
                    "avg_launch_ms": None if t_ms != t_ms else round(t_ms, 4),
                    "avg_launch_ms_note": "HIP events around the entry point's launches in the eager step, on the launch stream (average over "
                                          "the profiled steps; the launch gaps of eager launches are inside the bracket; gs_blend_bwd = the "
                                          "kernel + the two small launches that group its work units by fill class in front of it)",
                    "back_to_back_launch_ms": None if dom not in kernel_ms else round(kernel_ms[dom], 4),
                    # priced against HBM as the contract asks; the kernel's actual limiter is VALU issue (roofline_compute)
                    "limiter": "valu-issue"}
        # the whole step against the same peak: SURVEY.md 8d's algorithmic bytes per frame for the realised N, N_vis, I (per-tile LDS sort:
        # 16 I), plus the loss (24 HW + 72 HW of maps) and Adam (28 x 59 N) rows of DESIGN.md section 2
        Ng, K_act = args.gaussians, (sc["sh_degree"] + 1) ** 2
        step_bytes = {"project_fwd": 68 * Ng + 20 * Ng, "sh_fwd": (12 * K_act + 12) * n_vis + 12 * Ng, "emit": 20 * Ng + 12 * n_isects,
                      "sort": 16 * n_isects, "offsets": 8 * n_isects + 4 * (W // 16 + 1) * (H // 16 + 1), "blend_fwd": alg["gs_blend_fwd"],
                      "l1_ssim": 2 * (24 + 72) * H * W, "blend_bwd": alg["gs_blend_bwd"],
                      "sh_bwd_project_bwd": (24 + 12 * K_act) * n_vis + 132 * Ng, "adam": 28 * 59 * Ng}
        step_total = sum(step_bytes.values())
        ms_step = 1e3 * elapsed / args.steps
        roofline_step = {"bound": "hbm", "algorithmic_bytes": step_total, "by_stage": step_bytes, "ms_per_step": round(ms_step, 4),
                         "achieved": round(step_total / (ms_step * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(step_total / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         "note": "all stages of one train step (SURVEY.md 8d per-unit figures, SH gradients never materialised: fused Adam) "
                                 "over the timed step; the two blend kernels are issue-bound (roofline_compute), the rest streams"}
        # compute view of the same kernel: (pixel, Gaussian) pairs and VALU wave-instructions against the issue rate
        rc_obj = {"bound": "valu-issue", "kernel": kname[dom]}
        if dom == "gs_blend_bwd" and dbg.get("unit_counter") is not None:
            n_units = int(dbg["unit_counter"].item())
            listed = int(dbg["qcnt"].sum().item())
            ue = int(dbg.get("unit_entries", 64))
            rc_obj.update(work_units=n_units, entries_per_unit=ue, quadrant_entries_listed=listed,
                          pairs_evaluated=n_units * ue * 64, pairs_listed=listed * 64,
                          pairs_evaluated_per_s=None if not t_ms or t_ms != t_ms else round(n_units * ue * 64 / (t_ms * 1e-3), 0))
        sq, sq_src = sq_counters(kname[dom])
        # The shader clock the kernel ACTUALLY ran at (tools/clock_probe.py: every wave's d(s_memtime) / d(s_memrealtime), measured
        # inside blend_bwd itself) and the issue cost of each instruction class at that clock (tools/micro/clock_probe.hip, four
        # waves per SIMD) -- VERDICT r3 item 5: the round-3 line priced the kernel against a self-measured "3.2 nominal cycles".
        clk, clk_src = _profile_json("clock.json")
        clock_mhz, cls_cost = None, {}
        if clk:
            kk = clk.get("kernels", {}).get("blend_bwd_kernel" if dom == "gs_blend_bwd" else "blend_fwd_kernel<train>", {})
            clock_mhz = kk.get("clock_MHz")
            for m in clk.get("micro", []):
                if m.get("waves_per_simd") == 4 and "cycles_per_wave_instr_at_measured_clock" in m:
                    cls_cost[m["kernel"]] = m["cycles_per_wave_instr_at_measured_clock"]
        clock_hz = 1e6 * clock_mhz if clock_mhz else CLOCK_HZ_NOMINAL
        peak_rate = N_SIMD * clock_hz / VALU_CYCLES_PER_WAVE_INST
        rc_obj.update(peak=round(peak_rate / 1e9, 1), unit="G wave-instr/s", clock_mhz=clock_mhz, clock_source=clk_src,
                      peak_note="1024 SIMD-32 x the shader clock measured inside the kernel / 2 cycles per wave64 instruction (the guide's rate)")
        if sq and sq.get("SQ_INSTS_VALU") and t_ms == t_ms and t_ms > 0:
            rate = sq["SQ_INSTS_VALU"] / (t_ms * 1e-3)
            rc_obj.update(valu_wave_insts_per_launch=sq["SQ_INSTS_VALU"], achieved=round(rate / 1e9, 1),
                          frac=round(rate / peak_rate, 4), counters_source=sq_src,
                          counters={k: sq[k] for k in sorted(sq) if k.startswith("SQ_")})
            if dom == "gs_blend_bwd" and {"v_fma_f32", "v_cmp+v_cndmask", "v_exp_f32"} <= set(cls_cost):
                # what this instruction MIX can issue at, from the measured class costs: not a hardware peak, a model of the
                # stream as compiled -- reported so that "how far from the guide's 2 cycles" and "why" are separate numbers
                n_mix = sum(BWD_LOOP_MIX.values())
                cyc = (BWD_LOOP_MIX["simple"] * cls_cost["v_fma_f32"] + BWD_LOOP_MIX["cmp_cndmask"] * cls_cost["v_cmp+v_cndmask"]
                       + BWD_LOOP_MIX["transcendental"] * cls_cost["v_exp_f32"]) / n_mix
                rc_obj["issue_model"] = {
                    "loop_mix_valu_per_step": BWD_LOOP_MIX, "class_cycles_measured": {k: cls_cost[k] for k in ("v_fma_f32", "v_cmp+v_cndmask", "v_exp_f32")},
                    "modelled_cycles_per_wave_instr": round(cyc, 3),
                    "frac_of_modelled_issue_rate": round(rate / (N_SIMD * clock_hz / cyc), 4),
                    "note": "class costs at 4 waves per SIMD (the kernel runs 3: plain fma measured 5.5 / 2.8 / 2.55 / 2.3 cycles at 1 / 2 / 4 / 8 "
                            "waves per SIMD -- a wave cannot issue VALU back to back, the guide's 2 cycles need >= 8 waves); a fraction above 1 "
                            "means hipcc's schedule hides part of the v_cmp -> v_cndmask dependency the micro-kernel exposes"}
        result = headline_line(elapsed)
        result.update({"forward_fps": round(args.steps / fwd_elapsed, 2),
                       "forward_ms": round(1e3 * fwd_elapsed / args.steps, 4),
                       "forward_step_ms": _percentiles(fwd_ms),
                       "stage_ms": {k: round(v, 4) for k, v in sorted(stage_ms.items())},
                       "blend_kernel_ms": {k: round(v, 4) for k, v in sorted(kernel_ms.items())},
                       "roofline": roofline,
                       "roofline_compute": rc_obj,
                       "roofline_step": roofline_step})
        result["config"].update(n_visible=n_vis, n_isects=n_isects, n_isects_gsplat_lists=n_isects_ref)
        if static_view is not None:
            result["static_view"] = static_view
        if lazy_handback is not None:
            result["lazy_handback"] = lazy_handback
        if host_fed is not None:
            result["host_fed"] = host_fed
        if per_rank is not None:
            result["per_rank"] = per_rank
        result.update(extras)
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(sc, args.cpu_sample, args.cpu_reps)
        # the figures a reader of the LAST 1500 characters of this line needs (a record that keeps only the tail of stdout)
        def _g(d, *ks):
            for k in ks:
                d = d.get(k) if isinstance(d, dict) else None
            return d
        cfgs = result.get("captured_step_configs", {})
        result["summary"] = {
            "train_iters_per_s": result["value"], "forward_fps": result.get("forward_fps"), "lazy_handback_it_s": _g(result, "lazy_handback", "train_iters_per_s"),
            "host_fed_it_s": {k: _g(result, "host_fed", k, "train_iters_per_s") for k in ("float32", "uint8")},
            "real_loop_it_s": {k: _g(result, "real_loop", k, "train_iters_per_s") for k in ("captured", "eager")},
            "e2e": {"psnr": _g(result, "e2e", "captured", "psnr"), "it_s": _g(result, "e2e", "captured", "train_iters_per_s"), "n_final": _g(result, "e2e", "captured", "n_gaussians_final")},
            "configs_it_s_gsplat_lists_tight": {k: [_g(v, "gsplat_eager", "train_iters_per_s"), _g(v, "tight", "train_iters_per_s")] for k, v in cfgs.items() if isinstance(v, dict)},
            # [it/s with the list stages in one round, in two depth rounds] where TrainStepGraph's rounds="auto" turned them on (tight lists)
            "configs_it_s_one_round_vs_depth_rounds": {k: [_g(v, "tight", "one_round", "train_iters_per_s"), _g(v, "tight", "train_iters_per_s")]
                                                       for k, v in cfgs.items() if isinstance(v, dict) and _g(v, "tight", "depth_rounds")},
            "configs_forward_fps_one_round_vs_auto": {k: [_g(v, "forward_fps", "one_round"), _g(v, "forward_fps", "rounds_auto")] for k, v in cfgs.items() if isinstance(v, dict)},
            "configs_peak_GiB": {k: _g(v, "gsplat_eager", "peak_GiB") for k, v in cfgs.items() if isinstance(v, dict)},
            "configs_runner_bytes_per_listed_isect": {k: _g(v, "gsplat_eager", "runner_bytes_per_listed_isect") for k, v in cfgs.items() if isinstance(v, dict)},
            "roofline_frac": _g(result, "roofline", "frac"), "cpu_baseline_it_s": _g(result, "cpu_baseline", "value")}
        print(json.dumps(result), flush=True)
    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()
    return rc


def main():
    args = parse_args()
    if os.environ.get("GS_BENCH_FAULT_AFTER"):   # debugging aid: dump every thread's stack after N seconds (and go on)
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["GS_BENCH_FAULT_AFTER"]), repeat=False, file=sys.stderr)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    sys.exit(run_rank(args))


if __name__ == "__main__":
    main()
