#!/usr/bin/env python3
"""More than four feature channels: the native call against the loop a caller writes without it, on the workload of
tools/blend_time.py (config_bench_1m, 1920 x 1080, `_tile_culling="tight"`).   tools/wide_channels_time.py [n_gauss] [--channels 8,16,32]
[--out FILE]

Per D, in one process, alternating step by step, 5 warm-up and 30 timed steps each, device events around every step:
  (a) native : rasterization(colors[N, D])
  (b) sliced : ceil(D / 4) calls on colors[:, first:first+count] plus torch.cat of the images
each as inference (no grad: forward alone) and as training (forward + backward to every input).  Reported: median / min / max per
form, the A/B rule of profiles/stage_calls_ab.json for inference -- median of (a) <= slowest (b) + (b)'s spread --, the per-stage
device times (rendering.profile_stages, a pass of its own: median per launch and launches per step) and
torch.cuda.max_memory_allocated of each form (a pass of its own, from the same starting point).
Then the new streaming kernels on the image / rows of that workload against gs_clamp01 over the same image in the same run (one read,
one write per float: the library's bandwidth yardstick).  One JSON line; nothing is asserted about speed."""
import json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from easy_gaussian_splatting_amd import _native as nat, rendering
from easy_gaussian_splatting_amd.synthetic import config_bench_1m

args = sys.argv[1:]
def opt(name, default):
    if name in args:
        i = args.index(name); v = args[i + 1]; del args[i:i + 2]
        return v
    return default
Ds = [int(x) for x in opt("--channels", "8,16,32").split(",")]
out_path = opt("--out", None)
n = int(args[0]) if args else 1_000_000
W, H, WARM, STEPS = 1920, 1080, 5, 30
dev = torch.device("cuda:0")
sc = config_bench_1m(n=n)
t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
geo = [t[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")]


def raster(colors, bg):
    return rendering.rasterization(*geo, colors, t["viewmats"], t["Ks"], W, H, sh_degree=None, packed=False, backgrounds=bg,
                                   _tile_culling="tight")


def forms(D):
    feats = torch.rand((n, D), generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
    bg = torch.ones((1, D), device=dev)
    vc = torch.randn((1, H, W, D), generator=torch.Generator().manual_seed(1)).to(dev) / (W * H)
    chunks = rendering.channel_chunks(D)

    def native(train):
        with torch.set_grad_enabled(train):
            img = raster(feats, bg)[0]
            if train:
                torch.autograd.grad((img * vc).sum(), geo + [feats])

    def sliced(train):
        with torch.set_grad_enabled(train):
            img = torch.cat([raster(feats[:, f:f + c], bg[:, f:f + c])[0] for f, c in chunks], dim=-1)
            if train:
                torch.autograd.grad((img * vc).sum(), geo + [feats])
    return {"native": native, "sliced": sliced}


def timed(fn, train):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(train); e.record()
    return s, e


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


res = {"n_gauss": n, "width": W, "height": H, "warmup": WARM, "steps": STEPS, "channels": {}}
for D in Ds:
    fs = forms(D)
    r = {"chunks": math.ceil(D / 4)}
    for train in (False, True):
        mode = "training" if train else "inference"
        for _ in range(WARM):
            for f in fs.values(): f(train)
        ev = {k: [] for k in fs}
        for _ in range(STEPS):
            for k, f in fs.items(): ev[k].append(timed(f, train))
        torch.cuda.synchronize()
        r[mode] = {k: summary([s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}
        a, b = r[mode]["native"], r[mode]["sliced"]
        r[mode]["limit"] = round(b["max"] + (b["max"] - b["min"]), 4)
        r[mode]["native_within_limit"] = a["median"] <= r[mode]["limit"]
        r[mode]["native_over_sliced"] = round(a["median"] / b["median"], 4)
        # stage times and memory peaks: passes of their own
        for k, f in fs.items():
            rendering.profile_stages(True)
            for _ in range(10): f(train)
            st = rendering.profile_stages(False)
            r[mode][k]["stage_ms"] = {s[3:]: {"median": round(float(np.median(v)), 4), "per_step": len(v) / 10} for s, v in sorted(st.items())}
            torch.cuda.synchronize(); rendering.reset_hints(); torch.cuda.empty_cache()
            f(train); torch.cuda.synchronize(); base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(3): f(train)
            torch.cuda.synchronize()
            r[mode][k]["peak_MiB"] = round(torch.cuda.max_memory_allocated() / 2**20, 1)
            r[mode][k]["peak_over_resident_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    res["channels"][str(D)] = r
    del fs
    torch.cuda.empty_cache()

# the streaming kernels against gs_clamp01: D = 8 (whole quads: float4) and D = 9's tail (count = 1: floats) on the image, the row fold
# on as many rows as a training step of this workload leaves (about the listed intersections)
L, st = nat.lib(), lambda: torch.cuda.current_stream(dev).cuda_stream
P = W * H
p = lambda x: x.data_ptr()
img8, img9, dense = torch.rand((P, 8), device=dev), torch.rand((P, 9), device=dev), torch.rand((P, 4), device=dev)
n_rows = int(raster(torch.rand((n, 4), device=dev), None)[2]["flatten_ids"].shape[0])
rows, acc = torch.rand((n_rows, 12), device=dev), torch.zeros((n_rows, 12), device=dev)
out3 = torch.empty((P, 3), device=dev)
kernels = {   # name: (call, bytes moved)
    "gs_clamp01": (lambda: L.gs_clamp01(st(), 3 * P, p(img8), None, p(out3)), 8 * 3 * P),
    "gs_chunk_scatter_quad": (lambda: L.gs_chunk_scatter(st(), P, 8, 4, 4, p(dense), p(img8)), 32 * P),
    "gs_chunk_gather_quad": (lambda: L.gs_chunk_gather(st(), P, 8, 4, 4, p(img8), p(dense)), 32 * P),
    "gs_chunk_scatter_tail1": (lambda: L.gs_chunk_scatter(st(), P, 9, 8, 1, p(dense), p(img9)), 8 * P),
    "gs_chunk_gather_tail1": (lambda: L.gs_chunk_gather(st(), P, 9, 8, 1, p(img9), p(dense)), 8 * P),
    "gs_rows_accumulate_first": (lambda: L.gs_rows_accumulate(st(), n_rows, p(rows), p(acc), 1), (32 + 48) * n_rows),
    "gs_rows_accumulate_add": (lambda: L.gs_rows_accumulate(st(), n_rows, p(rows), p(acc), 0), (64 + 32) * n_rows),
}
res["streaming"] = {"n_rows": n_rows}
CALLS = 20
for name, (fn, nbytes) in kernels.items():
    ms = []
    for w in range(1 + 7):   # one warm window, then seven; CALLS calls enqueued back to back per window
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(CALLS): nat.check(fn(), name)
        e.record(); torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / CALLS)
    med = statistics.median(ms[1:])
    res["streaming"][name] = {"median_us": round(1e3 * med, 2), "min_us": round(1e3 * min(ms[1:]), 2), "max_us": round(1e3 * max(ms[1:]), 2),
                              "bytes": nbytes, "GBps": round(nbytes / (1e6 * med), 1)}
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f)
