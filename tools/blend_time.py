#!/usr/bin/env python3
"""Kernel times of the rasterizer's stages on a FIXED scene (no optimizer in the loop): rasterization forward + backward of the
bench workload, HIP events around every stage (rendering.profile_stages), 30 repetitions.  For A/B runs of library variants
whose backward may be numerically wrong on purpose (timing experiments):  GS_LIB_PATH=... tools/blend_time.py [n_gauss]
`--channels D`: non-SH colour features [N, D] with backgrounds [1, D] instead of the SH colours (D = 3: the RGB path
with pre-activated colours; D = 1, 2, 4: the channel entry points; D > 4: chunks of four over one set of lists, without `absgrad`,
which such a call refuses -- a stage that runs once per chunk is reported as the median of all its launches).
`--render-mode M[,M...]` (RGB, D, ED, RGB+D, RGB+ED): the render modes to time; several are interleaved step by step in this one
process (an A/B on one box) and reported one JSON line each."""
import json, os, sys
ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
import numpy as np, torch
from easy_gaussian_splatting_amd import rendering
from easy_gaussian_splatting_amd.synthetic import config_bench_1m
args = sys.argv[1:]
channels = None
if "--channels" in args:
    i = args.index("--channels")
    channels = int(args[i + 1])
    del args[i:i + 2]
modes = ["RGB"]
if "--render-mode" in args:
    i = args.index("--render-mode")
    modes = args[i + 1].split(",")
    del args[i:i + 2]
n = int(args[0]) if args else 1_000_000
dev = torch.device("cuda:0")
sc = config_bench_1m(n=n)
t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
ins = [t[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")]
sh0, shr = t["shs"][:, :1].contiguous().requires_grad_(True), t["shs"][:, 1:].contiguous().requires_grad_(True)
if channels is not None:
    feats = torch.rand((n, channels), generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
    bg = torch.ones((1, channels), device=dev)
vcs = {}
def step(mode="RGB"):
    if channels is None:
        img, _, meta = rendering.rasterization(*ins, (sh0, shr), t["viewmats"], t["Ks"], 1920, 1080, sh_degree=3, packed=False,
                                               backgrounds=t["backgrounds"], absgrad=True, _tile_culling="tight", render_mode=mode)
        params = ins + [sh0, shr]
    else:
        img, _, meta = rendering.rasterization(*ins, feats, t["viewmats"], t["Ks"], 1920, 1080, sh_degree=None, packed=False,
                                               backgrounds=bg, absgrad=channels <= 4, _tile_culling="tight", render_mode=mode)
        params = ins + [feats]
    if mode not in vcs:
        vcs[mode] = torch.randn_like(img) / (1920 * 1080)
    torch.autograd.grad((img * vcs[mode]).sum(), params, allow_unused=True)   # (D / ED: the colours receive no gradient)
    return meta
for m in modes:
    meta = step(m)
for _ in range(5):
    for m in modes: step(m)
rendering.profile_stages(True)
events = {m: {} for m in modes}
for _ in range(30):
    for m in modes:
        rendering._prof = events[m]   # (one event dictionary per mode: no synchronisation between the steps)
        step(m)
rendering.profile_stages(False)
torch.cuda.synchronize()
times = {m: {k: [s.elapsed_time(e) / r for s, e, r in v] for k, v in events[m].items()} for m in modes}
for m in modes:
    print(json.dumps({"lib": os.path.basename(os.environ.get("GS_LIB_PATH", "libgsraster.so")), "channels": channels, "render_mode": m,
                      "n_isects": int(meta["flatten_ids"].shape[0]),
                      **{k[3:]: round(float(np.median(v)), 4) for k, v in sorted(times[m].items())}}))
