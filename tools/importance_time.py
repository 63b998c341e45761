#!/usr/bin/env python3
"""Blend-weight scores: rendering.blend_weights against the inference forward and against the workaround a caller writes
without it, on the bench workload (config_bench_1m) and on config_heavy, 1 M Gaussians at 1920 x 1080, `_tile_culling="tight"`.
tools/importance_time.py [n_gauss] [--scenes bench,heavy] [--out FILE]

Per scene, in one process, three repeats; in each the forms alternate step by step, 5 warm-up and 20 timed steps, device events around
every step:
  scores     : blend_weights(...)                                   -- weight_sum, weight_max, hits
  inference  : rasterization(SH colours) under no_grad              -- (a) the frame a viewer renders
  workaround : rasterization(colors = ones[N,1]) + backward of img.sum() to the colours alone   -- (b) yields the sum only
Reported per form: the median of each repeat, their spread (max - min of the three medians).  Acceptance (the scoring call does strictly
less work than the workaround): every repeat's `scores` median below every repeat's `workaround` median by more than the larger of the
two spreads -- `accepted`.  Then, passes of their own: the per-stage device times of `scores` and `workaround`
(rendering.profile_stages: median per launch), which put gs_blend_scores next to gs_blend_bwd on the same walk, and gs_score_accumulate
on the call's [1,N] outputs (20 calls back to back per window, seven windows).  One JSON line."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from easy_gaussian_splatting_amd import rendering
from easy_gaussian_splatting_amd.importance import BlendWeightStats
from easy_gaussian_splatting_amd.synthetic import config_bench_1m, config_heavy

args = sys.argv[1:]
def opt(name, default):
    if name in args:
        i = args.index(name); v = args[i + 1]; del args[i:i + 2]
        return v
    return default
scenes = opt("--scenes", "bench,heavy").split(",")
out_path = opt("--out", None)
n = int(args[0]) if args else 1_000_000
W, H, WARM, STEPS, REPEATS = 1920, 1080, 5, 20, 3
dev = torch.device("cuda:0")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record()
    return s, e


def run(sc):
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
    geo = [t[k] for k in ("means", "quats", "scales", "opacities")]
    N = geo[0].shape[0]
    ones = torch.ones((N, 1), device=dev, requires_grad=True)
    last = {}

    def scores():
        last["scores"] = rendering.blend_weights(*geo, t["viewmats"], t["Ks"], W, H, _tile_culling="tight")

    def inference():
        with torch.no_grad():
            rendering.rasterization(*geo, t["shs"], t["viewmats"], t["Ks"], W, H, sh_degree=int(sc["sh_degree"]), packed=False,
                                    backgrounds=t["backgrounds"], _tile_culling="tight")

    def workaround():
        img = rendering.rasterization(*geo, ones, t["viewmats"], t["Ks"], W, H, sh_degree=None, packed=False, _tile_culling="tight")[0]
        last["sum"] = torch.autograd.grad(img.sum(), [ones])[0]

    fs = {"scores": scores, "inference": inference, "workaround": workaround}
    r = {"n_gauss": N, "medians_ms": {k: [] for k in fs}}
    for _ in range(REPEATS):
        for _ in range(WARM):
            for f in fs.values(): f()
        ev = {k: [] for k in fs}
        for _ in range(STEPS):
            for k, f in fs.items(): ev[k].append(timed(f))
        torch.cuda.synchronize()
        for k, v in ev.items():
            r["medians_ms"][k].append(round(statistics.median(s.elapsed_time(e) for s, e in v), 4))
    med = r["medians_ms"]
    r["spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in med.items()}
    r["gap_ms"] = round(min(med["workaround"]) - max(med["scores"]), 4)
    r["accepted"] = r["gap_ms"] > max(r["spread_ms"]["scores"], r["spread_ms"]["workaround"])
    r["scores_over_workaround"] = round(statistics.median(med["scores"]) / statistics.median(med["workaround"]), 4)
    r["scores_over_inference"] = round(statistics.median(med["scores"]) / statistics.median(med["inference"]), 4)
    # what was measured is the same quantity: the workaround's colour gradient is the weight sum
    ref, got = last["sum"][:, 0].double(), last["scores"]["weight_sum"][0].double()
    r["sum_rel_l2"] = float((got - ref).norm() / ref.norm())
    r["gaussians_hit"] = int((last["scores"]["hits"] > 0).sum())
    for k in ("scores", "workaround"):
        rendering.profile_stages(True)
        for _ in range(10): fs[k]()
        st = rendering.profile_stages(False)
        r[k + "_stage_ms"] = {s[3:]: {"median": round(float(np.median(v)), 4), "per_step": len(v) / 10} for s, v in sorted(st.items())}
    a, b = r["scores_stage_ms"].get("gs_blend_scores"), r["workaround_stage_ms"].get("gs_blend_bwd")
    if a and b:
        r["blend_scores_over_blend_bwd"] = round(a["median"] / b["median"], 4)
    stats, CALLS, ms = BlendWeightStats(N, dev), 20, []
    for w in range(1 + 7):   # one warm window, then seven
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(CALLS): stats.add(last["scores"])
        e.record(); torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / CALLS)
    nbytes = N * (16 + 2 * 28)   # four [1,N] 4-byte inputs; 8 + 4 + 8 + 4 + 4 bytes of totals read and written
    r["gs_score_accumulate"] = {"median_us": round(1e3 * statistics.median(ms[1:]), 2), "min_us": round(1e3 * min(ms[1:]), 2),
                                "max_us": round(1e3 * max(ms[1:]), 2), "GBps": round(nbytes / (1e6 * statistics.median(ms[1:])), 1)}
    return r


res = {"width": W, "height": H, "warmup": WARM, "steps": STEPS, "repeats": REPEATS, "scenes": {}}
for name in scenes:
    sc = {"bench": config_bench_1m, "heavy": config_heavy}[name](n=n)
    res["scenes"][name] = run(sc)
    torch.cuda.empty_cache(); rendering.reset_hints()
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f)
