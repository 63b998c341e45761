#!/usr/bin/env python3
"""Times the device k-NN initialisation (knn.knn_distances, GaussianModel.from_pointcloud(knn="device")) next to the host path
(sklearn's kd-tree on one CPU thread, the default of from_pointcloud) on the same machine.

Workloads (seeded, generated here): 100 k and 1 M uniform points, 1 M clustered points (200 centres, per-POINT spread over four
decades: an SfM-like density range), 5 M uniform points.  Per workload:

    knn_ms          device time of knn_distances(points, 3): HIP events around one call, warm, the median of `--calls` calls
                    (codes + torch.sort + gather + boxes + search; check_finite off: its read-back is no device work)
    device_init_s   wall time of from_pointcloud(knn="device") from the float64 host cloud to a synchronised model, upload included
    host_init_s     wall time of from_pointcloud(knn="host") for the workloads in `--host` (the code every earlier revision runs);
                    skipped with a note when scikit-learn is not installed
    sample_err_u    the worst relative error, in units of 2^-24, of 64 sampled rows against float64 brute force on the device

One process, no file read outside the repository, nothing asserted about speed.  Run it under a time limit of its own:

    timeout -k 10 900 python tools/knn_time.py --out profiles/knn_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def clustered(n, seed, n_centres=200):
    rng = np.random.default_rng(seed)
    centres = rng.random((n_centres, 3)) * 10.0
    spread = 10.0 ** rng.uniform(-4.0, 0.0, n)          # per point, four decades
    return centres[rng.integers(0, n_centres, n)] + spread[:, None] * rng.standard_normal((n, 3))


WORKLOADS = {"100k_uniform": lambda: uniform(100_000, 1), "1m_uniform": lambda: uniform(1_000_000, 2),
             "1m_clustered": lambda: clustered(1_000_000, 3), "5m_uniform": lambda: uniform(5_000_000, 4)}


def sample_error(points32, dists, n_rows=64):
    """Worst relative error (in u = 2^-24) of `n_rows` sampled rows against float64 brute force over the whole cloud."""
    n = points32.shape[0]
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:n_rows].to(points32.device)
    p = points32.double()
    d2 = torch.zeros((rows.numel(), n), dtype=torch.float64, device=p.device)
    for a in range(3):
        d2 += (p[rows, a, None] - p[None, :, a]) ** 2
    d2[torch.arange(rows.numel(), device=p.device), rows] = float("inf")
    ref = torch.sqrt(torch.topk(d2, dists.shape[1], dim=1, largest=False, sorted=True).values)
    got = dists[rows].double()
    rel = torch.where(ref > 0, (got - ref).abs() / ref.clamp_min(1e-300), (got != 0).double() * float("inf"))
    return float(rel.max()) / 2.0 ** -24


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_time.json"))
    ap.add_argument("--calls", type=int, default=11, help="timed calls of knn_distances per workload (>= 10)")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--host", default="100k_uniform,1m_uniform", help="workloads that also time the host path ('' = none)")
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls: at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("knn_time.py measures on the GPU and found none: nothing measured")
    from easy_gaussian_splatting_amd.knn import knn_distances
    from easy_gaussian_splatting_amd.model import GaussianModel
    from easy_gaussian_splatting_amd.scene import Pointcloud
    try:
        import sklearn
        sk = sklearn.__version__
    except ImportError:
        sk = None
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"tool": "tools/knn_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
           "sklearn": sk, "k": 3, "calls": args.calls, "host_threads_note": "sklearn's kneighbors runs on one CPU thread (n_jobs=None)",
           "workloads": {}}
    host_set = {w for w in args.host.split(",") if w}
    for name in [w for w in args.workloads.split(",") if w]:
        x64 = WORKLOADS[name]()
        n = x64.shape[0]
        pc = Pointcloud(x64, np.full((n, 3), 127, dtype=np.uint8))
        centred = torch.from_numpy((x64 - 0.5 * (x64.min(axis=0) + x64.max(axis=0))).astype(np.float32)).to(dev)
        for _ in range(2):   # warm: code objects, the sort's temporary storage, the allocator
            d = knn_distances(centred, 3, check_finite=False)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d = knn_distances(centred, 3, check_finite=False)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        row = {"n": n, "knn_ms": round(statistics.median(ms), 3), "knn_ms_min": round(min(ms), 3), "knn_ms_max": round(max(ms), 3),
               "sample_err_u": round(sample_error(centred, d), 2), "mean_3nn_distance": float(d.mean())}
        del d, centred
        walls = []
        for _ in range(2):   # (the second call is the warm one; both are reported)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            m = GaussianModel.from_pointcloud(pc, 3, knn="device", device=dev)
            torch.cuda.synchronize(dev)
            walls.append(round(time.perf_counter() - t0, 4))
            del m
        row["device_init_s"], row["device_init_s_first"] = walls[1], walls[0]
        if name in host_set:
            if sk is None:
                row["host_init_s"], row["host_note"] = None, "scikit-learn is not installed here: the host path was not timed"
            else:
                t0 = time.perf_counter()
                m = GaussianModel.from_pointcloud(pc, 3)
                row["host_init_s"] = round(time.perf_counter() - t0, 3)
                del m
        res["workloads"][name] = row
        print(json.dumps({name: row}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
