#!/usr/bin/env python3
"""Times the device k-means (kmeans.py, csrc/gs_kmeans.hip) against what a caller would write in torch, and a whole export.

One process, runs alternating, `--repeats` (3) repeats, HIP events around warm calls, the median reported with min and max.

  assign    1 M x 45 floats at the scale of a trained sh_rest against K = 65 536 centroids (5.9 TFLOP): `gs_kmeans_assign` (prep +
            fused product + argmin, no score stored) next to the torch workaround, chunked `x @ c.T` + `argmin` with the chunk sized so
            that the score block stays at or under 1 GiB.  Achieved TFLOP/s beside the 122 TF of an untuned f32-MFMA GEMM and the
            157 TF peak; the fraction of labels on which the two agree (they differ where float32 cannot tell two centroids apart).
  update    `kmeans.update` (stable sort + bincount + `gs_kmeans_update`) and the kernel alone, next to `index_add_` + a division.
  export    a whole `save_compact` (5 Lloyd iterations, 65 536 clusters) of a 1 M-Gaussian SH-3 model: seconds, file bytes per
            Gaussian next to the pickled .pth's.
  psnr      the tools/e2e_train.py run (`--steps`, captured) exported and loaded again: PSNR of the compact model's renders of
            the held-out views against the uncompressed model's, and each against the ground truth; file sizes of the .pth, the
            .ply and the compact file.  `--steps 0` skips it.

Nothing is asserted about speed.  Run it under a time limit of its own:

    timeout -k 10 900 python tools/compress_time.py --out profiles/compress_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNTUNED_GEMM_TF, PEAK_TF = 122.0, 157.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def torch_assign(x, c, chunk):
    cn = (c * c).sum(1)
    labels = torch.empty((x.shape[0],), dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        labels[i:i + chunk] = torch.argmin(torch.addmm(cn[None, :], x[i:i + chunk], c.t(), alpha=-2.0), dim=1)
    return labels


def torch_update(x, labels, c):
    sums = torch.zeros(c.shape, dtype=torch.float64, device=x.device).index_add_(0, labels, x.double())
    counts = torch.bincount(labels, minlength=c.shape[0])
    return torch.where(counts[:, None] > 0, (sums / counts.clamp_min(1)[:, None]).float(), c), counts


def sh_like(n, d, dev, seed):
    """`n` rows of `d` floats at the scale of a trained sh_rest: a few hundred loose clusters, bands fading with the degree"""
    g = torch.Generator().manual_seed(seed)
    band = torch.cat([torch.full((9,), 0.08), torch.full((15,), 0.05), torch.full((21,), 0.03)])[:d] if d == 45 else torch.full((d,), 0.05)
    centres = torch.randn(512, d, generator=g) * band
    return (centres[torch.randint(0, 512, (n,), generator=g)] + 0.4 * torch.randn(n, d, generator=g) * band).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_time.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3000, help="iterations of the tools/e2e_train.py run behind the PSNR figure (0: skip)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compress_time.py measures on the GPU and found none: nothing measured")
    from easy_gaussian_splatting_amd import _native as nat
    from easy_gaussian_splatting_amd import compress as C
    from easy_gaussian_splatting_amd import kmeans as KM
    from easy_gaussian_splatting_amd.checkpoint import save_gaussian_model, save_ply
    from easy_gaussian_splatting_amd.model import GaussianModel
    dev = torch.device("cuda", torch.cuda.current_device())
    n, k, d = args.n, args.k, 45
    res = {"tool": "tools/compress_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
           "n": n, "k": k, "d": d, "repeats": args.repeats}
    x = sh_like(n, d, dev, 1)
    c = x[torch.randperm(n, generator=torch.Generator().manual_seed(2))[:k].to(dev)].contiguous()
    chunk = max(1, (1 << 30) // (4 * k))
    L, st = nat.lib(), torch.cuda.current_stream(dev).cuda_stream

    # ---- assign ----
    KM.assign(x, c); torch_assign(x, c, chunk); torch.cuda.synchronize(dev)   # warm
    ours, theirs = [], []
    for _ in range(args.repeats):
        t, (labels, dist2) = timed(lambda: KM.assign(x, c))
        ours.append(t)
        t, tl = timed(lambda: torch_assign(x, c, chunk))
        theirs.append(t)
    flop = 2.0 * n * k * d
    res["assign"] = {"hip": stats(ours), "torch_chunked_matmul_argmin": stats(theirs), "torch_chunk_rows": chunk,
                     "hip_tflops": round(flop / (statistics.median(ours) * 1e-3) / 1e12, 1),
                     "torch_tflops": round(flop / (statistics.median(theirs) * 1e-3) / 1e12, 1),
                     "untuned_f32_mfma_gemm_tflops": UNTUNED_GEMM_TF, "peak_f32_tflops": PEAK_TF,
                     "speedup": round(statistics.median(theirs) / statistics.median(ours), 2),
                     "labels_agree": round(float((labels.long() == tl).double().mean()), 6)}
    print(json.dumps({"assign": res["assign"]}), flush=True)

    # ---- update ----
    order = torch.sort(labels, stable=True).indices.to(torch.int32)
    seg = torch.zeros((k + 1,), dtype=torch.int32, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(labels, minlength=k), 0)
    counts = torch.empty((k,), dtype=torch.int32, device=dev)
    c1 = c.clone()

    def kernel_only():
        nat.check(L.gs_kmeans_update(st, n, k, d, x.data_ptr(), order.data_ptr(), seg.data_ptr(), c1.data_ptr(), counts.data_ptr()), "gs_kmeans_update")
    l64 = labels.long()
    KM.update(x, labels, c.clone()); kernel_only(); torch_update(x, l64, c); torch.cuda.synchronize(dev)
    whole, kern, theirs = [], [], []
    for _ in range(args.repeats):
        c2 = c.clone()
        whole.append(timed(lambda: KM.update(x, labels, c2))[0])
        kern.append(timed(kernel_only)[0])
        t, (tc, _) = timed(lambda: torch_update(x, l64, c))
        theirs.append(t)
    res["update"] = {"hip_with_sort": stats(whole), "hip_kernel": stats(kern), "torch_index_add_div": stats(theirs),
                     "speedup_with_sort": round(statistics.median(theirs) / statistics.median(whole), 2),
                     "max_abs_diff_to_torch": float((c2 - tc).abs().max())}
    print(json.dumps({"update": res["update"]}), flush=True)
    del order, seg, l64, tl, labels, dist2

    # ---- a whole export ----
    with tempfile.TemporaryDirectory() as tmp:
        g = torch.Generator().manual_seed(3)
        big = GaussianModel(means=3 * torch.randn(n, 3, generator=g), log_scales=torch.randn(n, 3, generator=g) - 4, quats=torch.randn(n, 4, generator=g),
                            sh_0=torch.randn(n, 1, 3, generator=g), sh_rest=x.cpu().reshape(n, 15, 3), logit_opacities=2 * torch.randn(n, generator=g),
                            sh_degree=3).to(dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        C.save_compact(big, os.path.join(tmp, "big.compact"), sh_clusters=k, generator=torch.Generator().manual_seed(4))
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        save_gaussian_model(Path(tmp) / "big.pth", big)
        res["export_1m"] = {"save_compact_s": round(wall, 2), "compact_bytes_per_gaussian": round(os.path.getsize(os.path.join(tmp, "big.compact")) / n, 2),
                            "pth_bytes_per_gaussian": round(os.path.getsize(os.path.join(tmp, "big.pth")) / n, 2),
                            "note": "random geometry (deflate finds nothing in it), sh_rest = the assign workload"}
        print(json.dumps({"export_1m": res["export_1m"]}), flush=True)
        del big, x, c

        # ---- the trained model ----
        if args.steps > 0:
            import e2e_train as E
            keep = {}
            ds = E.write_dataset(Path(tmp) / "dome")
            run = E.train(Path(tmp) / "dome", args.steps, captured=True, keep=keep)
            model, eval_datas = keep["model"], keep["eval_datas"]
            t0 = time.perf_counter()
            C.save_compact(model, os.path.join(tmp, "m.compact"), generator=torch.Generator().manual_seed(5))
            wall = time.perf_counter() - t0
            save_gaussian_model(Path(tmp) / "m.pth", model)
            save_ply(model, os.path.join(tmp, "m.ply"))
            back = C.load_compact(os.path.join(tmp, "m.compact"), device=dev)

            def psnr(a, b):
                return float(-10.0 * torch.log10(torch.mean((a - b) ** 2).clamp_min(1e-12)))
            with torch.no_grad():
                rows = [(model(dd)["render_img"], back(dd)["render_img"], dd["image"]) for dd in eval_datas]
            nm = model.nbr_gaussians
            res["trained"] = {"e2e": {kk: run[kk] for kk in ("steps", "psnr", "ssim", "n_gaussians_final", "active_sh_degree")}, "dataset_views": ds.get("n_test"),
                              "save_compact_s": round(wall, 2), "sh_clusters": min(65536, nm),
                              "psnr_compact_vs_uncompressed": round(statistics.mean(psnr(a, b) for a, b, _ in rows), 2),
                              "psnr_uncompressed_vs_truth": round(statistics.mean(psnr(a, t) for a, _, t in rows), 2),
                              "psnr_compact_vs_truth": round(statistics.mean(psnr(b, t) for _, b, t in rows), 2),
                              "bytes_per_gaussian": {kind: round(os.path.getsize(os.path.join(tmp, "m." + kind)) / nm, 2) for kind in ("pth", "ply", "compact")}}
            print(json.dumps({"trained": res["trained"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
