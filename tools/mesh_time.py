#!/usr/bin/env python3
"""Times the mesh extraction (mesh.py, csrc/gs_tsdf.hip): TSDF integration of one view and marching tetrahedra over the volume.

One process, runs alternating, `--repeats` (3) repeats, HIP events around warm calls (`--calls` (20) back-to-back calls per window
for the sub-millisecond ones, `integrate` and `gs_clamp01`), the median reported with min and max.
Workload: a 1080p `RGB+ED` render of `synthetic.make_scene` folded into 256^3 and 512^3 volumes over the scene's extent.

  integrate  `TSDFVolume.integrate` (one launch, the render read in place) next to the plain-torch way of doing the same: the
             cached `meshgrid` of sample positions projected, the depth image indexed, `torch.where` over the three arrays.  Peak
             memory of both; the bytes the native kernel must move (40 per voxel the view reaches with colour: 20 read, 20
             written) per second, beside what `gs_clamp01` reaches on a buffer of the volume's size in the same run.
  extract    `TSDFVolume.extract` (flags, two scans, the host read, two emit kernels) against nothing: there is no alternative
             on the box.  Vertices, faces, peak memory.

Nothing is asserted about speed.  Run it under a time limit of its own:

    timeout -k 10 600 python tools/mesh_time.py --out profiles/mesh_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, calls=1):
    """(ms per call, the last result): `calls` back-to-back calls between two events, so that a sub-millisecond kernel is timed over
    a window that is not all launch and clock"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, out


def stats(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def peak_of(fn, dev):
    """bytes the call allocates above what is live when it starts"""
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return int(peak)


def torch_integrate(pts, tsdf, weight, color, image, alphas, viewmat, K, trunc, min_alpha, depth_max, max_weight):
    """What a caller would write in torch: -> the new (tsdf, weight, color); pts = the cached meshgrid, three [n] coordinate planes."""
    H, W, _ = image.shape
    px, py, pz = pts
    cam = lambda r: viewmat[r, 0] * px + viewmat[r, 1] * py + viewmat[r, 2] * pz + viewmat[r, 3]
    x, y, z = cam(0), cam(1), cam(2)
    u, v = K[0, 0] * (x / z) + K[0, 2], K[1, 1] * (y / z) + K[1, 2]
    pu, pv = torch.floor(u), torch.floor(v)
    ok = (z > 0) & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    idx = torch.where(ok, pv * W + pu, torch.zeros_like(pu)).long()
    planes = image.reshape(H * W, -1).t().contiguous()   # (channel planes: 1-D gathers)
    d = planes[3][idx]
    texel = torch.stack([planes[0][idx], planes[1][idx], planes[2][idx]], 1)
    ok &= torch.isfinite(d) & (d > 0) & (d <= depth_max) & (alphas.reshape(-1)[idx] >= min_alpha)
    sdf = d - z
    ok &= sdf >= -trunc
    s = torch.clamp(sdf / trunc, max=1.0)
    w1 = weight + 1.0
    new_t = torch.where(ok, (tsdf * weight + s) / w1, tsdf)
    new_c = torch.where(ok[:, None], (color * weight[:, None] + texel) / w1[:, None], color)
    new_w = torch.where(ok, torch.clamp(w1, max=max_weight), weight)
    return new_t, new_w, new_c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_time.json"))
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--gaussians", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window of integrate and gs_clamp01")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_time.py measures on the GPU and found none: nothing measured")
    from easy_gaussian_splatting_amd import mesh
    from easy_gaussian_splatting_amd.model import clamp01
    from easy_gaussian_splatting_amd.rendering import rasterization
    from easy_gaussian_splatting_amd.synthetic import make_scene
    dev = torch.device("cuda", torch.cuda.current_device())
    W, H = 1920, 1080
    sc = make_scene(args.gaussians, W, H, sh_degree=0, n_views=1, seed=7, scale_range=(0.01, 0.05))
    t = lambda k: torch.from_numpy(sc[k]).to(dev)
    with torch.no_grad():
        img, alphas, _ = rasterization(means=t("means"), quats=t("quats"), scales=t("scales"), opacities=t("opacities"), colors=t("shs"),
                                       sh_degree=0, viewmats=t("viewmats"), Ks=t("Ks"), width=W, height=H, backgrounds=t("backgrounds"),
                                       packed=False, render_mode="RGB+ED")
    image, alphas, viewmat, K = img[0].contiguous(), alphas[0].contiguous(), t("viewmats")[0].contiguous(), t("Ks")[0].contiguous()
    res = {"tool": "tools/mesh_time.py", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
           "view": [H, W], "gaussians": args.gaussians, "repeats": args.repeats, "calls_per_window": args.calls, "alpha_coverage": round(float((alphas >= 0.5).float().mean()), 4),
           "volumes": {}}
    for r in args.resolutions:
        vol = mesh.TSDFVolume.from_bounds((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), r, device=dev)
        nx, ny, nz = vol.dims
        n = nx * ny * nz
        kw = dict(depth_channel=3, color_channels=(0, 1, 2), alphas=alphas, min_alpha=0.5)
        ax = [torch.arange(m, device=dev, dtype=torch.float32) * vol.voxel_size + o for m, o in zip(vol.dims, vol.origin)]
        gz, gy, gx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        pts = (gx.reshape(-1).contiguous(), gy.reshape(-1).contiguous(), gz.reshape(-1).contiguous())
        del gx, gy, gz
        fresh = lambda: (torch.ones((n,), device=dev), torch.zeros((n,), device=dev), torch.zeros((n, 3), device=dev))
        targs = (image, alphas, viewmat, K, vol.trunc, 0.5, float("inf"), float("inf"))
        buf = torch.rand((5 * n,), device=dev)   # (the volume's own size: tsdf + weight + colour)

        for warm in (lambda: vol.integrate(image, viewmat, K, **kw), lambda: torch_integrate(pts, *fresh(), *targs), lambda: clamp01(buf)):
            warm()
            torch.cuda.synchronize(dev)
        ours, theirs, clamp = [], [], []
        for _ in range(args.repeats):
            ours.append(timed(lambda: vol.integrate(image, viewmat, K, **kw), args.calls)[0])
            a = fresh()
            theirs.append(timed(lambda: torch_integrate(pts, *a, *targs))[0])
            del a
            clamp.append(timed(lambda: clamp01(buf), args.calls)[0])
        touched = int((vol.weight > 0).sum())
        vol2 = mesh.TSDFVolume(vol.origin, vol.voxel_size, vol.dims, device=dev)
        vol2.integrate(image, viewmat, K, **kw)
        a = fresh()
        tt, tw, tc = torch_integrate(pts, *a, *targs)
        agree = {"weight_equal": round(float((tw == vol2.weight.reshape(-1)).float().mean()), 6),
                 "tsdf_max_abs_diff_where_weights_agree": float(((tt - vol2.tsdf.reshape(-1)).abs() * (tw == vol2.weight.reshape(-1))).max())}
        del tt, tw, tc, a
        peak_hip = peak_of(lambda: vol2.integrate(image, viewmat, K, **kw), dev)
        a = fresh()
        peak_torch = peak_of(lambda: torch_integrate(pts, *a, *targs), dev)
        del a
        moved = 40.0 * touched
        entry = {"dims": list(vol.dims), "voxels": n, "voxels_reached": touched,
                 "integrate": {"hip": stats(ours), "torch_meshgrid_index_where": stats(theirs),
                               "speedup": round(statistics.median(theirs) / statistics.median(ours), 2),
                               "hip_peak_bytes": peak_hip, "torch_peak_bytes": peak_torch, "torch_cached_meshgrid_bytes": int(12 * n),
                               "hip_min_bytes_moved": int(moved), "hip_gbytes_per_s": round(moved / (statistics.median(ours) * 1e-3) / 1e9, 1),
                               "clamp01_same_size": stats(clamp),
                               "clamp01_gbytes_per_s": round(8.0 * buf.numel() / (statistics.median(clamp) * 1e-3) / 1e9, 1), **agree}}
        del pts, buf
        print(json.dumps({str(r): entry["integrate"]}), flush=True)

        vol2.extract(); torch.cuda.synchronize(dev)   # warm
        ex = []
        for _ in range(args.repeats):
            tms, (v, f, c) = timed(lambda: vol2.extract())
            ex.append(tms)
        entry["extract"] = {"hip": stats(ex), "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
                            "hip_peak_bytes": peak_of(lambda: vol2.extract(), dev), "output_bytes": int(24 * v.shape[0] + 12 * f.shape[0])}
        print(json.dumps({str(r): entry["extract"]}), flush=True)
        res["volumes"][str(r)] = entry
        del vol, vol2, v, f, c
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
