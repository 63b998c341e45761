#!/usr/bin/env python3
"""The reference's acceptance test, end to end, on a dataset that can be made here (VERDICT r5 missing #3):

    train on a dataset through the loaders with densify / reset / SH-degree schedule, report held-out PSNR
    (/root/reference/README.md:5-9, train.py:93-157, eval.py:120-133, configs/nerf_synthetic.yaml)

No capture of a real scene exists in this container, so the dataset is rendered: ground-truth Gaussians laid on surfaces
(a sphere, a ground disc, a box; smooth procedural colours with a mild view-dependent SH band) are rendered by the HIP
forward from 40 training and 8 held-out cameras on a dome and WRITTEN TO DISK in nerf_synthetic's layout (RGBA PNGs +
transforms_{train,test}.json, tools/make_synthetic_dataset.py's writer conventions).  Everything after that is the reference's path:

    scene.Scene(data_format="blender")  ->  GaussianModel.from_pointcloud(generate_pointcloud(...): 100 k grey random points)
    ->  configs/nerf_synthetic.yaml's schedule scaled from 30 000 to `steps` iterations (densify every refine_every in
        (refine_start, refine_stop], opacity reset every reset_every, SH degree + 1 every sh_interval, means-LR schedule)
    ->  train_graph.TrainStepGraph (captured) or the eager model / loss / FusedAdam loop
    ->  PSNR / SSIM / fps on the held-out views (eval.py's Evaluator: clamp, mean over views).

    python tools/e2e_train.py [--knn host|device] [--lambda-normal X] [--normal-from STEP] [--geometry] [steps] [captured|eager|both] [out.json]

`--knn device` takes the initial scales from the device's exact 3-NN search (knn.knn_distances) instead of the host's kd-tree;
the default, `host`, is the run every recorded figure was made with.  `--lambda-normal X` (default 0: off) adds X times the
normal-consistency loss of a second, normal render (normals.py) to the eager loop's total from step `--normal-from` on; `--geometry`
adds that loss on the held-out views and the size of the 256^3 mesh to every run's result.  Without them the run is the one it was.
"""
from __future__ import annotations

import json
import math
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

SH_C0 = 0.28209479177387814
FOV_X = 0.6911112070083618   # nerf_synthetic's camera_angle_x


# ------------------------------------------------------------------------------------------------ ground truth
def _frame_from_normal(n: np.ndarray) -> np.ndarray:
    """wxyz quaternions of rotations whose third axis is `n` (unit normals [M, 3])."""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    t1 = np.cross(n, a)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(n, t1)
    R = np.stack([t1, t2, n], axis=2)   # columns
    w = np.sqrt(np.maximum(0.0, 1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2])) / 2.0
    w = np.maximum(w, 1e-6)
    x = (R[:, 2, 1] - R[:, 1, 2]) / (4 * w)
    y = (R[:, 0, 2] - R[:, 2, 0]) / (4 * w)
    z = (R[:, 1, 0] - R[:, 0, 1]) / (4 * w)
    return np.stack([w, x, y, z], axis=1)


def make_ground_truth(seed: int = 0, density: float = 1.0):
    """Gaussians on surfaces: flat (a seventh of their tangent extent along the normal), nearly opaque, coloured by smooth
    functions of the position, with a mild first-band SH term (a sheen that follows the viewing direction)."""
    rng = np.random.default_rng(seed)
    pts, nrm, col, spacing = [], [], [], []

    def add(p, n, c, area):
        pts.append(p); nrm.append(n); col.append(c)
        spacing.append(np.full((p.shape[0],), math.sqrt(area / p.shape[0])))

    # sphere, radius 0.9, centred at (0, 0, 0.1)
    m = int(36000 * density)
    v = rng.standard_normal((m, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    c = 0.5 + 0.45 * np.stack([np.sin(4.0 * v[:, 0] + 1.0) * np.cos(3.0 * v[:, 2]), np.sin(5.0 * v[:, 1]), np.cos(4.0 * v[:, 2] + 2.0 * v[:, 0])], axis=1)
    add(0.9 * v + np.array([0.0, 0.0, 0.1]), v, c, 4 * math.pi * 0.81)
    # ground disc z = -0.8, radius 2.0
    m = int(30000 * density)
    r, th = 2.0 * np.sqrt(rng.random(m)), 2 * math.pi * rng.random(m)
    p = np.stack([r * np.cos(th), r * np.sin(th), np.full(m, -0.8)], axis=1)
    chk = 0.5 + 0.5 * np.tanh(4.0 * np.sin(3.0 * p[:, 0]) * np.sin(3.0 * p[:, 1]))
    c = np.stack([0.25 + 0.5 * chk, 0.3 + 0.4 * chk, 0.7 - 0.4 * chk], axis=1)
    add(p, np.tile(np.array([[0.0, 0.0, 1.0]]), (m, 1)), c, math.pi * 4.0)
    # a box beside the sphere: five visible faces
    ctr, h = np.array([1.35, -0.2, -0.45]), 0.35
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            if axis == 2 and sgn < 0:
                continue
            m = int(2500 * density)
            uv = (rng.random((m, 2)) * 2 - 1) * h
            p = np.zeros((m, 3)); n = np.zeros((m, 3))
            p[:, axis] = sgn * h; p[:, (axis + 1) % 3] = uv[:, 0]; p[:, (axis + 2) % 3] = uv[:, 1]
            n[:, axis] = sgn
            c = np.clip(np.array([[0.85, 0.55, 0.2]]) + 0.25 * np.sin(9.0 * uv[:, :1]) * np.array([[0.3, 1.0, 0.6]]), 0, 1) * (0.75 + 0.08 * axis)
            add(p + ctr, n, c, 4 * h * h)
    pts, nrm, col, spacing = np.concatenate(pts), np.concatenate(nrm), np.concatenate(col), np.concatenate(spacing)
    n = pts.shape[0]
    scales = np.stack([0.75 * spacing, 0.75 * spacing, 0.75 * spacing / 7.0], axis=1) * np.exp(rng.normal(0.0, 0.1, (n, 3)))
    shs = np.zeros((n, 4, 3))
    shs[:, 0] = (np.clip(col, 0.02, 0.98) - 0.5) / SH_C0
    shs[:, 1:4] = 0.12 * nrm[:, :, None] * np.array([[[1.0, 0.9, 0.8]]])   # first band along the normal: brighter when seen head-on
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(means=f32(pts), quats=f32(_frame_from_normal(nrm)), scales=f32(scales), opacities=f32(np.full((n,), 0.97)), shs=f32(shs))


def dome_cameras(n: int, radius: float, seed: int, el_range=(0.25, 1.1)):
    """Blender-convention camera-to-world matrices (X right, Y up, Z back) on a dome, looking at the origin; world Z up."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        az = 2 * math.pi * (i + 0.37 * rng.random()) / n
        el = el_range[0] + (el_range[1] - el_range[0]) * rng.random()
        pos = radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        z = pos / np.linalg.norm(pos)   # camera looks along -Z
        x = np.cross(np.array([0.0, 0.0, 1.0]), z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, pos
        out.append(c2w)
    return out


def write_dataset(root: Path, size: int = 400, n_train: int = 40, n_test: int = 8, seed: int = 0, device="cuda:0"):
    """Renders the ground truth with the HIP forward and writes it in nerf_synthetic's layout.  Returns what went in."""
    from PIL import Image
    from easy_gaussian_splatting_amd.rendering import rasterization
    gt = make_ground_truth(seed)
    dev = torch.device(device)
    t = {k: torch.from_numpy(v).to(dev) for k, v in gt.items()}
    fx = size / (2 * math.tan(FOV_X / 2))
    K = torch.tensor([[fx, 0, size / 2.0], [0, fx, size / 2.0], [0, 0, 1]], dtype=torch.float32, device=dev)
    root.mkdir(parents=True, exist_ok=True)
    for split, n, sd in (("train", n_train, seed + 1), ("test", n_test, seed + 2)):
        (root / split).mkdir(exist_ok=True)
        frames = []
        for i, c2w in enumerate(dome_cameras(n, 4.0, sd)):
            cv = c2w.copy()
            cv[:3, 1:3] *= -1   # blender -> opencv, as scene.load_frames does
            w2c = torch.tensor(np.linalg.inv(cv), dtype=torch.float32, device=dev)
            with torch.no_grad():
                img, alpha, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["shs"], w2c[None], K[None], size, size,
                                              sh_degree=1, packed=False, backgrounds=None)
            a = alpha[0].clamp(0, 1)
            rgb = torch.where(a > 1e-4, img[0] / a.clamp_min(1e-4), torch.zeros_like(img[0])).clamp(0, 1)   # straight (un-premultiplied) colour
            rgba = torch.cat([rgb, a], dim=-1)
            Image.fromarray((rgba * 255.0 + 0.5).to(torch.uint8).cpu().numpy(), "RGBA").save(root / split / f"r_{i}.png")
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(root / f"transforms_{split}.json", "w") as f:
            json.dump({"camera_angle_x": FOV_X, "frames": frames}, f)
    return {"n_gt_gaussians": int(gt["means"].shape[0]), "size": size, "n_train": n_train, "n_test": n_test}


# ------------------------------------------------------------------------------------------------ the reference's loop
def schedule(steps: int):
    """configs/nerf_synthetic.yaml scaled from its 30 000 iterations to `steps` (rounded to the refinement period)."""
    refine_every = max(20, steps // 30)   # (200 of 30 000 is steps / 150: every step would refine a 3 000-step run out of statistics; 1 / 30 keeps ~14 refinements)
    return dict(total_iterations=steps, refine_start=refine_every, refine_stop=steps // 2, refine_every=refine_every,
                reset_opacities_every=10 * refine_every, sh_degree_interval=max(1, steps // 6),
                means_lr_init=1e-3, means_lr_final=1e-5, means_lr_schedule_max_steps=steps, log_scales_lr=1e-2, quats_lr=1e-3,
                sh_0_lr=2.5e-3, sh_rest_lr=1.25e-4, logit_opacities_lr=5e-2, min_opacity=0.005, densify_grad_thresh=5e-4,
                densify_scale_thresh=0.5, num_splits=2, prune_radii_ratio_thresh=0.15, prune_scale_thresh=1.0, lambda_ssim=0.2, sh_degree=3)


@torch.no_grad()
def evaluate(model, eval_datas):
    """eval.py's Evaluator on the held-out views: PSNR and SSIM (data range 1) of the clamped render, mean over views; fps of
    `model(data)` as the reference times it, synchronised."""
    from easy_gaussian_splatting_amd.loss import ssim
    psnr = ss = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = [model(d)["render_img"] for d in eval_datas]
    torch.cuda.synchronize()
    cost = time.perf_counter() - t0
    for d, img in zip(eval_datas, outs):
        mse = torch.mean((img - d["image"]) ** 2)
        psnr += float(-10.0 * torch.log10(mse.clamp_min(1e-12)))
        ss += float(ssim(img.permute(2, 0, 1)[None], d["image"].permute(2, 0, 1)[None]))
    n = max(1, len(eval_datas))
    return {"psnr": psnr / n, "ssim": ss / n, "fps": n / cost, "views": len(eval_datas)}


@torch.no_grad()
def geometry_report(model, eval_datas, resolution: int = 256):
    """What `--geometry` adds to a run: the normal-consistency loss of the model on the held-out views (mean) and the size of the mesh
    `extract_mesh` takes from those views at `resolution`^3."""
    from easy_gaussian_splatting_amd.mesh import extract_mesh
    from easy_gaussian_splatting_amd.normals import normal_consistency_loss, render_normals
    losses = []
    for d in eval_datas:
        rn = render_normals(model, d)
        losses.append(float(normal_consistency_loss(rn["render4"], rn["alphas"], d["K"])))
    v, f, _ = extract_mesh(model, eval_datas, resolution=resolution, color=False)
    return {"normal_loss": round(sum(losses) / max(1, len(losses)), 5), "mesh_resolution": resolution, "mesh_vertices": int(v.shape[0]),
            "mesh_faces": int(f.shape[0])}


def train(data_dir: Path, steps: int = 3000, captured: bool = True, seed: int = 0, device="cuda:0", eval_every: int = 0, knn: str = "host",
          keep=None, lambda_normal: float = 0.0, normal_from: int = 0, geometry: bool = False):
    """`keep`: a dict that receives the trained "model" and the held-out "eval_datas" (tools/compress_time.py exports and re-renders them).
    `lambda_normal` > 0 adds `lambda_normal * normal_consistency_loss` of a second, normal render to the total from step `normal_from`
    on (eager loop only); `geometry` adds `geometry_report` to the result."""
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
    from easy_gaussian_splatting_amd.scene import Scene
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    if lambda_normal > 0 and captured:
        raise SystemExit("--lambda-normal: the normal term runs in the eager loop only (the captured step is out of its scope)")
    if lambda_normal > 0:
        from easy_gaussian_splatting_amd.normals import normal_consistency_loss, render_normals
    cfg = schedule(steps)
    dev = torch.device(device)
    np.random.seed(seed)   # (generate_pointcloud draws from numpy's global generator, as the reference's does)
    torch.manual_seed(seed)
    scene = Scene(str(data_dir), "blender", None, cfg["total_iterations"], eval=True, eval_split_ratio=0.125, eval_in_val=False, eval_in_test=True,
                  use_masks=False, mask_expand_pixels=0, white_background=True)
    model = GaussianModel.from_pointcloud(
        scene.pc, cfg["sh_degree"], cfg["sh_degree_interval"], white_background=True, densify_grad_thresh=cfg["densify_grad_thresh"],
        densify_scale_thresh=cfg["densify_scale_thresh"], num_splits=cfg["num_splits"], prune_radii_ratio_thresh=cfg["prune_radii_ratio_thresh"],
        prune_scale_thresh=cfg["prune_scale_thresh"], min_opacity=cfg["min_opacity"], means_lr_init=cfg["means_lr_init"],
        means_lr_final=cfg["means_lr_final"], means_lr_schedule_max_steps=cfg["means_lr_schedule_max_steps"],
        **({} if knn == "host" else {"knn": knn, "device": dev})).to(dev)
    opt = build_optimizers(model, cfg["means_lr_init"], cfg["log_scales_lr"], cfg["quats_lr"], cfg["sh_0_lr"], cfg["sh_rest_lr"],
                           cfg["logit_opacities_lr"], fused="hip")
    lc = LossComputer(cfg["lambda_ssim"], clamp_input=True)

    def to_dev(d):
        return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}

    # (the frames are decoded once and kept on the device: the per-step host feed is bench.py's `host_fed` figure, not this one's)
    n_train_frames = len(set(scene.train_indexes))
    train_datas = {i: to_dev(scene.frames[i].to_data()) for i in sorted(set(scene.train_indexes))}
    eval_datas = [to_dev(scene.get_data("eval", i)) for i in range(scene.nbr_data("eval"))]
    order = torch.randperm(len(scene.train_indexes), generator=torch.Generator().manual_seed(seed)).tolist()   # DataLoader(shuffle=True)
    gen = torch.Generator(device=dev).manual_seed(seed + 7)
    first = train_datas[scene.train_indexes[order[0]]]
    runner = TrainStepGraph(model, opt, lc, first, first["image"], None, handback="lazy") if captured else None
    one = torch.ones((), device=dev)
    n_hist, evals = [model.nbr_gaussians], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(1, steps + 1):
        d = train_datas[scene.train_indexes[order[step - 1]]]
        if runner is not None:
            runner.step(d, d["image"])
        else:
            out = model(d, clamp=False)
            if lambda_normal > 0 and step >= normal_from:
                rn = render_normals(model, d)
                total = lc.get_loss_dict(out["render_img"], d["image"], None)["total"]
                (total + lambda_normal * normal_consistency_loss(rn["render4"], rn["alphas"], d["K"])).backward(gradient=one)
            else:
                lc.get_loss_dict(out["render_img"], d["image"], None)["total"].backward(gradient=one)
            model.update_statistics(d, out)
            opt.step(); opt.zero_grad()
        # refinement: the reference collects statistics inside (refine_start, refine_stop] only -- the step here always does,
        # so what it gathered up to refine_start is dropped there
        if step == cfg["refine_start"]:
            if runner is not None:
                runner.fence()
            model.grad_norm_accum.zero_(); model.collecting_counts.zero_(); model.max_radii.zero_()
        if cfg["refine_start"] < step <= cfg["refine_stop"]:
            if (step - cfg["refine_start"]) % cfg["refine_every"] == 0:
                if runner is not None:
                    runner.finish()
                model.densify_and_prune(generator=gen)
                n_hist.append(model.nbr_gaussians)
            if (step - cfg["refine_start"]) % cfg["reset_opacities_every"] == 0:
                if runner is not None:
                    runner.finish()
                model.reset_opacities()
        if cfg["sh_degree_interval"] and step % cfg["sh_degree_interval"] == 0:
            model.up_sh_degree()
        model.update_learning_rate(step)
        if eval_every and step % eval_every == 0:
            if runner is not None:
                runner.finish()
            evals.append(dict(step=step, **evaluate(model, eval_datas)))
    if runner is not None:
        runner.finish()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    final = evaluate(model, eval_datas)
    rep = runner.report() if runner is not None else None
    if keep is not None:
        keep["model"], keep["eval_datas"] = model, eval_datas
    extra = {}
    if lambda_normal > 0:
        extra.update(lambda_normal=lambda_normal, normal_from=normal_from)
    if geometry:
        extra["geometry"] = geometry_report(model, eval_datas)
    res = {"mode": "captured" if captured else "eager", "steps": steps, "wall_s": round(wall, 3), "train_iters_per_s": round(steps / wall, 1),
            "psnr": round(final["psnr"], 3), "ssim": round(final["ssim"], 4), "eval_fps": round(final["fps"], 1), "held_out_views": final["views"],
            "train_views": n_train_frames, "n_gaussians_initial": n_hist[0], "n_gaussians_final": model.nbr_gaussians, "n_gaussians": n_hist,
            "active_sh_degree": int(model.active_sh_degree), "schedule": {k: cfg[k] for k in ("refine_start", "refine_stop", "refine_every",
                                                                                             "reset_opacities_every", "sh_degree_interval")},
            "evals": evals, "runner": None if rep is None else {k: rep[k] for k in ("captures", "overflows", "replayed_steps", "rebuilds", "projected_rebuilds", "build_ms",
                                                                             "capture_ms", "pool_allocs", "binning", "overflow_log") if k in rep}}
    res.update(extra)
    return res


def run(steps: int = 3000, modes=("captured", "eager"), size: int = 400, out_dir=None, eval_every: int = 0, knn: str = "host",
        lambda_normal: float = 0.0, normal_from: int = 0, geometry: bool = False):
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(out_dir) if out_dir else Path(tmp) / "synthetic_dome"
        t0 = time.perf_counter()
        ds = write_dataset(root, size=size)
        ds["write_s"] = round(time.perf_counter() - t0, 2)
        res = {"dataset": dict(ds, layout="nerf_synthetic (transforms_{train,test}.json + RGBA PNGs), rendered by the HIP forward from ground-truth "
                                           "Gaussians on a sphere, a ground disc and a box; white background"),
               "runs": {m: train(root, steps, captured=(m == "captured"), eval_every=eval_every, knn=knn, lambda_normal=lambda_normal,
                                   normal_from=normal_from, geometry=geometry) for m in modes}}
    if knn != "host":
        res["knn"] = knn
    return res


def split_knn_option(argv):
    """(`--knn host|device` or `--knn=...` taken out of argv, the remaining positional arguments)."""
    knn, rest, i = "host", [], 0
    while i < len(argv):
        a = argv[i]
        if a == "--knn":
            if i + 1 >= len(argv):
                raise SystemExit("--knn needs a value: host or device")
            knn, i = argv[i + 1], i + 1
        elif a.startswith("--knn="):
            knn = a[len("--knn="):]
        else:
            rest.append(a)
        i += 1
    if knn not in ("host", "device"):
        raise SystemExit(f"--knn: host or device, got {knn!r}")
    return knn, rest


def split_normal_options(argv):
    """(`--lambda-normal X`, `--normal-from STEP` and `--geometry` taken out of argv -- 0.0, 0 and False when absent --, the rest)."""
    lam, start, geometry, rest, i = 0.0, 0, False, [], 0
    while i < len(argv):
        a = argv[i]
        name, eq, val = a.partition("=")
        if name in ("--lambda-normal", "--normal-from"):
            if not eq:
                if i + 1 >= len(argv):
                    raise SystemExit(f"{name} needs a value")
                val, i = argv[i + 1], i + 1
            if name == "--lambda-normal":
                lam = float(val)
            else:
                start = int(val)
        elif a == "--geometry":
            geometry = True
        else:
            rest.append(a)
        i += 1
    if not lam >= 0.0 or start < 0:
        raise SystemExit("--lambda-normal must be >= 0 and --normal-from a step >= 0")
    return lam, start, geometry, rest


if __name__ == "__main__":
    knn_mode, argv = split_knn_option(sys.argv[1:])
    lambda_normal, normal_from, geometry, argv = split_normal_options(argv)
    steps = int(argv[0]) if len(argv) > 0 else 3000
    which = argv[1] if len(argv) > 1 else "both"
    res = run(steps, ("captured", "eager") if which == "both" else (which,), eval_every=int(os.environ.get("GS_E2E_EVAL_EVERY", "0")),
              knn=knn_mode, lambda_normal=lambda_normal, normal_from=normal_from, geometry=geometry)
    txt = json.dumps(res)
    if len(argv) > 2:
        open(argv[2], "w").write(txt + "\n")
    print(txt)
