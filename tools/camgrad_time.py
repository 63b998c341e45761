"""What camera gradients cost: backward time of one eager rasterization() of the bench scene (1 M Gaussians, 1920x1080, SH3) with
and without `_camera_grads=True`, interleaved in one process, by device events: `python tools/camgrad_time.py [reps] [warmup]`.
Prints one JSON line (medians and quartiles in ms).  Under `rocprofv3 --kernel-trace --stats` the same run gives the per-kernel
times of project_cam_kernel / cam_sum_kernel next to project_bwd_kernel."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from easy_gaussian_splatting_amd.rendering import rasterization  # noqa: E402
from easy_gaussian_splatting_amd.synthetic import config_bench_1m  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    dev = torch.device("cuda:0")
    sc = config_bench_1m()
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
    W, H = int(sc["width"]), int(sc["height"])
    leaves = [t[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "shs")]
    vc = torch.randn((1, H, W, 3), generator=torch.Generator().manual_seed(0)).to(dev)
    times = {False: [], True: []}
    for it in range(warmup + reps):
        for cam in (False, True) if it % 2 == 0 else (True, False):
            V = t["viewmats"].clone().requires_grad_(cam)
            img, _, _ = rasterization(*leaves, V, t["Ks"], W, H, sh_degree=3, packed=False, backgrounds=t["backgrounds"],
                                      absgrad=True, _camera_grads=cam)
            loss = (img * vc).sum()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            torch.autograd.grad(loss, leaves + ([V] if cam else []))
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[cam].append(e0.elapsed_time(e1))
    q = lambda x: [round(float(v), 4) for v in np.percentile(x, [25, 50, 75])]
    plain, cam = q(times[False]), q(times[True])
    print(json.dumps({"workload": "config_bench_1m SH3 1920x1080, eager backward (blend bwd + projection bwd), ms [q25, median, q75]",
                      "reps": reps, "backward_ms": plain, "backward_camera_grads_ms": cam,
                      "delta_median_ms": round(cam[1] - plain[1], 4), "delta_pct": round(100 * (cam[1] / plain[1] - 1), 2)}))


if __name__ == "__main__":
    main()
