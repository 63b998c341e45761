"""Where a viewer frame's time goes: `python tools/viewer_time.py [H W [frames [n_gaussians]]]` takes a `FrameRenderer`'s frame apart
at one size (default 1080 1920, 48 frames on an orbit, the bench scene's 1 M Gaussians) and sets it beside the parent's way --
`model(data)["render_img"].cpu().numpy()`, then numpy padding for the client's aspect, then numpy `floor(x * 255).astype(uint8)`
-- measured in the same process.  Prints one JSON line.

Device time from events (medians): `render_ms` (`model(data, clamp=False)`), `finish_*_us` (`gs_frame_finish`: uint8, float32,
float32 padded to aspect 2, the depth grey), `range_us` (`gs_frame_range`), `copy_*_ms` (the frame into page-locked memory).
Host wall time (medians): `render_call_*_ms` (`FrameRenderer.render`), `parent_*_ms`.  `path_fps_*`: frames per second of
`render_path` with a consumer that does nothing; `parent_video_fps`: of the parent's per-frame loop with its host quantisation."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from easy_gaussian_splatting_amd.checkpoint import CameraState  # noqa: E402
from easy_gaussian_splatting_amd.model import GaussianModel  # noqa: E402
from easy_gaussian_splatting_amd.synthetic import make_scene  # noqa: E402
from easy_gaussian_splatting_amd.viewer import FrameRenderer, aspect_size, finish_frame, frame_depth_range  # noqa: E402


def med(xs):
    return round(float(np.median(xs)), 4)


def device_ms(fn, reps, inner=1):
    """median device time of fn() in ms (inner calls between one pair of events)"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out))


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    H = int(sys.argv[1]) if len(sys.argv) > 1 else 1080
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    n = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
    dev = torch.device("cuda:0")
    sc = make_scene(n, W, H, sh_degree=3, n_views=frames, seed=42, extent=(4, 2.25, 4), scale_range=(0.003, 0.03), dist=8.0, white_bg=False)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    model = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=T(sc["shs"][:, :1].copy()),
                          sh_rest=T(sc["shs"][:, 1:].copy()), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3).to(dev).eval()
    cams = [CameraState(sc["viewmats"][v].astype(np.float64), sc["Ks"][v].copy(), W, H) for v in range(frames)]
    renderer = FrameRenderer(model)

    def data_of(cs):   # the reference's two synchronous uploads
        return {"w2c": torch.tensor(cs.w2c, dtype=torch.float32, device=dev), "K": torch.tensor(cs.K, dtype=torch.float32, device=dev),
                "height": cs.height, "width": cs.width}

    res = {"workload": f"{n} Gaussians SH3, {W}x{H}, {frames} cameras on an orbit; device times by events, host times by perf_counter, medians",
           "height": H, "width": W, "gaussians": n, "frames": frames}
    with torch.no_grad():
        for cs in cams[:6]:   # warm-up: every path below, the workspace leases, the pinned rings
            renderer.render(cs)
            renderer.render(cs, fmt="uint8")
            renderer.render(cs, mode="depth", fmt="uint8")
            model(data_of(cs))["render_img"].cpu().numpy()
        list(renderer.render_path(cams[:4]))
        # ---- device time of the parts
        datas = [data_of(cs) for cs in cams]
        k = [0]

        def render_one():
            k[0] = (k[0] + 1) % frames
            return model(datas[k[0]], clamp=False)

        res["render_ms"] = round(device_ms(render_one, 24), 4)
        out = model(datas[0], clamp=False, depth="ED", alphas=True)
        img, depth, alpha = out["render_img"].contiguous(), out["render_depth"], out["render_alpha"]
        pH, pW = aspect_size(H, W, 2.0)
        bufs = {"u8": torch.empty((H, W, 3), dtype=torch.uint8, device=dev), "f32": torch.empty((H, W, 3), dtype=torch.float32, device=dev),
                "f32_padded": torch.empty((pH, pW, 3), dtype=torch.float32, device=dev)}
        rng = frame_depth_range(depth, alpha)
        res["finish_u8_us"] = round(1e3 * device_ms(lambda: finish_frame(img, fmt="uint8", out=bufs["u8"]), 15, inner=20), 2)
        res["finish_f32_us"] = round(1e3 * device_ms(lambda: finish_frame(img, fmt="float32", out=bufs["f32"]), 15, inner=20), 2)
        res["finish_f32_padded_us"] = round(1e3 * device_ms(lambda: finish_frame(img, fmt="float32", pad_to=(pH, pW), out=bufs["f32_padded"]), 15, inner=20), 2)
        res["finish_depth_u8_us"] = round(1e3 * device_ms(lambda: finish_frame(depth, mode="depth", fmt="uint8", alphas=alpha, depth_range=rng, out=bufs["u8"]), 15, inner=20), 2)
        res["range_us"] = round(1e3 * device_ms(lambda: frame_depth_range(depth, alpha, out=rng), 15, inner=20), 2)
        res["clamp01_us"] = round(1e3 * device_ms(lambda: torch.clamp(img, 0.0, 1.0), 15, inner=20), 2)   # (the parent's clamp, for scale)
        for name in ("u8", "f32"):
            host = torch.empty(bufs[name].shape, dtype=bufs[name].dtype).pin_memory()
            res[f"copy_{name}_ms"] = round(device_ms(lambda: host.copy_(bufs[name], non_blocking=True), 15, inner=4), 4)
        res["frame_bytes"] = {"u8": H * W * 3, "f32": H * W * 12}
        # ---- host latency of one displayed frame
        j = [0]

        def cam():
            j[0] = (j[0] + 1) % frames
            return cams[j[0]]

        res["render_call_f32_ms"] = round(wall_ms(lambda: renderer.render(cam()), 30), 4)
        res["render_call_u8_ms"] = round(wall_ms(lambda: renderer.render(cam(), fmt="uint8"), 30), 4)
        res["render_call_f32_aspect2_ms"] = round(wall_ms(lambda: renderer.render(cam(), aspect=2.0), 30), 4)
        res["render_call_depth_u8_ms"] = round(wall_ms(lambda: renderer.render(cam(), mode="depth", fmt="uint8"), 30), 4)

        def parent(pad=False, quantise=False):
            image = model(data_of(cam()))["render_img"].cpu().numpy()
            if pad:
                padded = np.zeros((pH, pW, 3), dtype=np.float32)
                padded[:H, :W] = image
                image = padded
            if quantise:
                image = np.floor(image * 255.0).astype(np.uint8)
            return image

        res["parent_f32_ms"] = round(wall_ms(parent, 30), 4)
        res["parent_f32_aspect2_ms"] = round(wall_ms(lambda: parent(pad=True), 30), 4)
        res["parent_u8_ms"] = round(wall_ms(lambda: parent(quantise=True), 30), 4)
        # ---- a camera path, twice each, alternating
        fps = {"path_fps_u8": [], "path_fps_f32": [], "parent_video_fps": []}
        for _ in range(2):
            for key, fmt in (("path_fps_u8", "uint8"), ("path_fps_f32", "float32")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                count = sum(1 for _ in renderer.render_path(cams, fmt=fmt))
                fps[key].append(count / (time.perf_counter() - t0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                parent(quantise=True)
            fps["parent_video_fps"].append(frames / (time.perf_counter() - t0))
        for key, v in fps.items():
            res[key] = [round(x, 2) for x in v]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
