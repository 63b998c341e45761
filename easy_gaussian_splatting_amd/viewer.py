"""What the reference's viewer calls and what its `RecordManager` does (the reference's launch_viewer.py, viewer/utils.py,
viewer/viewer_runtime.py), without the UI: viser, the per-client threads and the GUI callbacks stay the reference's
(SURVEY.md row 17).

    finish_frame          a render -> a displayable frame: clamp, aspect padding, uint8 quantisation or a depth grey, ONE pass
                          (csrc/gs_frame.hip: `gs_frame_finish`, `gs_frame_range`)
    FrameRenderer         the viewer's `render_func`: camera upload from pinned memory, `model(data)`, `gs_frame_finish`, one
                          asynchronous copy into a ring of page-locked host buffers; `render_path` pipelines a camera path
    camera_interpolation  key cameras -> a camera path (viewer/utils.py:70-101): distance-proportional frame counts, constant
                          screw motion between two keys; SE(3) log / exp in float64 numpy
    export_video          `RecordManager.export_video` (viewer/utils.py:118-135): interpolate, render, hand the frames to a writer
    viewer_render_func    `Viewer(viewer_render_func(model), camera_states, ...)`

Per displayed frame the reference uploads two matrices synchronously, clamps, reads the float32 image back through pageable
memory (24.9 MB at 1080p), pads it on the host for the client's aspect and, for a video, quantises it on the host.  Here the
frame is finished on the device and what crosses the bus is the finished frame: a quarter of the bytes for a video.
"""
from __future__ import annotations

import threading
from datetime import datetime
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .checkpoint import CameraState

_WORKSPACES: Dict[Any, Tensor] = {}   # (device, stream) -> gs_frame_range's partial pairs + the {lo, hi} it leaves; grows
_FORMATS = {"float32": torch.float32, "uint8": torch.uint8}
_MODES = ("rgb", "depth")


def _workspace(dev: torch.device, stream: int, floats: int) -> Tensor:
    key = (dev, stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < floats:
        ws = _WORKSPACES[key] = torch.empty((floats,), dtype=torch.float32, device=dev)
    return ws


# ---------------------------------------------------------------------------------------------------------------------------
# finish_frame

def _clamp01_keep_nan(x: Tensor) -> Tensor:
    """clamp(x, 0, 1) as `gs_frame_finish` states it: a NaN stays a NaN, -0 becomes +0."""
    return torch.where(x > 0, torch.clamp(x, max=1.0), torch.where(torch.isnan(x), x, torch.zeros_like(x)))


def _torch_range(depth: Tensor, alphas: Tensor, alpha_min: float) -> Tensor:
    covered = (alphas >= alpha_min) & ~torch.isnan(depth)
    if not bool(covered.any()):
        return torch.zeros(2, dtype=depth.dtype, device=depth.device)
    d = depth[covered]
    return torch.stack([d.min(), d.max()])


def _torch_finish(render: Tensor, mode: str, fmt: str, out_hw: Tuple[int, int], alphas: Optional[Tensor],
                  depth_range: Optional[Tensor], alpha_min: float) -> Tensor:
    """`gs_frame_finish` (and `gs_frame_range`) in plain torch, on any device."""
    H, W = int(render.shape[0]), int(render.shape[1])
    if mode == "rgb":
        x = render[..., :3].to(torch.float32)
    else:
        d = render[..., -1].to(torch.float32)
        a = alphas.reshape(H, W).to(torch.float32)
        rng = _torch_range(d, a, alpha_min) if depth_range is None else depth_range.to(torch.float32)
        lo, hi = rng[0], rng[1]
        t = torch.where(hi == lo, torch.zeros_like(d), (d - lo) / (hi - lo))
        g = torch.where(a >= alpha_min, 1.0 - _clamp01_keep_nan(t), torch.zeros_like(d))
        x = g.unsqueeze(2).expand(H, W, 3)
    c = _clamp01_keep_nan(x)
    if fmt == "uint8":
        c = torch.floor(torch.where(torch.isnan(c), torch.zeros_like(c), c) * 255.0).to(torch.uint8)
    if out_hw == (H, W):
        return c.contiguous()
    frame = torch.zeros((out_hw[0], out_hw[1], 3), dtype=c.dtype, device=c.device)
    frame[:H, :W] = c
    return frame


def _depth_source(render: Tensor) -> Tuple[Tensor, int, int]:
    """-> (tensor to keep alive, pointer, cin) for a depth frame's source.  `[H, W, 4]` contiguous: itself.  `[H, W, 1]`: itself
    when contiguous; when it is channel 3 of a contiguous four-channel image -- `model(data, depth=...)["render_depth"]` is such a
    view -- the kernel walks it in place with cin = 4 (it reads that channel only), which saves the 4 H W byte copy."""
    H, W, C = (int(s) for s in render.shape)
    if C == 1 and not render.is_contiguous() and tuple(render.stride()) == (4 * W, 4, 1) and render.storage_offset() >= 3:
        ptr = render.data_ptr() - 12
        if ptr % 16 == 0:
            return render, ptr, 4
    r = render.contiguous()
    if r.data_ptr() % 16:
        r = r.clone()
    return r, r.data_ptr(), C


def _aligned(t: Tensor) -> Tensor:
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


@torch.no_grad()
def finish_frame(render: Tensor, *, mode: str = "rgb", fmt: str = "uint8", pad_to: Optional[Tuple[int, int]] = None,
                 alphas: Optional[Tensor] = None, depth_range: Union[None, Tensor, Sequence[float]] = None, alpha_min: float = 0.5,
                 out: Optional[Tensor] = None) -> Tensor:
    """A render -> a frame `[out_H, out_W, 3]`, `fmt` "uint8" (packed RGB, `floor(clamp(x, 0, 1) * 255)`: one rounded float32
    product, then floor; a NaN gives 0) or "float32" (`clamp(x, 0, 1)`; a NaN stays a NaN).

    `render`: the UN-clamped image `[H, W, C]`.  `mode="rgb"`: channels 0-2 of C = 3 or 4.  `mode="depth"`: the last channel of
    C = 4 (`render_mode="RGB+D"` / `"RGB+ED"`) or a depth image `[H, W, 1]`, with `alphas` `[H, W]` or `[H, W, 1]`: a pixel whose
    alpha is below `alpha_min` is 0, every other is the grey `1 - clamp((d - lo) / (hi - lo), 0, 1)` on all three channels (near
    is bright; 1 where `hi == lo`).  `depth_range`: `{lo, hi}` as a `[2]` tensor on `render`'s device or a pair of numbers;
    None: the min and max of the covered depths (`gs_frame_range`: NaN depths skipped, {0, 0} when nothing is covered).
    `pad_to=(out_H, out_W)`, neither smaller than the render: the image sits top-left and everything else is zero (the
    reference's `adjust_image_aspect`).  `out`: where to write, a contiguous tensor of that shape and dtype on `render`'s device.

    Float32 tensors on the GPU go through `gs_frame_finish`: one launch that writes every element of the frame (nothing clears
    `out` first), no allocation beyond the frame and a cached workspace, nothing read back.  Anything else is the same
    arithmetic in plain torch."""
    if mode not in _MODES:
        raise ValueError(f"mode: 'rgb' or 'depth', got {mode!r}")
    if fmt not in _FORMATS:
        raise ValueError(f"fmt: 'uint8' or 'float32', got {fmt!r}")
    if render.dim() != 3:
        raise ValueError(f"render must be [H, W, C], got {tuple(render.shape)}")
    H, W, C = (int(s) for s in render.shape)
    if H <= 0 or W <= 0:
        raise ValueError(f"render must not be empty, got {tuple(render.shape)}")
    if C not in ((3, 4) if mode == "rgb" else (1, 4)):
        raise ValueError(f"mode={mode!r} takes a render with {'3 or 4' if mode == 'rgb' else '1 or 4'} channels, got {C}")
    out_hw = (H, W) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
    if out_hw[0] < H or out_hw[1] < W:
        raise ValueError(f"pad_to={out_hw} is smaller than the render ({H}, {W})")
    dev = render.device
    if mode == "depth":
        if alphas is None:
            raise ValueError("mode='depth' needs alphas")
        if alphas.numel() != H * W or tuple(alphas.shape[:2]) != (H, W):
            raise ValueError(f"alphas has shape {tuple(alphas.shape)}, expected ({H}, {W}) or ({H}, {W}, 1)")
        if alphas.device != dev:
            raise ValueError(f"alphas is on {alphas.device}, render on {dev}")
        if depth_range is not None:
            if isinstance(depth_range, Tensor):
                if depth_range.numel() != 2 or depth_range.device != dev:
                    raise ValueError(f"depth_range must be a [2] tensor on {dev}")
                depth_range = depth_range.reshape(2)
            else:
                lo, hi = depth_range
                depth_range = torch.tensor([float(lo), float(hi)], dtype=torch.float32, device=dev)
    shape = (out_hw[0], out_hw[1], 3)
    if out is not None and (tuple(out.shape) != shape or out.dtype != _FORMATS[fmt] or out.device != dev or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {fmt} tensor of shape {shape} on {dev}")
    if not (dev.type == "cuda" and render.dtype == torch.float32):
        frame = _torch_finish(render, mode, fmt, out_hw, alphas, depth_range, alpha_min)
        if out is None:
            return frame
        out.copy_(frame)
        return out
    from . import _native as nat
    L = nat.lib()
    if out is None:
        out = torch.empty(shape, dtype=_FORMATS[fmt], device=dev)
    elif out.data_ptr() % 16:
        raise ValueError("out must be 16-byte aligned")
    st = torch.cuda.current_stream(dev).cuda_stream
    code = nat.GS_FRAME_U8 if fmt == "uint8" else nat.GS_FRAME_F32
    with torch.cuda.device(dev):
        if mode == "rgb":
            r = _aligned(render)
            nat.check(L.gs_frame_finish(st, H, W, C, r.data_ptr(), nat.GS_FRAME_RGB, code, None, None, float(alpha_min),
                                        out_hw[0], out_hw[1], out.data_ptr()), "gs_frame_finish")
            return out
        keep, ptr, cin = _depth_source(render)
        a = alphas if alphas.dtype == torch.float32 else alphas.to(torch.float32)
        a = _aligned(a)
        if depth_range is None:
            n = int(L.gs_frame_workspace_floats(H, W))
            ws = _workspace(dev, st, n + 2)
            depth_range = ws[n:n + 2]
            nat.check(L.gs_frame_range(st, H, W, cin, ptr, a.data_ptr(), float(alpha_min), ws.data_ptr(), depth_range.data_ptr()),
                      "gs_frame_range")
        else:
            depth_range = depth_range.to(torch.float32).contiguous()
        nat.check(L.gs_frame_finish(st, H, W, cin, ptr, nat.GS_FRAME_DEPTH, code, a.data_ptr(), depth_range.data_ptr(),
                                    float(alpha_min), out_hw[0], out_hw[1], out.data_ptr()), "gs_frame_finish")
        del keep
    return out


@torch.no_grad()
def frame_depth_range(render: Tensor, alphas: Tensor, alpha_min: float = 0.5, out: Optional[Tensor] = None) -> Tensor:
    """-> `[2]` = {lo, hi}: the min and max of `render`'s last channel (C = 1 or 4) over the pixels with `alphas >= alpha_min`,
    NaN depths skipped, {0, 0} when nothing is covered -- what `finish_frame(mode="depth", depth_range=None)` scales by; keep it
    to give a whole camera path one grey scale.  `gs_frame_range` for float32 tensors on the GPU, plain torch otherwise."""
    if render.dim() != 3 or int(render.shape[2]) not in (1, 4):
        raise ValueError(f"render must be [H, W, 1] or [H, W, 4], got {tuple(render.shape)}")
    H, W = int(render.shape[0]), int(render.shape[1])
    if alphas.numel() != H * W or alphas.device != render.device:
        raise ValueError(f"alphas must hold ({H}, {W}) values on {render.device}")
    dev = render.device
    if not (dev.type == "cuda" and render.dtype == torch.float32):
        rng = _torch_range(render[..., -1].to(torch.float32), alphas.reshape(H, W).to(torch.float32), alpha_min)
        if out is None:
            return rng
        out.copy_(rng)
        return out
    from . import _native as nat
    L = nat.lib()
    if out is None:
        out = torch.empty((2,), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (2,) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [2] tensor on {dev}")
    st = torch.cuda.current_stream(dev).cuda_stream
    keep, ptr, cin = _depth_source(render)
    a = _aligned(alphas if alphas.dtype == torch.float32 else alphas.to(torch.float32))
    ws = _workspace(dev, st, int(L.gs_frame_workspace_floats(H, W)) + 2)
    with torch.cuda.device(dev):
        nat.check(L.gs_frame_range(st, H, W, cin, ptr, a.data_ptr(), float(alpha_min), ws.data_ptr(), out.data_ptr()), "gs_frame_range")
    del keep
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# FrameRenderer

def aspect_size(height: int, width: int, aspect: Optional[float]) -> Tuple[int, int]:
    """The padded size the reference's `adjust_image_aspect` gives an `height x width` image for a client of that aspect
    (viewer/viewer_runtime.py:104-116): a narrower image grows to `int(h * aspect)` columns, a wider one to `int(w / aspect)`
    rows."""
    if aspect is None:
        return height, width
    if width / height < aspect:
        return height, int(height * aspect)
    if width / height > aspect:
        return int(width / aspect), width
    return height, width


class _Slot:
    """One frame in flight: the camera's pinned staging row and its device copy, the finished frame on the device, its
    page-locked host buffer and the event of the copy between the two."""

    def __init__(self, dev: torch.device):
        self.cam_host = torch.empty((32,), dtype=torch.float32).pin_memory()
        self.cam_dev = torch.empty((32,), dtype=torch.float32, device=dev)
        self.frame_dev: Optional[Tensor] = None
        self.frame_host: Optional[Tensor] = None
        self.finished = torch.cuda.Event()
        self.copied = torch.cuda.Event()
        self.copy_pending = False

    def buffers(self, shape: Tuple[int, int, int], dtype: torch.dtype, dev: torch.device) -> None:
        """(re)allocates on a change of size or format; a returned array keeps its old buffer alive"""
        if self.frame_dev is None or tuple(self.frame_dev.shape) != shape or self.frame_dev.dtype != dtype:
            self.frame_dev = torch.empty(shape, dtype=dtype, device=dev)
            self.frame_host = torch.empty(shape, dtype=dtype).pin_memory()


class FrameRenderer:
    """The viewer's `render_func` (the reference's launch_viewer.py:29-37, train.py:172-183) for a `GaussianModel` on the GPU.

    `render(camera_state)` is callable from any host thread; calls are serialised by one lock, as the reference's `Viewer`
    serialises its clients (viewer/viewer.py:23-27).  Per call: the two camera matrices go through one pinned staging row and one
    non-blocking upload; `model(data, clamp=False)` runs under `no_grad`; `gs_frame_finish` clamps, pads for the client's aspect
    and quantises in one launch on the same stream; one non-blocking copy takes the finished frame into the next of `ring`
    page-locked host buffers, and the call waits on that copy's event alone.

    Streams.  The render and the finish run on the CALLING thread's current stream of the model's device, the copy on a side
    stream of the renderer's, ordered by events both ways.  Between two `TrainStepGraph.step()` calls a render is therefore
    ordered as an evaluation is: the next step waits for the caller's stream on entry; with `handback="lazy"`
    call `runner.fence()` first.  It takes none of the captured step's buffers and leaves the run bit-identical.

    A model in training mode is put into `eval()` for the call and back into `train()` after it.

    `camera_model` ("pinhole" | "ortho" | "fisheye"): what the model's forward receives as `data["camera_model"]` for every frame."""

    def __init__(self, model, ring: int = 3, device: Optional[Union[str, torch.device]] = None, camera_model: str = "pinhole") -> None:
        if camera_model not in ("pinhole", "ortho", "fisheye"):
            raise ValueError(f"camera_model: 'pinhole', 'ortho' or 'fisheye' (got {camera_model!r})")
        self.camera_model = camera_model
        if ring < 2:
            raise ValueError("ring must be at least 2: one buffer with the consumer, one being filled")
        if device is None:
            device = next(model.parameters()).device
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"FrameRenderer needs a model on the GPU (got {self.device}): there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.model = model
        self.ring = int(ring)
        self._lock = threading.Lock()
        self._slots = [_Slot(self.device) for _ in range(self.ring)]
        self._next = 0
        self._copy_stream = torch.cuda.Stream(self.device)

    # ---- one frame: enqueue (render, finish, copy) and wait
    def _enqueue(self, slot: _Slot, cs: CameraState, fmt: str, out_hw: Tuple[int, int], mode: str,
                 depth_range: Optional[Tensor]) -> None:
        """Everything of one frame up to the copy into `slot.frame_host`, enqueued; nothing waits for it here."""
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        if slot.copy_pending:   # the slot's last copy still reads frame_dev and cam_host may still be read by its upload
            slot.copied.synchronize()
            slot.copy_pending = False
        cam = slot.cam_host.numpy()
        cam[:16] = np.asarray(cs.w2c, dtype=np.float32).reshape(16)
        cam[16:25] = np.asarray(cs.K, dtype=np.float32).reshape(9)
        slot.cam_dev.copy_(slot.cam_host, non_blocking=True)
        H, W = int(cs.height), int(cs.width)
        data = {"w2c": slot.cam_dev[:16].view(4, 4), "K": slot.cam_dev[16:25].view(3, 3), "height": H, "width": W}
        if self.camera_model != "pinhole":
            data["camera_model"] = self.camera_model
        slot.buffers((out_hw[0], out_hw[1], 3), _FORMATS[fmt], dev)
        if mode == "rgb":
            out = self.model(data, clamp=False)
            finish_frame(out["render_img"], mode="rgb", fmt=fmt, pad_to=out_hw, out=slot.frame_dev)
        else:
            out = self.model(data, clamp=False, depth="ED", alphas=True)
            finish_frame(out["render_depth"], mode="depth", fmt=fmt, pad_to=out_hw, alphas=out["render_alpha"],
                         depth_range=depth_range, out=slot.frame_dev)
        slot.finished.record(stream)
        self._copy_stream.wait_event(slot.finished)
        with torch.cuda.stream(self._copy_stream):
            slot.frame_host.copy_(slot.frame_dev, non_blocking=True)
        slot.copied.record(self._copy_stream)
        slot.copy_pending = True
        # (frame_dev is written again only by this slot's next frame, which waits for `copied` on the host above)

    @staticmethod
    def _wait(slot: _Slot) -> np.ndarray:
        slot.copied.synchronize()
        slot.copy_pending = False
        return slot.frame_host.numpy()

    def _check(self, fmt: str, mode: str) -> None:
        if fmt not in _FORMATS:
            raise ValueError(f"fmt: 'uint8' or 'float32', got {fmt!r}")
        if mode not in _MODES:
            raise ValueError(f"mode: 'rgb' or 'depth', got {mode!r}")

    @torch.no_grad()
    def render(self, camera_state: CameraState, *, fmt: str = "float32", aspect: Optional[float] = None, mode: str = "rgb",
               depth_range: Optional[Tensor] = None, copy: bool = False) -> np.ndarray:
        """-> the frame of `camera_state` as a numpy array `[out_H, out_W, 3]`.  The defaults give what the reference's
        `gs_render_func` gives, bit for bit: float32 `[H, W, 3]` in [0, 1].  `fmt="uint8"`: `floor(that * 255)` as bytes, formed
        on the device (a quarter of the bytes read back).  `aspect`: the client's, for which the reference's
        `adjust_image_aspect` pads the image on the host (`aspect_size`); here the padding is part of the finishing launch.
        `mode="depth"`: the expected depth (`render_mode="RGB+ED"`) as a grey, near bright, 0 where the accumulated opacity is
        below 0.5; scaled by the frame's own range or by `depth_range` (a `[2]` device tensor, `frame_depth_range`).

        The returned array IS one of the renderer's `ring` page-locked buffers: it stays valid until `ring - 1` further frames
        have been produced by this renderer.  `copy=True` returns a private array instead."""
        self._check(fmt, mode)
        with self._lock:
            was_training = bool(getattr(self.model, "training", False))
            if was_training:
                self.model.eval()
            try:
                with torch.cuda.device(self.device):
                    slot = self._slots[self._next]
                    self._next = (self._next + 1) % self.ring
                    out_hw = aspect_size(int(camera_state.height), int(camera_state.width), aspect)
                    self._enqueue(slot, camera_state, fmt, out_hw, mode, depth_range)
                    frame = self._wait(slot)
                    return frame.copy() if copy else frame
            finally:
                if was_training:
                    self.model.train()

    @torch.no_grad()
    def render_path(self, camera_states: Iterable[CameraState], *, fmt: str = "uint8", mode: str = "rgb",
                    depth_range: Optional[Tensor] = None) -> Iterator[np.ndarray]:
        """A generator over the frames of a camera path.  Frame i + 1 -- render, finish and the copy behind them on the side
        stream -- is enqueued before the host waits for frame i's copy, so the device works while the consumer (an encoder)
        holds frame i.  The path has a ring of its own, apart from `render()`'s; the renderer's lock is taken per frame, not
        across the path, so a viewer's `render()` calls interleave with an export.

        A yielded array is one of the path's `ring` page-locked buffers.  Its slot is handed to the device again only when the
        consumer has asked for the frame `ring - 1` places later: with `ring=2` a frame is valid until the next is asked for,
        with `ring=3` (the default) one frame longer.  Copy what has to live longer."""
        self._check(fmt, mode)
        slots = [_Slot(self.device) for _ in range(self.ring)]
        it = iter(camera_states)

        def enqueue(i: int, cs: CameraState) -> None:
            with self._lock:
                was_training = bool(getattr(self.model, "training", False))
                if was_training:
                    self.model.eval()
                try:
                    with torch.cuda.device(self.device):
                        self._enqueue(slots[i % self.ring], cs, fmt, (int(cs.height), int(cs.width)), mode, depth_range)
                finally:
                    if was_training:
                        self.model.train()

        try:
            cs = next(it, None)
            if cs is None:
                return
            enqueue(0, cs)
            i = 0
            while True:
                nxt = next(it, None)
                if nxt is not None:
                    enqueue(i + 1, nxt)   # slot (i + 1) % ring: frame i + 1 - ring, which the consumer let go by asking for frame i
                yield self._wait(slots[i % self.ring])
                if nxt is None:
                    return
                i += 1
        finally:
            for s in slots:   # a consumer that stops early: no copy may still be writing into memory about to be freed
                if s.copy_pending:
                    s.copied.synchronize()


def viewer_render_func(model, camera_model: str = "pinhole") -> Callable[[CameraState], np.ndarray]:
    """`Viewer(viewer_render_func(gaussian_model), camera_states, ...)`: the reference's `gs_render_func`."""
    return FrameRenderer(model, camera_model=camera_model).render


# ---------------------------------------------------------------------------------------------------------------------------
# camera paths: SE(3) log / exp in float64

SMALL_ANGLE = 0.25   # below it the coefficients with a cancelling numerator come from their series (truncation < 1e-15 there)


def _hat(w: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _so3_log(R: np.ndarray) -> np.ndarray:
    """Rotation vector of R through the unit quaternion (the largest of its four components first, so nothing small is
    divided by): theta = 2 atan2(|v|, w) is well conditioned at every angle -- near pi, where the antisymmetric part of R
    vanishes and acos of the trace loses half the digits, w is small and |v| is 1."""
    m00, m11, m22 = R[0, 0], R[1, 1], R[2, 2]
    cand = np.array([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22])
    k = int(np.argmax(cand))
    s = 2.0 * np.sqrt(max(cand[k], 0.0))   # 4 * the component
    if k == 0:
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif k == 1:
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif k == 2:
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    w, v = q[0], q[1:]
    n = np.linalg.norm(v)
    if n < 1e-8:   # theta / |v| = 2 atan(n / w) / n = 2 / w (1 - n^2 / (3 w^2) + ...): the second term is below 1e-16 here
        return v * (2.0 / w)
    return v * (2.0 * np.arctan2(n, w) / n)


def _coefficients(theta: float) -> Tuple[float, float, float, float]:
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3 (exp: R = I + A W + B W^2, V = I + B W + C W^2) and
    D = (1 - (t / 2) cot(t / 2)) / t^2 (log: V^-1 = I - W / 2 + D W^2).  C and D subtract nearly equal numbers for small t: below
    SMALL_ANGLE they are summed from their series (five terms: the sixth is below 1e-15), as is A at t = 0."""
    t2 = theta * theta
    if theta < SMALL_ANGLE:
        A = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0 * (1.0 - t2 / 110.0))))
        B = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0 * (1.0 - t2 / 90.0 * (1.0 - t2 / 132.0))))
        C = 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0 * (1.0 - t2 / 110.0 * (1.0 - t2 / 156.0))))
        D = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))))
        return A, B, C, D
    h = 0.5 * theta
    sh = np.sin(h)
    A = np.sin(theta) / theta
    B = 2.0 * sh * sh / t2
    C = (theta - np.sin(theta)) / (t2 * theta)
    D = (1.0 - h * np.cos(h) / sh) / t2
    return float(A), float(B), float(C), float(D)


def se3_log(T: np.ndarray) -> np.ndarray:
    """-> the twist `[u (3), omega (3)]` of a rigid transform `[4, 4]`, `se3_exp`'s inverse for rotations up to pi."""
    T = np.asarray(T, dtype=np.float64)
    w = _so3_log(T[:3, :3])
    theta = float(np.linalg.norm(w))
    W = _hat(w)
    _, _, _, D = _coefficients(theta)
    Vinv = np.eye(3) - 0.5 * W + D * (W @ W)
    return np.concatenate([Vinv @ T[:3, 3], w])


def se3_exp(xi: np.ndarray) -> np.ndarray:
    """-> the rigid transform `[4, 4]` of the twist `[u (3), omega (3)]`."""
    xi = np.asarray(xi, dtype=np.float64)
    u, w = xi[:3], xi[3:]
    theta = float(np.linalg.norm(w))
    W = _hat(w)
    W2 = W @ W
    A, B, C, _ = _coefficients(theta)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W2
    T[:3, 3] = (np.eye(3) + B * W + C * W2) @ u
    return T


def _rigid_inverse(T: np.ndarray) -> np.ndarray:
    T = np.asarray(T, dtype=np.float64)
    inv = np.eye(4)
    inv[:3, :3] = T[:3, :3].T
    inv[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return inv


def camera_interpolation(camera_states: List[CameraState], duration: float, fps: float) -> List[CameraState]:
    """Key cameras -> the cameras of a `duration`-second path at `fps` (the reference's viewer/utils.py:70-101).  The
    `int(duration * fps)` frames are shared among the segments in proportion to the distance between their keys' centres, each
    share truncated; a segment whose share is 0 contributes its end key alone.  Inside a segment the camera-to-world pose moves
    along the constant screw from the start key to the end key: `start @ exp(log(start^-1 @ end) * j / n)`, j = 1 .. n, so the
    last frame of a segment is its end key.  Frame 0 is the first key itself; every generated state carries the FIRST key's
    `K`, `width` and `height`, as the reference's do.  With fewer frames than keys the keys are returned as they are.
    (Keys that all share one centre have no distances to share by: the segments then get equal shares, where the reference
    divides by zero.)"""
    n = len(camera_states)
    total_frames = int(duration * fps)
    if total_frames < n:
        return camera_states
    c2ws = [_rigid_inverse(cs.w2c) for cs in camera_states]
    dist = np.array([np.linalg.norm(c2ws[i][:3, 3] - c2ws[i + 1][:3, 3]) for i in range(n - 1)])
    shares = dist / dist.sum() * total_frames if dist.sum() > 0 else np.full((n - 1,), total_frames / max(n - 1, 1))
    first = camera_states[0]

    def state(w2c: np.ndarray) -> CameraState:
        return CameraState(w2c, first.K.copy(), first.width, first.height)

    path: List[CameraState] = [first]
    for i in range(n - 1):
        frames = int(shares[i])
        if frames == 0:
            path.append(state(camera_states[i + 1].w2c))
            continue
        twist = se3_log(_rigid_inverse(c2ws[i]) @ c2ws[i + 1])
        for j in range(1, frames + 1):
            path.append(state(_rigid_inverse(c2ws[i] @ se3_exp(twist * j / frames))))
    return path


# ---------------------------------------------------------------------------------------------------------------------------
# video export

def write_ppm_frames(path: Path, frames: Iterable[np.ndarray], fps: float) -> Path:
    """The writer for a machine without imageio: binary PPM files `frame_%05d.ppm` in the directory `path` without its suffix,
    and a one-line `README.txt` with the ffmpeg command that makes the video of them.  -> the directory."""
    path = Path(path)
    directory = path.with_suffix("") if path.suffix else path
    directory.mkdir(parents=True, exist_ok=True)
    for i, frame in enumerate(frames):
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        with open(directory / f"frame_{i:05d}.ppm", "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (frame.shape[1], frame.shape[0]))
            f.write(frame.tobytes())
    (directory / "README.txt").write_text(f"ffmpeg -framerate {fps:g} -i frame_%05d.ppm -pix_fmt yuv420p {directory.name}.mp4\n")
    return directory


def _imageio_writer(path: Path, frames: Iterable[np.ndarray], fps: float) -> Path:
    import imageio
    with imageio.get_writer(path, fps=fps) as w:   # (frame by frame: mimsave would be handed a list)
        for frame in frames:
            w.append_data(frame)
    return path


def _default_writer() -> Callable[[Path, Iterable[np.ndarray], float], Optional[Path]]:
    try:
        import imageio  # noqa: F401
    except ImportError:
        return write_ppm_frames
    return _imageio_writer


def export_video(renderer_or_func: Union[FrameRenderer, Callable[[CameraState], np.ndarray]], camera_states: List[CameraState],
                 duration: float, fps: float, output_dir: Path,
                 writer: Optional[Callable[[Path, Iterable[np.ndarray], float], Optional[Path]]] = None) -> Optional[Path]:
    """The reference's `RecordManager.export_video` (viewer/utils.py:118-135): the key cameras become a path
    (`camera_interpolation`), every camera of it a uint8 frame, the frames a video `<output_dir>/<%m-%d_%H-%M-%S>.mp4`.
    One key camera or none is refused as the reference refuses it: a printed line, None returned.

    A `FrameRenderer` renders through `render_path` (uint8 formed on the device, frame i + 1 in flight while frame i is being
    encoded); any other callable is called per camera as the reference calls its `render_func`, `floor(image * 255)` on the host.
    The frames go to `writer(path, frames, fps)` as an ITERABLE that is consumed as the frames arrive -- the reference's list
    of all frames (6 MB each at 1080p) is never built; a frame is valid only until the writer asks for the next.  Default
    writer: imageio where it imports, else `write_ppm_frames`.  -> what the writer returns, or `path`."""
    if len(camera_states) <= 1:
        print(f"export_video: refused, a path needs at least two key cameras (got {len(camera_states)})")
        return None
    path_states = camera_interpolation(camera_states, duration, fps)
    if isinstance(renderer_or_func, FrameRenderer):
        frames: Iterable[np.ndarray] = renderer_or_func.render_path(path_states, fmt="uint8")
    else:
        frames = (np.floor(renderer_or_func(cs) * 255.0).astype(np.uint8) for cs in path_states)
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / (datetime.now().strftime(r"%m-%d_%H-%M-%S") + ".mp4")
    written = (writer or _default_writer())(path, frames, fps)
    result = Path(written) if written is not None else path
    print(f"export_video: {len(path_states)} frames written to {result}")
    return result
