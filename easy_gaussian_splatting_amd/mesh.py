"""A triangle mesh out of a trained model (csrc/gs_tsdf.hip; DESIGN.md 30, INTEGRATION.md "Extracting a mesh").

    vertices, faces, colors = mesh.extract_mesh(model, views, resolution=256)
    mesh.save_mesh_ply("scene_mesh.ply", vertices, faces, colors)

`TSDFVolume` is a dense truncated-signed-distance volume on the device.  `integrate` folds one pinhole view in -- the `[H,W,4]` buffer
`rasterization(render_mode="RGB+ED")` returns is read in place, the depth being one of its channels -- and `extract` runs marching
tetrahedra over the six-tetrahedron Kuhn split of every cell: a watertight, consistently oriented surface wherever all eight
corners of a cell were observed.  `fuse_model` renders and integrates a list of views, `extract_mesh` does all of it.  Every value
is the function csrc/gs_tsdf.h states, bit for bit; no atomics, so the same input gives the same mesh.  GPU only: there is no CPU
fallback.  Pinhole cameras only: a fisheye depth is not a z-depth along straight columns."""
from __future__ import annotations

import ctypes as ct
import math
import threading
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _native as nat

_tls = threading.local()


def _dims3(dims) -> Tuple[int, int, int]:
    d = tuple(int(v) for v in dims)
    if len(d) != 3:
        raise ValueError(f"dims must be (nx, ny, nz), got {dims!r}")
    return d


def check_dims(dims) -> None:
    """Raises ValueError unless every dimension is >= 2 and 7 * nx * ny * nz < 2^31 -- the C entry's own argument check
    (`gs_mt_scan_workspace_ints` returns 0 for a refused volume); nothing is allocated."""
    d = _dims3(dims)
    if any(not -2**31 <= v < 2**31 for v in d) or int(nat.lib().gs_mt_scan_workspace_ints((ct.c_int32 * 3)(*d))) == 0:
        raise ValueError(f"TSDFVolume: dims {d} refused: every dimension must be >= 2 and 7 * nx * ny * nz < 2^31")


class TSDFVolume:
    """A dense TSDF volume: `dims = (nx, ny, nz)` samples at `origin + i * voxel_size` per axis.  `.tsdf` (fresh: 1), `.weight`
    (fresh: 0) and -- `color=True` -- `.color` (fresh: 0) are plain float32 tensors shaped [nz, ny, nx(, 3)] on `device`."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], trunc: Optional[float] = None, color: bool = True,
                 device=None):
        self.dims = _dims3(dims)
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        if len(self.origin) != 3 or not all(math.isfinite(v) for v in self.origin):
            raise ValueError(f"origin must be three finite numbers, got {origin!r}")
        if not (self.voxel_size > 0 and math.isfinite(self.voxel_size)):
            raise ValueError(f"voxel_size must be positive and finite, got {voxel_size!r}")
        if not (self.trunc > 0 and math.isfinite(self.trunc)):
            raise ValueError(f"trunc must be positive and finite, got {trunc!r}")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else \
            torch.device("cpu" if device is None else device)
        if dev.type != "cuda":
            raise NotImplementedError("TSDFVolume lives on the GPU only (csrc/gs_tsdf.hip); there is no CPU fallback")
        check_dims(self.dims)
        self.device = dev
        nx, ny, nz = self.dims
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        self.color = torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=dev) if color else None

    @classmethod
    def from_bounds(cls, lo: Sequence[float], hi: Sequence[float], resolution: int, **kwargs) -> "TSDFVolume":
        """The volume over the box [lo, hi] whose longest side has `resolution` samples; the other sides as many as cover them."""
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3 or not all(b > a for a, b in zip(lo, hi)) or not all(math.isfinite(v) for v in lo + hi):
            raise ValueError(f"from_bounds: lo < hi per axis, three finite numbers each (got {lo}, {hi})")
        if int(resolution) < 2:
            raise ValueError(f"resolution must be >= 2, got {resolution!r}")
        h = max(b - a for a, b in zip(lo, hi)) / (int(resolution) - 1)
        dims = [max(2, int(math.ceil((b - a) / h - 1e-6)) + 1) for a, b in zip(lo, hi)]
        return cls(lo, h, dims, **kwargs)

    @property
    def bounds(self) -> Tuple[Tuple[float, float, float], Tuple[float, float, float]]:
        return self.origin, tuple(o + (n - 1) * self.voxel_size for o, n in zip(self.origin, self.dims))

    def _c_grid(self):
        return (ct.c_int32 * 3)(*self.dims), (ct.c_float * 3)(*self.origin)

    def _on_device(self, t, what: str, shape=None) -> Tensor:
        if not isinstance(t, Tensor):
            raise ValueError(f"{what} must be a tensor, got {type(t).__name__}")
        if t.device.type != "cuda":
            raise NotImplementedError(f"{what} is on {t.device}: TSDFVolume runs on the GPU only, there is no CPU fallback")
        if t.device != self.device:
            raise ValueError(f"{what} is on {t.device}, the volume on {self.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} must be float32, got {t.dtype}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
        return t

    @torch.no_grad()
    def integrate(self, image: Tensor, viewmat: Tensor, K: Tensor, *, depth_channel: int = -1,
                  color_channels: Optional[Sequence[int]] = (0, 1, 2), alphas: Optional[Tensor] = None, min_alpha: float = 0.5,
                  depth_max: float = math.inf, max_weight: float = math.inf) -> "TSDFVolume":
        """Folds one pinhole view in: one launch on the current stream, no host read.  `image` [H, W, D] float32 (read in place when
        contiguous), the z-depth in channel `depth_channel`, the colour in the three consecutive channels `color_channels` (None, or
        a volume without colour: depth only); `viewmat` [4, 4] world -> camera and `K` [3, 3] (no skew) are read on the device;
        `alphas` [H, W(, 1)]: pixels with alpha < min_alpha are holes, as are depths that are not finite, <= 0 or > depth_max."""
        self._on_device(image, "image")
        if image.dim() != 3:
            raise ValueError(f"image must be [H, W, D], got {list(image.shape)}")
        H, W, D = (int(v) for v in image.shape)
        viewmat = self._on_device(viewmat, "viewmat", (4, 4)).contiguous()
        K = self._on_device(K, "K", (3, 3)).contiguous()
        dch = int(depth_channel) + (D if int(depth_channel) < 0 else 0)
        if not 0 <= dch < D:
            raise ValueError(f"depth_channel {depth_channel} outside the image's {D} channels")
        cch = -1
        if self.color is not None and color_channels is not None:
            cc = [int(c) for c in color_channels]
            if len(cc) != 3 or cc[1] != cc[0] + 1 or cc[2] != cc[0] + 2 or not 0 <= cc[0] <= D - 3:
                raise ValueError(f"color_channels must be three consecutive channels of the image's {D}, got {color_channels!r}")
            cch = cc[0]
        elif self.color is not None:
            raise ValueError("this volume carries colour: give color_channels, or build it with color=False")
        if alphas is not None:
            self._on_device(alphas, "alphas")
            if tuple(alphas.shape) not in ((H, W), (H, W, 1)):
                raise ValueError(f"alphas must be [{H}, {W}] or [{H}, {W}, 1], got {list(alphas.shape)}")
            alphas = alphas.contiguous()
        image = image.contiguous()
        dims, origin = self._c_grid()
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(nat.lib().gs_tsdf_integrate(
                st, dims, origin, self.voxel_size, self.trunc, float(depth_max), float(min_alpha), float(max_weight), viewmat.data_ptr(),
                K.data_ptr(), W, H, image.data_ptr(), D, dch, cch, None if alphas is None else alphas.data_ptr(), self.tsdf.data_ptr(),
                self.weight.data_ptr(), None if cch < 0 else self.color.data_ptr()), "gs_tsdf_integrate")
        return self

    @torch.no_grad()
    def extract(self, min_weight: float = 1.0) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
        """-> (vertices float32 [V, 3], faces int32 [F, 3], colors float32 [V, 3] or None): marching tetrahedra over the cells all of
        whose corners have weight >= min_weight (> 0).  Vertices are numbered by (owner voxel, edge kind), faces ordered by (cell,
        tetrahedron, triangle) with (v1 - v0) x (v2 - v0) pointing from inside (tsdf < 0) to outside.  One host read -- the two
        totals, page-locked memory behind an event; an empty surface returns empty tensors and launches no emit kernel."""
        if not float(min_weight) > 0:
            raise ValueError(f"min_weight must be positive (a voxel no view reached has weight 0), got {min_weight!r}")
        L, dev = nat.lib(), self.device
        nx, ny, nz = self.dims
        n = nx * ny * nz
        dims, origin = self._c_grid()
        i32 = dict(dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            st = stream.cuda_stream
            edge_flags, edge_incl = torch.empty((7 * n,), **i32), torch.empty((7 * n,), **i32)
            tri_counts, tri_incl = torch.empty((n,), **i32), torch.empty((n,), **i32)
            scan_ws = torch.empty((int(L.gs_mt_scan_workspace_ints(dims)),), **i32)
            host = getattr(_tls, "totals", None)
            if host is None:   # (page-locked int64[2] per host thread: read before the call returns, so one is enough)
                host = _tls.totals = torch.zeros((2,), dtype=torch.int64, pin_memory=True)
            host.fill_(-1)
            nat.check(L.gs_mt_flags(st, dims, float(min_weight), self.tsdf.data_ptr(), self.weight.data_ptr(), edge_flags.data_ptr(),
                                    edge_incl.data_ptr(), tri_counts.data_ptr(), tri_incl.data_ptr(), scan_ws.data_ptr(), host.data_ptr()),
                      "gs_mt_flags")
            ev = torch.cuda.Event()
            ev.record(stream)
            ev.synchronize()
            nv, nf = (int(v) for v in host.tolist())
            if not (0 <= nv <= 7 * n and 0 <= nf <= 12 * n):
                raise nat.NativeLibraryError(f"TSDFVolume.extract: the totals record holds {(nv, nf)} for {n} voxels")
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((nf, 3), **i32)
            colors = None if self.color is None else torch.empty((nv, 3), dtype=torch.float32, device=dev)
            if nv > 0:
                nat.check(L.gs_mt_vertices(st, dims, origin, self.voxel_size, self.tsdf.data_ptr(),
                                           None if self.color is None else self.color.data_ptr(), edge_flags.data_ptr(), edge_incl.data_ptr(),
                                           nv, vertices.data_ptr(), None if colors is None else colors.data_ptr()), "gs_mt_vertices")
            if nf > 0:
                nat.check(L.gs_mt_faces(st, dims, self.tsdf.data_ptr(), tri_counts.data_ptr(), tri_incl.data_ptr(), edge_incl.data_ptr(), nv, nf,
                                        faces.data_ptr()), "gs_mt_faces")
        return vertices, faces, colors


def _pinhole(data: Dict[str, Any], what: str) -> None:
    cm = data.get("camera_model", "pinhole")
    if cm != "pinhole":
        raise NotImplementedError(f"{what}: camera_model {cm!r} is not supported -- TSDF fusion projects voxels through a pinhole, and "
                                  "a fisheye or orthographic depth is not a z-depth along its columns")


@torch.no_grad()
def fuse_model(model, views: Iterable[Dict[str, Any]], volume: TSDFVolume, *, depth: str = "ED", min_alpha: float = 0.5,
               depth_max: float = math.inf) -> TSDFVolume:
    """Renders every data dict of `views` (what `GaussianModel.forward` takes: w2c, K, width, height) with `render_mode="RGB+" +
    depth` -- the model's parameters and activations as `GaussianModel.forward` passes them -- and integrates the returned 4-channel
    buffer and its alphas into `volume` directly: no copy, no host read."""
    from .rendering import rasterization
    if depth not in ("D", "ED"):
        raise ValueError(f"depth: 'D' or 'ED', got {depth!r}")
    if model.means.device.type != "cuda":
        raise NotImplementedError("fuse_model runs on the GPU only; there is no CPU fallback")
    raw = getattr(model, "fuse_activations", True)
    rmode = getattr(model, "rasterize_mode", "classic")
    for data in views:
        _pinhole(data, "fuse_model")
        img, alphas, _ = rasterization(
            means=model.means, quats=model.quats, scales=model.log_scales if raw else model.scales,
            opacities=model.logit_opacities if raw else model.opacities,
            colors=(model.sh_0, model.sh_rest) if getattr(model, "fuse_sh_cat", True) else model.shs, sh_degree=model.active_sh_degree,
            viewmats=data["w2c"][None], Ks=data["K"][None], width=data["width"], height=data["height"],
            backgrounds=model.BACKGROUND[None], packed=False, render_mode="RGB+" + depth,
            _tile_culling=getattr(model, "tile_culling", "tight"), _activations="exp_sigmoid" if raw else "none",
            **({} if rmode == "classic" else {"rasterize_mode": rmode}))
        volume.integrate(img[0], data["w2c"], data["K"], depth_channel=3, color_channels=(0, 1, 2) if volume.color is not None else None,
                         alphas=alphas[0], min_alpha=min_alpha, depth_max=depth_max)
    return volume


@torch.no_grad()
def extract_mesh(model, views: Iterable[Dict[str, Any]], *, bounds=None, resolution: int = 256, trunc: Optional[float] = None,
                 color: bool = True, depth: str = "ED", min_alpha: float = 0.5, depth_max: float = math.inf, min_weight: float = 1.0):
    """-> (vertices, faces, colors) of `model` seen from `views`.  `bounds = (lo, hi)`; default: the box between the 1st and the 99th
    percentile of `model.means` per axis, grown by the truncation distance.  `resolution`: samples along the longest side."""
    if model.means.device.type != "cuda":
        raise NotImplementedError("extract_mesh runs on the GPU only; there is no CPU fallback")
    views = list(views)
    for data in views:
        _pinhole(data, "extract_mesh")
    if bounds is None:
        m = model.means.detach().float()
        k_lo, k_hi = max(1, int(math.ceil(0.01 * m.shape[0]))), max(1, int(math.ceil(0.99 * m.shape[0])))
        lo = [float(m[:, a].kthvalue(k_lo).values) for a in range(3)]
        hi = [float(m[:, a].kthvalue(k_hi).values) for a in range(3)]
        h = max(b - a for a, b in zip(lo, hi)) / max(1, int(resolution) - 1)
        grow = 4.0 * h if trunc is None else float(trunc)
        lo, hi = [v - grow for v in lo], [v + grow for v in hi]
    else:
        lo, hi = bounds
    volume = TSDFVolume.from_bounds(lo, hi, resolution, trunc=trunc, color=color, device=model.means.device)
    fuse_model(model, views, volume, depth=depth, min_alpha=min_alpha, depth_max=depth_max)
    return volume.extract(min_weight=min_weight)


# ---- binary little-endian PLY ----

def _ply_header(nv: int, nf: int, colors: bool) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {nv}", "property float x", "property float y", "property float z"]
    if colors:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += [f"element face {nf}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _to_host(t: Tensor) -> Tensor:
    """a contiguous CPU copy; a device tensor comes through a page-locked buffer in one copy"""
    t = t.detach().contiguous()
    if t.device.type == "cpu":
        return t
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host


def save_mesh_ply(path, vertices: Tensor, faces: Tensor, colors: Optional[Tensor] = None) -> None:
    """Binary little-endian PLY: `vertex x y z [red green blue uchar]` and `face vertex_indices list uchar int`.  Colours are clamped
    to [0, 1] and rounded to uint8 where they live; each array crosses to the host once."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"vertices [V, 3] and faces [F, 3] expected, got {list(vertices.shape)} and {list(faces.shape)}")
    if colors is not None and tuple(colors.shape) != tuple(vertices.shape):
        raise ValueError(f"colors must be {list(vertices.shape)}, got {list(colors.shape)}")
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    v = vertices.detach().to(torch.float32)
    if colors is None:
        rows = _to_host(v.contiguous().view(torch.uint8).reshape(nv, 12))
    else:
        c8 = (colors.detach().to(torch.float32).clamp(0.0, 1.0) * 255.0 + 0.5).floor().to(torch.uint8)
        rows = _to_host(torch.cat([v.contiguous().view(torch.uint8).reshape(nv, 12), c8], dim=1))
    f = faces.detach().to(torch.int32).contiguous()
    frows = torch.cat([torch.full((nf, 1), 3, dtype=torch.uint8, device=f.device), f.view(torch.uint8).reshape(nf, 12)], dim=1)
    frows = _to_host(frows)
    with open(path, "wb") as fh:
        fh.write(_ply_header(nv, nf, colors is not None))
        fh.write(rows.numpy().tobytes())
        fh.write(frows.numpy().tobytes())


def load_mesh_ply(path) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """-> (vertices float32 [V, 3], faces int32 [F, 3], colors float32 [V, 3] in [0, 1] or None) of a file `save_mesh_ply` wrote."""
    import numpy as np
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[1].strip() != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only binary little-endian PLY is read, got `{lines[1]}`")
    nv = nf = None
    props: Dict[str, list] = {}
    cur = None
    for ln in lines[2:]:
        w = ln.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "element":
            cur = w[1]
            props[cur] = []
            if cur == "vertex":
                nv = int(w[2])
            elif cur == "face":
                nf = int(w[2])
        elif w[0] == "property" and cur is not None:
            props[cur].append(" ".join(w[1:]))
    xyz, rgb = ["float x", "float y", "float z"], ["uchar red", "uchar green", "uchar blue"]
    if nv is None or nf is None or props.get("vertex") not in (xyz, xyz + rgb) or props.get("face") != ["list uchar int vertex_indices"]:
        raise ValueError(f"{path}: not the layout save_mesh_ply writes ({props})")
    has_color = props["vertex"] == xyz + rgb
    stride = 15 if has_color else 12
    body = np.frombuffer(blob, np.uint8, offset=end + len(b"end_header\n"))
    if body.size != nv * stride + nf * 13:
        raise ValueError(f"{path}: {body.size} bytes of data for {nv} vertices and {nf} faces")
    vrows = body[:nv * stride].reshape(nv, stride)
    vertices = torch.from_numpy(np.ascontiguousarray(vrows[:, :12]).view("<f4").reshape(nv, 3).copy())
    colors = torch.from_numpy(vrows[:, 12:].astype(np.float32) / 255.0) if has_color else None
    frows = body[nv * stride:].reshape(nf, 13)
    if nf and not (frows[:, 0] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    faces = torch.from_numpy(np.ascontiguousarray(frows[:, 1:]).view("<i4").reshape(nf, 3).copy())
    return vertices, faces, colors
