"""Per-view bilateral grids (gsplat's `use_bilateral_grid`, from *Bilateral Guided Radiance Field Processing*): one learnable
low-resolution 3-D grid of 3x4 colour affines per training image, sliced at each pixel's position and at the luminance of the
render's own colour and applied to the UN-clamped render in front of the loss -- local tone mapping, vignetting and an ISP whose
response depends on position and brightness then land in the view's grid instead of in floaters and view-dependent SH noise; a
total-variation term keeps the grids smooth.  The generalisation of `exposure.ExposureTable` (one global affine per view).  In the
eager loop: `grids(render, i)` between `model(data, clamp=False)` and `LossComputer(clamp_input=True)`, plus
`tv_weight * grids.tv_loss()`, through the HIP kernels of csrc/gs_bilagrid.hip on the device and as the plain torch `grid_sample`
expression anywhere else (the semantic reference).  In the captured step (`TrainStepGraph(..., bilagrid=BilateralGrids(n))`):
applied, differentiated, regularised and stepped on the device, with `BilagridAdamState` holding the optimizer state.  Held-out
views have no grid: evaluate on the raw render.  See INTEGRATION.md "Correcting per-view appearance with bilateral grids"."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .optim import DenseAdamState

LUMA = (0.299, 0.587, 0.114)


def _tv_scratch(L, dev):
    from . import _native as nat
    return torch.empty((nat.GS_BILAGRID_TV_DOUBLES,), dtype=torch.float64, device=dev)


class _BilagridApply(torch.autograd.Function):
    """HIP path (csrc/gs_bilagrid.hip): one streaming kernel forward; backward the slice's adjoint into the view's slab (fp64, fixed
    order, no atomics: reproducible bits) and dL/d out -> dL/d image in place, the part through the luminance included."""

    @staticmethod
    def forward(ctx, image: Tensor, grids: Tensor, index: int):
        from . import _native as nat
        L = nat.lib()
        H, W = image.shape[:2]
        n, _, gl, gy, gx = grids.shape
        out = torch.empty_like(image)
        with torch.cuda.device(image.device):
            st = torch.cuda.current_stream(image.device).cuda_stream
            nat.check(L.gs_bilagrid_apply(st, H, W, n, gx, gy, gl, None, int(index), grids.data_ptr(), image.data_ptr(), out.data_ptr()),
                      "gs_bilagrid_apply")
        ctx.save_for_backward(image, grids)
        ctx.index = int(index)
        return out

    @staticmethod
    def backward(ctx, v_out: Tensor):
        from . import _native as nat
        L = nat.lib()
        image, grids = ctx.saved_tensors
        H, W = image.shape[:2]
        n, _, gl, gy, gx = grids.shape
        dev = image.device
        v_image = v_out.to(torch.float32).contiguous().clone()   # (the kernel works in place; autograd's tensor is not ours to write)
        partials = torch.empty((int(L.gs_bilagrid_partials_doubles(H, W, gx, gy, gl)),), dtype=torch.float64, device=dev)
        v_grids = torch.zeros_like(grids)   # dense: the adjoint on the view's slab, exact zeros on every other
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_bilagrid_bwd(st, H, W, n, gx, gy, gl, None, ctx.index, grids.data_ptr(), image.data_ptr(), v_image.data_ptr(),
                                        partials.data_ptr(), v_grids[ctx.index].data_ptr()), "gs_bilagrid_bwd")
        return v_image, v_grids, None


class _BilagridTV(torch.autograd.Function):
    """tv(grids) through gs_bilagrid_tv: the value in fp64 in a fixed order; backward fl32(upstream * d tv / d grids), the captured
    step's own arithmetic at upstream = tv_weight."""

    @staticmethod
    def forward(ctx, grids: Tensor):
        from . import _native as nat
        L = nat.lib()
        n, _, gl, gy, gx = grids.shape
        dev = grids.device
        tv = torch.empty((1,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_bilagrid_tv(st, n, gx, gy, gl, grids.data_ptr(), 0.0, None, 0, None, None, tv.data_ptr(), None,
                                       _tv_scratch(L, dev).data_ptr()), "gs_bilagrid_tv")
        ctx.save_for_backward(grids)
        return tv[0]

    @staticmethod
    def backward(ctx, v_tv: Tensor):
        from . import _native as nat
        L = nat.lib()
        (grids,) = ctx.saved_tensors
        n, _, gl, gy, gx = grids.shape
        dev = grids.device
        v_grids = torch.empty_like(grids)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_bilagrid_tv(st, n, gx, gy, gl, grids.data_ptr(), float(v_tv), None, 0, None, None, None, v_grids.data_ptr(),
                                       _tv_scratch(L, dev).data_ptr()), "gs_bilagrid_tv")
        return v_grids


def slice_reference(grids: Tensor, image: Tensor, index: int) -> Tensor:
    """The semantic reference in plain torch: `grid_sample` of the view's slab at (pixel centre, pixel centre, luminance), the
    sampled 3x4 affine applied to the pixel.  Differentiable with respect to `grids` and `image` (through the luminance too)."""
    H, W = image.shape[:2]
    dt, dev = image.dtype, image.device
    g = grids[index:index + 1].to(dt)
    xs = (2.0 * (torch.arange(W, dtype=dt, device=dev) + 0.5) / W - 1.0).expand(H, W)
    ys = (2.0 * (torch.arange(H, dtype=dt, device=dev) + 0.5) / H - 1.0)[:, None].expand(H, W)
    luma = LUMA[0] * image[..., 0] + LUMA[1] * image[..., 1] + LUMA[2] * image[..., 2]
    xyz = torch.stack([xs, ys, 2.0 * luma - 1.0], dim=-1)[None, None]                    # [1, 1, H, W, 3]
    M = F.grid_sample(g, xyz, mode="bilinear", align_corners=True, padding_mode="border")   # [1, 12, 1, H, W]
    M = M[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (M[..., :3] @ image[..., None])[..., 0] + M[..., 3]


def tv_reference(grids: Tensor) -> Tensor:
    """(1 / n_views) * sum over the axes {L, Hg, Wg} of sum(forward difference^2) / (differences along the axis in one slab)."""
    n = grids.shape[0]
    total = grids.new_zeros(())
    for dim in (2, 3, 4):
        d = grids.narrow(dim, 1, grids.shape[dim] - 1) - grids.narrow(dim, 0, grids.shape[dim] - 1)
        total = total + d.pow(2).sum() / (d.numel() // n)
    return total / n


class BilateralGrids(nn.Module):
    """`grids[n_views, 12, grid_w, grid_y, grid_x]` float32: per training view a grid_x x grid_y x grid_w (luminance) grid of 3x4
    affines [A | b], channel k = 4 i + j entry (i, j), every node initialised to [I | 0]:

        forward(image[H, W, 3], index)[p] = M(p)[:, :3] @ image[p] + M(p)[:, 3]
        M(p) = the trilinear interpolation of grids[index] at ((x + 0.5) / W, (y + 0.5) / H, clamp(luma(image[p]), 0, 1))

    Input and output are the un-clamped image (`model(data, clamp=False)["render_img"]`); the clamp stays inside
    `LossComputer(clamp_input=True)`.  The gradient of `grids` is dense -- zeros on every other view -- which is what
    `torch.optim.Adam(grids.parameters())` expects (gsplat: lr 2e-3, eps 1e-15).  Add `10 * grids.tv_loss()` to the loss."""

    def __init__(self, n_views: int, grid_x: int = 16, grid_y: int = 16, grid_w: int = 8):
        super().__init__()
        n_views, grid_x, grid_y, grid_w = int(n_views), int(grid_x), int(grid_y), int(grid_w)
        if n_views < 1 or not (2 <= grid_x <= 64 and 2 <= grid_y <= 64 and 2 <= grid_w <= 16):
            raise ValueError(f"BilateralGrids: n_views >= 1, 2 <= grid_x, grid_y <= 64 and 2 <= grid_w <= 16 (got {n_views}, {grid_x}, {grid_y}, "
                             f"{grid_w})")
        if n_views * 12 * grid_w * grid_y * grid_x >= 2 ** 31:
            raise ValueError("BilateralGrids: n_views * 12 * grid_w * grid_y * grid_x must stay below 2^31")
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12)
        self.grids = nn.Parameter(eye[None, :, None, None, None].expand(n_views, 12, grid_w, grid_y, grid_x).contiguous())

    def _native(self, *tensors: Tensor) -> bool:
        g = self.grids
        return g.device.type == "cuda" and g.dtype == torch.float32 and g.is_contiguous() and all(
            t.device == g.device and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)

    def forward(self, image: Tensor, index: int) -> Tensor:
        g = self.grids
        i, n = int(index), int(g.shape[0])
        if not 0 <= i < n:
            raise IndexError(f"BilateralGrids: index {i} outside the {n} views")
        if image.dim() != 3 or image.shape[2] != 3 or image.numel() == 0:
            raise ValueError(f"BilateralGrids: an image [H, W, 3], got {tuple(image.shape)}")
        if self._native(image):
            return _BilagridApply.apply(image, g, i)
        return slice_reference(g, image, i)

    def tv_loss(self, fused: bool = False) -> Tensor:
        """The total variation of all views' grids.  `fused=True`: through gs_bilagrid_tv (the captured step's arithmetic, eager)."""
        if fused:
            if not self._native():
                raise ValueError("BilateralGrids.tv_loss(fused=True): contiguous float32 grids on a HIP device")
            return _BilagridTV.apply(self.grids)
        return tv_reference(self.grids)


class BilagridAdamState(DenseAdamState):
    """Adam's state for `BilateralGrids` stepped inside the captured train step (`TrainStepGraph(bilagrid=...)` makes one:
    `runner.bilagrid_state`): the two moments, shaped like `grids`, on its device and the number of steps taken -- dense Adam, every
    step counts for every view.  `state_dict()` / `load_state_dict()` let a checkpoint carry it next to `grids.state_dict()`."""

    def __init__(self, grids: BilateralGrids):
        super().__init__(grids.grids)
