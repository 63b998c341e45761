"""Per-view exposure compensation: one learnable 3x4 colour affine per training image, applied to the UN-clamped render in front of
the loss (3DGS's and gsplat's exposure optimisation) -- auto-exposure and white-balance drift from frame to frame then lands in
twelve numbers per view instead of in floaters and view-dependent SH noise.  In the eager loop: `table(render, i)` between
`model(data, clamp=False)` and `LossComputer(clamp_input=True)`, through the HIP kernels of csrc/gs_exposure.hip on the device and
as the plain torch expression anywhere else (the semantic reference).  In the captured step
(`TrainStepGraph(..., exposure=ExposureTable(n))`): applied, differentiated and stepped on the device, with `ExposureAdamState`
holding the optimizer state.  Held-out views have no row: evaluate on the raw render.  See INTEGRATION.md "Compensating per-view
exposure"."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .optim import DenseAdamState


class _ExposureApply(torch.autograd.Function):
    """HIP path (csrc/gs_exposure.hip): one streaming kernel forward; backward one more that turns dL/d out into dL/d image in place
    and leaves the 12 sums of the view's row (fp64, fixed order, no atomics: reproducible bits)."""

    @staticmethod
    def forward(ctx, image: Tensor, affine: Tensor, index: int):
        from . import _native as nat
        L = nat.lib()
        H, W = image.shape[:2]
        out = torch.empty_like(image)
        with torch.cuda.device(image.device):
            st = torch.cuda.current_stream(image.device).cuda_stream
            nat.check(L.gs_exposure_apply(st, H, W, affine.shape[0], None, int(index), affine.data_ptr(), image.data_ptr(), out.data_ptr()),
                      "gs_exposure_apply")
        ctx.save_for_backward(image, affine)
        ctx.index = int(index)
        return out

    @staticmethod
    def backward(ctx, v_out: Tensor):
        from . import _native as nat
        L = nat.lib()
        image, affine = ctx.saved_tensors
        H, W = image.shape[:2]
        dev = image.device
        v_image = v_out.to(torch.float32).contiguous().clone()   # (the kernel works in place; autograd's tensor is not ours to write)
        partials = torch.empty((int(L.gs_exposure_partials_doubles(H, W)),), dtype=torch.float64, device=dev)
        v_affine = torch.zeros_like(affine)   # dense: the 12 sums on the view's row, exact zeros on every other
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(L.gs_exposure_bwd(st, H, W, affine.shape[0], None, ctx.index, affine.data_ptr(), image.data_ptr(), v_image.data_ptr(),
                                        partials.data_ptr(), v_affine[ctx.index].data_ptr()), "gs_exposure_bwd")
        return v_image, v_affine, None


class ExposureTable(nn.Module):
    """`affine[n_views, 3, 4]` = [A | b] per training view, every row initialised to [I | 0]:

        forward(image[H, W, 3], index)[p] = A @ image[p] + b,   A = affine[index, :, :3],  b = affine[index, :, 3]

    Input and output are the un-clamped image (`model(data, clamp=False)["render_img"]`); the clamp stays inside
    `LossComputer(clamp_input=True)`.  The gradient of `affine` is dense -- zeros on every other row -- which is what
    `torch.optim.Adam(table.parameters())` expects.  Optimise it with an optimizer of its own next to the model's."""

    def __init__(self, n_views: int):
        super().__init__()
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
        self.affine = nn.Parameter(eye.expand(int(n_views), 3, 4).contiguous())

    def forward(self, image: Tensor, index: int) -> Tensor:
        a = self.affine
        i, n = int(index), int(a.shape[0])
        if not 0 <= i < n:
            raise IndexError(f"ExposureTable: index {i} outside the {n} views")
        if (image.device.type == "cuda" and a.device == image.device and image.dtype == torch.float32 and a.dtype == torch.float32
                and image.dim() == 3 and image.shape[2] == 3 and image.numel() > 0 and image.is_contiguous() and a.is_contiguous()):
            return _ExposureApply.apply(image, a, i)
        return image @ a[i, :, :3].to(image.dtype).T + a[i, :, 3].to(image.dtype)


class ExposureAdamState(DenseAdamState):
    """Adam's state for an `ExposureTable` stepped inside the captured train step (`TrainStepGraph(exposure=...)` makes one:
    `runner.exposure_state`): the two moments [n_views, 3, 4] on the table's device and the number of exposure steps taken -- dense
    Adam, every step counts for every row.  `state_dict()` / `load_state_dict()` let a checkpoint carry it next to
    `table.state_dict()`."""

    def __init__(self, table: ExposureTable):
        super().__init__(table.affine)
