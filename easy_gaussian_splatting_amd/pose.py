"""Per-view camera corrections for pose refinement.  In the eager loop: plain torch, no kernel -- the gradient of the corrected view
matrix comes from the rasterizer (`rasterization(_camera_grads=True)`, which `GaussianModel.forward` asks for whenever
`data["w2c"]` requires grad).  In the captured step (`TrainStepGraph(..., poses=CameraDeltas(n))`): composed, differentiated and
stepped on the device (csrc/gs_pose.h), with `PoseAdamState` holding the optimizer state.  See INTEGRATION.md "Refining camera
poses"."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .optim import DenseAdamState


class CameraDeltas(nn.Module):
    """One 6-vector per training view: axis-angle `omega` (3) and translation `tau` (3), zero-initialised, applied on the camera
    side of the world-to-camera matrix:

        forward(w2c, index) = [[exp([omega]x), tau], [0, 1]] @ w2c

    The rotation is `torch.linalg.matrix_exp` of the skew matrix: smooth at omega = 0, where training starts (a bare Rodrigues
    quotient sin|w| / |w| has no gradient there).  Optimise `deltas` with an optimizer of its own next to the model's."""

    def __init__(self, n_views: int):
        super().__init__()
        self.deltas = nn.Parameter(torch.zeros(int(n_views), 6))

    def forward(self, w2c: Tensor, index: int) -> Tensor:
        d = self.deltas[index]
        w, tau = d[:3], d[3:]
        zero = torch.zeros((), dtype=d.dtype, device=d.device)
        skew = torch.stack([torch.stack([zero, -w[2], w[1]]),
                            torch.stack([w[2], zero, -w[0]]),
                            torch.stack([-w[1], w[0], zero])])
        top = torch.cat([torch.linalg.matrix_exp(skew), tau[:, None]], dim=1)                 # [3,4]
        bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=d.dtype, device=d.device)
        return torch.cat([top, bottom], dim=0) @ w2c.to(d.dtype)


class PoseAdamState(DenseAdamState):
    """Adam's state for a `CameraDeltas` stepped inside the captured train step (`TrainStepGraph(poses=...)` makes one:
    `runner.pose_state`): the two moments [n_views, 6] on the deltas' device and the number of pose steps taken -- dense Adam, every
    step counts for every row.  `state_dict()` / `load_state_dict()` let a checkpoint carry it next to `poses.state_dict()`."""

    def __init__(self, poses: CameraDeltas):
        super().__init__(poses.deltas)
