"""float64 torch reference of the pose correction (csrc/gs_pose.h): `pose.CameraDeltas`' own formula -- torch.linalg.matrix_exp of
the skew matrix -- and autograd through it.  Shared by tests/test_pose_host.py and tests/test_gpu_pose_step.py."""
import math

import numpy as np
import torch

from easy_gaussian_splatting_amd.pose import CameraDeltas

THETAS = (0.0, 1e-9, 1e-4, 0.3, math.pi - 0.01)


def compose64(delta, w2c) -> torch.Tensor:
    """[[exp([omega]x), tau], [0, 1]] @ w2c in float64 through CameraDeltas.forward itself (one view)."""
    cd = CameraDeltas(1).double()
    with torch.no_grad():
        cd.deltas.copy_(torch.as_tensor(np.asarray(delta, dtype=np.float64)).reshape(1, 6))
    with torch.no_grad():
        return cd(torch.as_tensor(np.asarray(w2c, dtype=np.float64)).reshape(4, 4), 0)


def vjp64(delta, w2c, G, g=None) -> np.ndarray:
    """d/d delta of L = <G, V(delta)[0:3]> + <g, inv(V(delta))[:3,3]> by float64 autograd; G [3,4], g [3] (None: no centre term)."""
    cd = CameraDeltas(1).double()
    with torch.no_grad():
        cd.deltas.copy_(torch.as_tensor(np.asarray(delta, dtype=np.float64)).reshape(1, 6))
    V = cd(torch.as_tensor(np.asarray(w2c, dtype=np.float64)).reshape(4, 4), 0)
    L = (torch.as_tensor(np.asarray(G, dtype=np.float64)).reshape(3, 4) * V[:3]).sum()
    if g is not None:
        L = L + (torch.as_tensor(np.asarray(g, dtype=np.float64)) * torch.linalg.inv(V)[:3, 3]).sum()
    L.backward()
    return cd.deltas.grad[0].numpy().copy()


def random_rigid(rng) -> np.ndarray:
    """A random rigid world-to-camera matrix (float64): rotation from a QR factorisation, det +1, translation of a few units."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3] = q
    m[:3, 3] = rng.uniform(-3.0, 3.0, 3)
    return m


def delta_at(rng, theta) -> np.ndarray:
    """A 6-vector whose rotation part has norm `theta` about a random axis; translation of a few tenths."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    return np.concatenate([theta * axis, rng.uniform(-0.3, 0.3, 3)])
