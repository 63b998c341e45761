"""Checkpoint layout and camera export of the reference:

    <output>/checkpoints/iterations_<N>.pth      torch.save of the whole GaussianModel module (optimizer detached
                                                 unless save_optimizer=True)        /root/reference/utils.py:78-87
    <output>/cameras.json                        list of Frame.to_json dicts        /root/reference/scene/scene.py:91-94

`load_gaussian_model(path, iterations=None)` picks the requested or the latest `iterations_*.pth`
(/root/reference/utils.py:48-75).  The reference pickles the module by class reference
(`model.gaussian.GaussianModel`, with a `model.utils.LR_Scheduler` inside); this package's GaussianModel carries the
same attribute names, so files written here under those class paths unpickle in the reference, and files written by
the reference unpickle here -- `reference_class_paths()` installs / removes the two alias modules around the
(un)pickling, nothing of the reference is imported.
"""
from __future__ import annotations

import contextlib
import json
import sys
import types
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

from . import model as _model


@contextlib.contextmanager
def reference_class_paths():
    """Temporarily exposes this package's GaussianModel / LR_Scheduler as `model.gaussian.GaussianModel` and
    `model.utils.LR_Scheduler`, the paths the reference's pickles name (/root/reference/model/gaussian.py:14,
    model/utils.py:19)."""
    names = ("model", "model.gaussian", "model.utils")
    saved = {n: sys.modules.get(n) for n in names}
    pkg = types.ModuleType("model")
    pkg.__path__ = []   # a package
    gaussian = types.ModuleType("model.gaussian")
    utils = types.ModuleType("model.utils")
    gaussian.GaussianModel = _model.GaussianModel
    utils.LR_Scheduler = _model.LR_Scheduler
    pkg.gaussian, pkg.utils = gaussian, utils
    old_names = (_model.GaussianModel.__module__, _model.LR_Scheduler.__module__)
    sys.modules.update({"model": pkg, "model.gaussian": gaussian, "model.utils": utils})
    _model.GaussianModel.__module__, _model.LR_Scheduler.__module__ = "model.gaussian", "model.utils"
    try:
        yield
    finally:
        _model.GaussianModel.__module__, _model.LR_Scheduler.__module__ = old_names
        for n in names:
            if saved[n] is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = saved[n]


def as_torch_adam(optimizer) -> torch.optim.Adam:
    """A `torch.optim.Adam` over the same parameter objects with the same groups, step count and moments (copies) --
    what the reference's pickles hold (/root/reference/model/gaussian.py:389-412).  `optim.FusedAdam.state_dict()` is
    already in Adam's layout, so this is a plain load."""
    if isinstance(optimizer, torch.optim.Adam):
        return optimizer
    groups = [{"params": list(g["params"]), "lr": g["lr"], "name": g.get("name")} for g in optimizer.param_groups]
    adam = torch.optim.Adam(groups, betas=tuple(optimizer.defaults["betas"]), eps=optimizer.defaults["eps"])
    adam.load_state_dict(optimizer.state_dict())
    return adam


def as_fused_adam(optimizer):
    """The reverse: an `optim.FusedAdam` over the parameters of a `torch.optim.Adam` (they become views of its flat
    buffer, wherever they live now), moments and step count restored."""
    from .optim import FusedAdam
    groups = [{"params": list(g["params"]), "lr": g["lr"], "name": g.get("name")} for g in optimizer.param_groups]
    state = optimizer.state_dict()
    fused = FusedAdam(groups, betas=tuple(optimizer.defaults["betas"]), eps=optimizer.defaults["eps"])
    fused.load_state_dict(state)
    return fused


def save_gaussian_model(path: Path, gaussian_model: torch.nn.Module, save_optimizer: bool = False,
                        reference_compatible: bool = True):
    """`torch.save(gaussian_model, path)` with the optimizer detached unless asked for (reference behaviour,
    /root/reference/utils.py:78-87).  With `reference_compatible` the file names the reference's class paths and holds
    only what the reference's classes know: `MAX_SCALE_RATIO` as a tensor (the reference calls
    `torch.max(ratio, self.MAX_SCALE_RATIO)`, model/gaussian.py:380-382) and, with `save_optimizer`, a
    `torch.optim.Adam` carrying this optimizer's state (an `optim.FusedAdam` object would name a class the reference
    cannot import)."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    live_optimizer = gaussian_model.optimizer
    live_ratio = gaussian_model.__dict__.get("MAX_SCALE_RATIO")
    try:
        if not save_optimizer:
            gaussian_model.optimizer = None   # type: ignore
        elif reference_compatible and live_optimizer is not None:
            gaussian_model.optimizer = as_torch_adam(live_optimizer)
        if reference_compatible and live_ratio is not None and not isinstance(live_ratio, torch.Tensor):
            gaussian_model.MAX_SCALE_RATIO = torch.tensor(float(live_ratio), dtype=torch.float32, device=gaussian_model.means.device)
        with (reference_class_paths() if reference_compatible else contextlib.nullcontext()):
            torch.save(gaussian_model, path)
    finally:
        gaussian_model.optimizer = live_optimizer
        if live_ratio is not None:
            gaussian_model.MAX_SCALE_RATIO = live_ratio


def find_checkpoint(path: Path, iterations: Optional[int] = None) -> Path:
    cpt_lst = list((Path(path) / "checkpoints").glob("*.pth"))
    if iterations is not None:
        for cpt in cpt_lst:
            if cpt.stem == f"iterations_{iterations}":
                return cpt
        raise ValueError(f"cannot find checkpoint for iteration {iterations}")
    best, best_it = None, 0
    for cpt in cpt_lst:
        it = int(cpt.stem.split("_")[1])
        if it > best_it:
            best, best_it = cpt, it
    if best is None:
        raise ValueError("no checkpoint found")
    return best


def load_gaussian_model(path: Path, iterations: Optional[int] = None, device: Optional[str] = None,
                        optimizer: str = "keep") -> torch.nn.Module:
    """The reference loads to the CPU and then calls `.cuda()` (/root/reference/utils.py:48-75); `device=None` does that
    when a GPU is present.  Works on files written here and on files written by the reference (whose objects lack this
    package's extra attributes: they fall back to the class defaults of `model.GaussianModel`; their statistics and
    `MAX_SCALE_RATIO` are plain tensor attributes that `Module.to` does not move).
    A pickled optimizer (`save_optimizer=True`) is made steppable on `device`: `optimizer="keep"` leaves a
    `torch.optim.Adam` an Adam (state moved to the device), `"hip"` turns it into `optim.FusedAdam`; an
    `optim.FusedAdam` object found in an older file of this package is always rebuilt over the moved parameters."""
    if optimizer not in ("keep", "hip"):
        raise ValueError("optimizer: 'keep' or 'hip'")
    target = find_checkpoint(path, iterations)
    with reference_class_paths():
        gaussian_model = torch.load(target, map_location="cpu", weights_only=False)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    opt = gaussian_model.__dict__.get("optimizer")
    opt_state = None if opt is None else opt.state_dict()   # (before .to(): FusedAdam reads its flat CPU buffers here)
    gaussian_model = gaussian_model.to(device)
    for name in ("grad_norm_accum", "collecting_counts", "max_radii"):   # plain attributes in the reference's pickles
        t = gaussian_model.__dict__.get(name)
        if isinstance(t, torch.Tensor):
            gaussian_model.__dict__[name] = t.to(device)
    # MAX_SCALE_RATIO is a 0-d tensor in files the reference wrote (or `reference_compatible=True` here): a Python float from
    # now on -- read ONCE, on the CPU copy -- so that get_regularization_dict() never costs a device-to-host sync per
    # training step; save_gaussian_model(reference_compatible=True) re-tensorises it at save time
    ratio = gaussian_model.__dict__.get("MAX_SCALE_RATIO")
    if isinstance(ratio, torch.Tensor):
        gaussian_model.__dict__["MAX_SCALE_RATIO"] = float(ratio.detach().cpu())
    if opt is not None:
        from .optim import FusedAdam
        groups = [{"params": list(g["params"]), "lr": g["lr"], "name": g.get("name")} for g in opt.param_groups]
        betas, eps = tuple(opt.defaults["betas"]), opt.defaults["eps"]
        want_fused = optimizer == "hip" or isinstance(opt, FusedAdam)
        if want_fused and torch.device(device).type != "cuda":
            want_fused = False   # (FusedAdam steps on the GPU only; on the CPU the state stays a torch.optim.Adam)
        new = FusedAdam(groups, betas=betas, eps=eps) if want_fused else torch.optim.Adam(groups, betas=betas, eps=eps)
        new.load_state_dict(opt_state)   # (torch casts the moments to each parameter's device)
        gaussian_model.optimizer = new
    return gaussian_model


class CameraState:
    """What the reference's viewer / eval code gets from cameras.json (/root/reference/utils.py:28-46): w2c [4,4],
    K [3,3] (principal point at the image centre), width, height."""

    def __init__(self, w2c: np.ndarray, K: np.ndarray, width: int, height: int):
        self.w2c, self.K, self.width, self.height = w2c, K, width, height


def load_camera_states(path: Path) -> List[CameraState]:
    camera_states = []
    with open(Path(path) / "cameras.json", "r") as f:
        for cam in json.load(f):
            c2w = np.eye(4)
            c2w[:3, :3] = np.array(cam["rotation"])
            c2w[:3, 3] = np.array(cam["position"])
            K = np.array([[cam["fx"], 0, cam["width"] / 2], [0, cam["fy"], cam["height"] / 2], [0, 0, 1]], dtype=np.float32)
            camera_states.append(CameraState(np.linalg.inv(c2w), K, cam["width"], cam["height"]))
    return camera_states


# ---- the INRIA point_cloud.ply ----

_PLY_REST_COUNTS = {0: 0, 9: 1, 24: 2, 45: 3, 72: 4}   # f_rest properties -> SH degree: 3 ((deg + 1)^2 - 1)


def ply_properties(sh_degree: int) -> List[str]:
    """The property names of the INRIA layout, in file order: x y z nx ny nz f_dc_0..2 f_rest_0..3(K-1)-1 opacity scale_0..2 rot_0..3
    (K = (sh_degree + 1)^2), every one a little-endian float."""
    n_rest = 3 * ((sh_degree + 1) ** 2 - 1)
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(n_rest)] + ["opacity"]
            + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def save_ply(gaussian_model: torch.nn.Module, path) -> None:
    """The model as an INRIA `point_cloud.ply`: binary_little_endian, all properties float.  The values are the stored parameters,
    bit for bit: the normals zeros, `f_rest` channel-major (`sh_rest.transpose(1, 2).reshape(N, -1)`), `opacity` the logit,
    `scale_*` the logs, `rot_*` wxyz as stored, not normalised."""
    m = gaussian_model
    n, degree = int(m.means.shape[0]), int(m.MAX_SH_DEGREE)
    names = ply_properties(degree)
    cpu = lambda t: t.detach().float().cpu()   # noqa: E731
    cols = torch.cat([cpu(m.means).reshape(n, 3), torch.zeros((n, 3)), cpu(m.sh_0).reshape(n, 3),
                      cpu(m.sh_rest).transpose(1, 2).reshape(n, -1), cpu(m.logit_opacities).reshape(n, 1), cpu(m.log_scales).reshape(n, 3),
                      cpu(m.quats).reshape(n, 4)], dim=1).numpy()
    if cols.shape[1] != len(names):
        raise ValueError(f"sh_rest has {m.sh_rest.shape[1]} coefficients, SH degree {degree} has {(degree + 1) ** 2 - 1}")
    body = np.empty((n,), dtype=[(name, "<f4") for name in names])
    for i, name in enumerate(names):
        body[name] = cols[:, i]
    header = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property float {name}" for name in names]
                       + ["end_header"]) + "\n"
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(body.tobytes())


def load_ply(path, sh_degree: Optional[int] = None, device: Optional[str] = None, **model_kwargs) -> torch.nn.Module:
    """A `GaussianModel` from an INRIA `point_cloud.ply` (what `save_ply` writes; what the INRIA code and gsplat's exporters write).
    The SH degree is taken from the number of `f_rest_*` properties (0, 9, 24, 45, 72: degrees 0-4); a `sh_degree` given must agree.
    All SH bands are active.  `device=None`: the HIP device when there is one.  `model_kwargs` go to the constructor.
    ValueError: an ASCII or big-endian body, a property that is not a float, a property set that is not the INRIA one."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' ... 'end_header')")
    lines = [ln.strip() for ln in raw[:end].decode("ascii", "replace").splitlines()]
    lines = [ln for ln in lines[1:] if ln and not ln.startswith(("comment", "obj_info"))]
    if not lines or lines[0].split() != ["format", "binary_little_endian", "1.0"]:
        raise ValueError(f"{path}: only 'format binary_little_endian 1.0' is read, got {lines[0] if lines else 'no format line'!r}")
    n, names, in_vertex = None, [], False
    for ln in lines[1:]:
        w = ln.split()
        if w[0] == "element":
            if len(w) != 3 or (w[1] != "vertex" and int(w[2]) != 0) or (w[1] == "vertex" and n is not None):
                raise ValueError(f"{path}: one 'element vertex N' is read, got {ln!r}")
            in_vertex = w[1] == "vertex"
            if in_vertex:
                n = int(w[2])
        elif w[0] == "property" and in_vertex:
            if len(w) != 3 or w[1] not in ("float", "float32"):
                raise ValueError(f"{path}: every property must be a float, got {ln!r}")
            names.append(w[2])
        elif w[0] != "property":
            raise ValueError(f"{path}: unexpected header line {ln!r}")
    if n is None:
        raise ValueError(f"{path}: no 'element vertex'")
    n_rest = sum(nm.startswith("f_rest_") for nm in names)
    if n_rest not in _PLY_REST_COUNTS:
        raise ValueError(f"{path}: {n_rest} f_rest properties belong to no SH degree (0, 9, 24, 45, 72 give degrees 0-4)")
    degree = _PLY_REST_COUNTS[n_rest]
    if sh_degree is not None and sh_degree != degree:
        raise ValueError(f"{path}: the file holds SH degree {degree}, sh_degree = {sh_degree} was asked for")
    want = ply_properties(degree)
    if sorted(names) != sorted(want):
        odd = sorted(set(names) ^ set(want))
        raise ValueError(f"{path}: not the INRIA property set of SH degree {degree}: {odd[:6]} missing, unknown or repeated")
    start = end + len(b"end_header\n")
    if len(raw) - start < 4 * len(names) * n:
        raise ValueError(f"{path}: the body holds {len(raw) - start} bytes, {n} vertices of {len(names)} floats need {4 * len(names) * n}")
    body = np.frombuffer(raw, dtype=[(nm, "<f4") for nm in names], count=n, offset=start)   # (any property ORDER is read by name)

    def take(cols):
        return torch.from_numpy(np.stack([body[c] for c in cols], axis=1).astype(np.float32)) if n else torch.zeros((0, len(cols)))
    coeffs = (degree + 1) ** 2 - 1
    model = _model.GaussianModel(
        means=take(["x", "y", "z"]), log_scales=take([f"scale_{i}" for i in range(3)]), quats=take([f"rot_{i}" for i in range(4)]),
        sh_0=take([f"f_dc_{i}" for i in range(3)]).reshape(n, 1, 3),
        sh_rest=(take([f"f_rest_{i}" for i in range(n_rest)]).reshape(n, 3, coeffs).transpose(1, 2).contiguous() if coeffs
                 else torch.zeros((n, 0, 3))),
        logit_opacities=take(["opacity"]).reshape(n), sh_degree=degree, **model_kwargs)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    return model.to(device)
