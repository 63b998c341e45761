"""`FusedAdam.step(visible=...)` and `TrainStepGraph(visible_adam=True)`, host side: what they refuse, before the library is loaded and
before any device work -- and the scenes of tests/test_gpu_visible_step.py against the fp64 projection of the oracle.  No GPU."""
import numpy as np
import pytest
import torch

import visible_scene as VS
from easy_gaussian_splatting_amd.optim import FusedAdam
from oracle import torch_oracle as TO

NAMES = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")


def _opt(n=5, K=4):
    shapes = [(n, 3), (n, 3), (n, 4), (n, 1, 3), (n, K - 1, 3), (n,)]
    ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    return ps, FusedAdam([{"params": [p], "lr": 1e-3, "name": NAMES[i]} for i, p in enumerate(ps)])


@pytest.fixture()
def no_library(monkeypatch):
    """Every refusal stands in front of `_native.lib()`: loading the library is an error here."""
    from easy_gaussian_splatting_amd import _native

    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "lib", refuse)


def test_step_refuses_a_bad_visible_argument(no_library):
    ps, opt = _opt()
    radii = torch.ones(5, dtype=torch.int32)
    for bad, err in ((radii.float(), ValueError), (radii.long(), ValueError), (torch.ones(4, dtype=torch.int32), ValueError),
                     (torch.ones(6, dtype=torch.bool), ValueError), (torch.ones((2, 5), dtype=torch.bool), ValueError),
                     (torch.ones((1, 2, 5), dtype=torch.int32), ValueError), (radii.to("meta"), ValueError),
                     ([1, 1, 1, 1, 1], TypeError), (radii.numpy(), TypeError)):
        with pytest.raises(err, match="visible"):
            opt.step(visible=bad)
    stats = tuple(torch.zeros(5) for _ in range(4))
    with pytest.raises(ValueError, match="gs_adam_step_stats"):
        opt.step(visible=radii, stats=stats)
    assert opt._step == 0   # (a refused step does not count)
    # a parameter that does not hold one row per Gaussian
    ps2 = [torch.nn.Parameter(torch.zeros(s)) for s in ((5, 3), (7,))]
    opt2 = FusedAdam([{"params": [p], "lr": 1e-3, "name": n} for p, n in zip(ps2, ("means", "table"))])
    with pytest.raises(ValueError, match="'table'"):
        opt2.step(visible=radii)
    # what is accepted reaches the library: int32 [N], int32 [C, N], bool [N]
    for good in (radii, torch.ones((2, 5), dtype=torch.int32), torch.ones(5, dtype=torch.bool)):
        with pytest.raises(AssertionError, match="the library was loaded"):
            opt.step(visible=good)


def test_visible_rows_reduce_over_the_cameras():
    ps, opt = _opt()
    r2 = torch.tensor([[0, 3, 0, 0, -1], [0, 0, 2, 0, 0]], dtype=torch.int32)
    rows, widths = opt._visible_rows(r2, None)
    assert rows.dtype == torch.int32 and rows.tolist() == [0, 3, 2, 0, 0] and widths == [3, 3, 4, 3, 9, 1]
    rows, _ = opt._visible_rows(torch.tensor([True, False, True, False, False]), None)
    assert rows.dtype == torch.int32 and rows.tolist() == [1, 0, 1, 0, 0]
    _, opt0 = _opt(K=1)   # SH degree 0: an empty sh_rest is a segment of width 0
    assert opt0._visible_rows(torch.ones(5, dtype=torch.int32), None)[1] == [3, 3, 4, 3, 0, 1]


def _model(mode="classic"):
    from easy_gaussian_splatting_amd import model as M
    m = M.GaussianModel(means=torch.zeros((4, 3)), log_scales=torch.zeros((4, 3)), quats=torch.ones((4, 4)), sh_0=torch.zeros((4, 1, 3)),
                        sh_rest=torch.zeros((4, 3, 3)), logit_opacities=torch.zeros(4), sh_degree=1, white_background=True)
    if mode != "classic":
        m.rasterize_mode = mode
    return m


def test_train_step_graph_refuses_what_has_no_selective_kernel(no_library):
    from easy_gaussian_splatting_amd.depth_loss import DepthSupervision
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph, ViewParallelGraphStep, _refuse_combinations
    data = {"w2c": torch.eye(4), "K": torch.eye(3), "width": 32, "height": 32}
    gt = torch.zeros((32, 32, 3))
    stub = object()   # (every refusal comes before the runner looks at its optimizer or loss)
    for kw, variant in ((dict(mcmc=stub), "project_bwd_budget_kernel"), (dict(poses=stub), "SUMS = true"),
                        (dict(depth=DepthSupervision(0.1, "depth"), gt_depth=torch.ones(32, 32)), "project_bwd_depth_kernel")):
        with pytest.raises(ValueError, match="visible_adam=True.*gs_project_bwd_selective.*" + variant):
            TrainStepGraph(_model(), stub, stub, data, gt, visible_adam=True, **kw)
    for cam in ("ortho", "fisheye"):
        with pytest.raises(ValueError, match=f"visible_adam=True.*camera_model='{cam}'.*project_bwd_cm_kernel"):
            TrainStepGraph(_model(), stub, stub, dict(data, camera_model=cam), gt, camera_model=cam, visible_adam=True)
    for explicit in ({}, dict(rasterize_mode="antialiased")):
        with pytest.raises(ValueError, match="visible_adam=True.*antialiased.*project_bwd_aa_kernel"):
            TrainStepGraph(_model("antialiased"), stub, stub, data, gt, visible_adam=True, **explicit)
    with pytest.raises(ValueError, match="visible_adam.*adam_step_visible_kernel"):
        ViewParallelGraphStep(_model(), stub, stub, data, gt, vp=stub, visible_adam=True)
    # the existing callers of the helper keep their seven arguments, and the keyword is the constructor's last
    assert _refuse_combinations(_model(), "pinhole", None, None, None, None, "auto") == "classic"
    assert _refuse_combinations(_model(), "pinhole", None, None, None, None, "on", True) == "classic"
    import inspect
    assert list(inspect.signature(TrainStepGraph.__init__).parameters)[-1] == "visible_adam"
    assert inspect.signature(TrainStepGraph.__init__).parameters["visible_adam"].default is False


@pytest.mark.parametrize("N", VS.SIZES)
@pytest.mark.parametrize("case", VS.CASES)
def test_the_scenes_cull_what_they_say(case, N):
    """The preconditions tests/test_gpu_visible_step.py asserts on the step's radii, from the oracle's fp64 projection."""
    sc, behind, both = VS.scene(case, N, 0)
    f64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    radii = TO.project(f64(sc["means"]), f64(sc["quats"]), f64(sc["scales"]), f64(sc["viewmats"]), f64(sc["Ks"]), VS.W, VS.H, 0.3, 0.01, 1e10,
                       0.0)[0].numpy()
    seen0, seen1 = radii[0] > 0, radii[1] > 0
    assert np.array_equal(seen0, ~behind), (case, N)
    assert np.array_equal(seen1, ~both), (case, N)
    if case == "third":
        assert 0.2 <= seen0.mean() <= 0.8
    elif case == "block":
        assert not seen0[256:512].any() and seen0[:256].all() and seen0[512:].all()
    else:
        assert seen0.all()
    if behind.sum() >= 2:   # ("block" at N = 257: the second block is the one Gaussian 256)
        assert both.any() and (behind & ~both).any()   # the second view changes the culled set and leaves some culled
