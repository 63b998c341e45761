"""The training blend forward blends the same pairs with the same instructions as the inference walk; its bookkeeping (quadrant
sublists, work units and their checkpoints) rides along without touching the pixel states.  So the training forward's image and
alphas are the inference forward's bit for bit, on the bench scene at reduced N and on long saturated lists, and the work units
it publishes are exactly one per started GS_UNIT entries of every quadrant sublist.  (Sublists, rows and gradients against the
oracle and across captured / eager / depth rounds: test_gpu_parity.py, test_gpu_train_graph.py, test_gpu_rounds.py,
test_gpu_contributors.py.)"""
import numpy as np
import pytest
import torch

from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import rendering
from scenes import config_bench_1m, config_long_lists

pytestmark = pytest.mark.gpu

SCENES = {
    "bench_200k": lambda: config_bench_1m(n=200_000),
    "long_lists": lambda: config_long_lists(seed=1, n=45_000, width=640, height=368),
}


def _render(sc, train: bool, culling: str):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items() if isinstance(v, np.ndarray)}
    ins = [t[k].clone().requires_grad_(train) for k in ("means", "quats", "scales", "opacities", "shs")]
    dbg = {} if train else None
    with torch.set_grad_enabled(train):
        img, alpha, _ = rendering.rasterization(*ins, t["viewmats"], t["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=3,
                                                packed=False, backgrounds=t["backgrounds"], absgrad=train,
                                                _tile_culling=culling, _debug=dbg)
    torch.cuda.synchronize()
    return img.detach().cpu().numpy(), alpha.detach().cpu().numpy(), dbg


@pytest.mark.parametrize("culling", ["tight", "gsplat"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_training_forward_is_the_inference_forward(name, culling):
    sc = SCENES[name]()
    img_t, alpha_t, dbg = _render(sc, True, culling)
    img_i, alpha_i, _ = _render(sc, False, culling)
    assert img_t.tobytes() == img_i.tobytes(), f"{name}: training image differs from the inference image"
    assert alpha_t.tobytes() == alpha_i.tobytes(), f"{name}: training alphas differ from the inference alphas"
    qcnt = dbg["qcnt"].cpu().numpy().astype(np.int64)
    units = int(dbg["unit_counter"].item())
    assert qcnt.sum() > 0
    assert units == int(((qcnt + nat.GS_UNIT - 1) // nat.GS_UNIT).sum()), "published work units != started units of the sublists"
