"""The scale-ratio regulariser (use_scale_regularization) on the GPU:

* gs_scale_reg against torch autograd of `GaussianModel.get_regularization_dict()` on the same log-scales: the gradient bit for
  bit, the value to 1e-6 of an fp64 sum, the same bits from two calls;
* the captured step (`TrainStepGraph`, both Adam forms, both binnings, hipGraph or not, across a densify_and_prune) against the eager
  loop with the regulariser on;
* the captured view-parallel step against the eager exchange's "regularised" path, two ranks on one GPU.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from scenes import make_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def _model_of(log_scales: torch.Tensor, R: float) -> GaussianModel:
    n = log_scales.shape[0]
    quats = torch.zeros(n, 4)
    quats[:, 0] = 1.0
    return GaussianModel(means=torch.zeros(n, 3), log_scales=log_scales.cpu(), quats=quats, sh_0=torch.zeros(n, 1, 3),
                         sh_rest=torch.zeros(n, 15, 3), logit_opacities=torch.zeros(n), sh_degree=3,
                         use_scale_regularization=True, max_scale_ratio=R).to(log_scales.device)


def _rows(dev):
    """Log-scales with every case of the gradient's semantics, then random rows; N = 4010 (no multiple of the block size)."""
    special = torch.tensor([[0.0, 0.0, -3.0],     # tied maxima
                            [0.0, -3.0, -3.0],    # tied minima
                            [-1.0, -1.0, -1.0],   # all axes equal: ratio 1
                            [0.7, 0.1, 0.0],      # ratio exactly R (R is taken from this row)
                            [0.2, 0.1, 0.0],      # ratio below R
                            [-2.0, 1.5, 0.3],
                            [1.5, 1.5, 1.5],
                            [-4.0, 2.0, 2.0],     # tied maxima above R
                            [3.0, -4.0, -4.0]])   # tied minima above R
    rnd = torch.randn((1000, 3), generator=torch.Generator().manual_seed(3)) * 0.45 - 3.0
    # log-scales over a wide range, ratios above R: the gradient carries exp(l) itself, so these pin the kernel's exp to torch.exp
    l = torch.linspace(-12.0, 6.0, 3001)
    wide = torch.stack([l, l - 0.3, l + 0.9], 1)
    return torch.cat([special, rnd, wide]).to(dev)


def _run(ls, R, lam, v=None, loss3=None):
    L = nat.lib()
    N = ls.shape[0]
    ws = torch.zeros((int(L.gs_scale_reg_workspace_floats(N)),), dtype=torch.float32, device=ls.device)
    st = torch.cuda.current_stream(ls.device).cuda_stream
    nat.check(L.gs_scale_reg(st, N, ls.data_ptr(), R, lam, None if loss3 is None else loss3.data_ptr(), ws.data_ptr(),
                             None if v is None else v.data_ptr()), "gs_scale_reg")
    torch.cuda.synchronize()
    return ws


def test_scale_reg_kernel_equals_autograd():
    dev = torch.device("cuda:0")
    ls0 = _rows(dev)
    s3 = torch.exp(ls0[3])
    R = float(s3.max() / s3.min())   # the row "ratio exactly R"
    lam = 0.37
    ratio = torch.exp(ls0).amax(1) / torch.exp(ls0).amin(1)
    frac = float((ratio >= R).float().mean())
    assert 0.3 < frac < 0.9, frac
    # torch: the eager path's own expression (model.get_regularization_dict) under autograd
    m = _model_of(ls0, R)
    reg = m.get_regularization_dict()["scale_reg"]
    (lam * reg).backward()
    g_ref = m.log_scales.grad.detach()
    assert float(g_ref[2].abs().max()) == 0.0 and float(g_ref[4].abs().max()) == 0.0   # all equal (ratio 1) / below R
    assert float(g_ref[3].abs().max()) > 0.0   # ratio == R passes
    assert float(g_ref[0, 0]) == float(g_ref[0, 1]) > 0.0   # tied maxima share
    ls = ls0.clone().contiguous()
    v = torch.zeros_like(ls)
    loss3 = torch.tensor([0.25, 0.5, 0.75], device=dev)
    ws = _run(ls, R, lam, v, loss3)
    assert torch.equal(v, g_ref), f"max |diff| {float((v - g_ref).abs().max())}, rows {torch.nonzero((v != g_ref).any(1))[:8].flatten().tolist()}"
    ref64 = float(torch.mean(torch.clamp(ratio.double(), min=R) - R))
    assert abs(float(ws[0]) - ref64) <= 1e-6 * abs(ref64)
    assert abs(float(reg) - float(ws[0])) <= 1e-6 * abs(ref64)
    # loss3: only the total moves, by lambda * reg rounded as the eager total + lambda * reg
    assert float(loss3[0]) == 0.25 and float(loss3[1]) == 0.5
    assert torch.equal(loss3[2], torch.tensor(0.75, device=dev) + lam * ws[0])
    # the same bits again; without v_log_scales only the value
    v2 = torch.full_like(ls, 0.5)
    ws2 = _run(ls, R, lam, v2)
    assert torch.equal(ws2[0], ws[0]) and torch.equal(v2, 0.5 + g_ref)
    ws3 = _run(ls, R, lam)
    assert torch.equal(ws3[0], ws[0])


def _setup(n=20000, W=320, H=208, n_views=3, seed=3):
    dev = torch.device("cuda:0")
    sc = make_scene(n, W, H, sh_degree=3, n_views=n_views, seed=seed, scale_range=(0.01, 0.08), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"])
    ls = torch.log(T(sc["scales"]))
    ratio = torch.exp(ls).amax(1) / torch.exp(ls).amin(1)
    R = float(torch.quantile(ratio.double(), 2.0 / 3.0))   # a third of the Gaussians above it

    def make():
        m = GaussianModel(means=T(sc["means"]), log_scales=ls.clone(), quats=T(sc["quats"]),
                          sh_0=shs[:, :1].contiguous(), sh_rest=shs[:, 1:].contiguous(),
                          logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3, white_background=True,
                          means_lr_schedule_max_steps=40, use_scale_regularization=True, max_scale_ratio=R).to(dev)
        m.DENSIFY_GRAD_THRESH = 0.0   # (the refinement below clones / splits every visible Gaussian)
        return m, build_optimizers(m, *LRS, fused="hip")

    datas = [{"w2c": T(sc["viewmats"][v]).to(dev), "K": T(sc["Ks"][v]).to(dev), "width": W, "height": H} for v in range(n_views)]
    g = torch.Generator().manual_seed(11)
    gts = [torch.rand((H, W, 3), generator=g).to(dev) for _ in range(n_views)]
    return dev, make, datas, gts, R


def _eager_step(model, opt, lc, data, gt):
    out = model(data, clamp=False)
    loss = lc.get_loss_dict(out["render_img"], gt)
    loss["total"].backward()
    model.update_statistics(data, out)
    opt.step()
    opt.zero_grad()
    return torch.stack([loss["l1"].detach(), loss["ssim"].detach(), loss["total"].detach()]), loss["scale_reg"].detach()


def _state(m, o):
    out = {}
    for k in m.param_names:
        out[k] = getattr(m, k).detach().clone()
        mm, vv = o.moments_of(getattr(m, k))
        out["m_" + k], out["v_" + k] = mm.clone(), vv.clone()
    for k in ("max_radii", "grad_norm_accum", "collecting_counts"):
        out[k] = getattr(m, k).clone()
    return out


def _close(a, b, rtol=1e-6):
    return abs(float(a) - float(b)) <= rtol * max(abs(float(b)), 1e-30)


@pytest.mark.parametrize("binning", ["tiles", "bins"])
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_captured_step_with_the_regulariser_equals_eager(fuse_adam, binning, monkeypatch):
    """Seven steps -- three, densify_and_prune (N grows, the runner re-captures with the new 1 / N), four -- of the eager loop and of
    two runners (hipGraph replay and the same sequence issued eagerly): parameters, moments and statistics bit for bit; l1 and
    1 - ssim bit for bit, the total and scale_reg to 1e-6 (the eager mean sums in another order)."""
    monkeypatch.setenv("GS_BINNING", binning)
    dev, make, datas, gts, R = _setup()
    (ma, oa), (mb, ob), (mc, oc) = make(), make(), make()
    lam = 0.05
    lca, lcb, lcc = (LossComputer(0.2, clamp_input=True, model=m, lambda_scale=lam) for m in (ma, mb, mc))
    rb = TrainStepGraph(mb, ob, lcb, datas[0], gts[0], use_graph=True, check_every=2, fuse_adam=fuse_adam)
    rc = TrainStepGraph(mc, oc, lcc, datas[0], gts[0], use_graph=False, check_every=2, fuse_adam=fuse_adam)
    assert rb.report()["scale_reg"] and rb.report()["max_scale_ratio"] == R and rb.report()["lambda_scale"] == lam
    n0 = ma.nbr_gaussians
    totals = []
    for it in range(7):
        if it == 3:
            for m in (ma, mb, mc):
                m.densify_and_prune(generator=torch.Generator(device=dev).manual_seed(5))
            assert ma.nbr_gaussians == mb.nbr_gaussians == mc.nbr_gaussians > n0
        v = it % 3
        for m in (ma, mb, mc):
            m.update_learning_rate(it)
        l_ref, reg_ref = _eager_step(ma, oa, lca, datas[v], gts[v])
        outs = [r.step(datas[v], gts[v]) for r in (rb, rc)]
        for r in (rb, rc):
            r.finish()
        for out in outs:
            assert torch.equal(out["loss3"][:2], l_ref[:2]), it
            assert _close(out["loss3"][2], l_ref[2]) and _close(out["scale_reg"], reg_ref), (it, float(out["scale_reg"]), float(reg_ref))
            assert float(reg_ref) > 0.0
        assert torch.equal(outs[0]["loss3"], outs[1]["loss3"]) and torch.equal(outs[0]["scale_reg"], outs[1]["scale_reg"])
        totals.append(float(l_ref[2]))
        sa, sb, sc_ = _state(ma, oa), _state(mb, ob), _state(mc, oc)
        for k in sa:
            assert torch.equal(sb[k], sc_[k]), (it, k, "graph != no graph")
            assert torch.equal(sb[k], sa[k]), (it, k, float((sb[k] - sa[k]).abs().max()))
    # the device-side loss log (applied steps since the re-capture): totals with lambda * reg
    for r in (rb, rc):
        hist = r.loss_history(4)
        assert hist.shape == (4, 3)
        for h, t in zip(hist[:, 2].tolist(), totals[3:]):
            assert _close(h, t)
        rep = r.report()
        assert rep["steps"] == 7 and rep["overflows"] == 0 and rep["rebuilds"] >= 2


def test_captured_step_without_the_regulariser_has_no_new_outputs():
    dev, make, datas, gts, R = _setup(n=6000)
    m, o = make()
    m.USE_SCALE_REGULARIZATION = False
    r = TrainStepGraph(m, o, LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05), datas[0], gts[0])
    out = r.step(datas[0], gts[0])
    r.finish()
    assert set(out) == {"render_img", "loss3", "batch_radii", "absgrad"}
    assert "scale_reg" not in r.report()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_vp(dev):
    sc = make_scene(3000, 160, 112, sh_degree=3, n_views=2, seed=12, scale_range=(0.03, 0.15), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    shs = T(sc["shs"])
    model = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]),
                          sh_0=shs[:, :1].contiguous(), sh_rest=shs[:, 1:].contiguous(),
                          logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3, white_background=True,
                          use_scale_regularization=True, max_scale_ratio=1.5).to(dev)
    opt = build_optimizers(model, 1.6e-3, 5e-3, 1e-3, 2.5e-2, 1.25e-3, 5e-2, fused="hip")
    datas = [{"w2c": T(sc["viewmats"][v]).to(dev), "K": T(sc["Ks"][v]).to(dev), "width": 160, "height": 112} for v in range(2)]
    targets = torch.rand((2, 112, 160, 3), generator=torch.Generator().manual_seed(9)).to(dev)
    return model, opt, datas, targets


def _snap(model, opt):
    out = {k: getattr(model, k).detach().cpu().numpy() for k in model.param_names}
    out.update({"m_" + k: opt.moments_of(getattr(model, k))[0].cpu().numpy() for k in model.param_names})
    out.update(gn=model.grad_norm_accum.cpu().numpy(), cnt=model.collecting_counts.cpu().numpy(), rad=model.max_radii.cpu().numpy())
    return out


def _worker_vp(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from easy_gaussian_splatting_amd.distributed import ViewParallelStep
    from easy_gaussian_splatting_amd.train_graph import ViewParallelGraphStep
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n_steps = 5
    # (a) the eager exchange, "regularised": autograd's log-scale gradient (the regulariser's) added into the bucket
    model, opt, datas, targets = _make_vp(dev)
    vp = ViewParallelStep(model, opt)
    lc = LossComputer(0.2, clamp_input=True, model=model, lambda_scale=0.1)
    e_tot = []
    for it in range(n_steps):
        vp.begin_step(datas[rank])
        out = model(datas[rank], clamp=False)
        vp.after_forward(datas[rank], out)
        loss = lc.get_loss_dict(out["render_img"], targets[rank])
        loss["total"].backward()
        assert model.log_scales.grad is not None
        vp.step(datas[rank], out)
        e_tot.append(float(loss["total"]))
        model.update_learning_rate(it + 1)
    torch.cuda.synchronize()
    eager = _snap(model, opt)
    # (b) captured
    model, opt, datas, targets = _make_vp(dev)
    vp = ViewParallelStep(model, opt, guard_words=True)
    runner = ViewParallelGraphStep(model, opt, LossComputer(0.2, clamp_input=True, model=model, lambda_scale=0.1), datas[rank],
                                   targets[rank], None, vp=vp, check_every=2)
    c_tot = []
    for it in range(n_steps):
        out = runner.step(datas[rank], targets[rank])
        runner.finish()
        c_tot.append(float(out["loss3"][2]))
        model.update_learning_rate(it + 1)
    runner.finish()
    torch.cuda.synchronize()
    cap = _snap(model, opt)
    np.savez(os.path.join(out_dir, f"s{rank}.npz"), tot_eager=np.asarray(e_tot), tot_captured=np.asarray(c_tot), steps=runner.report()["steps"],
             **{"e_" + k: v for k, v in eager.items()}, **{"c_" + k: v for k, v in cap.items()})
    dist.barrier()
    dist.destroy_process_group()


def test_captured_view_parallel_step_with_the_regulariser(tmp_path):
    mp.spawn(_worker_vp, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [np.load(os.path.join(tmp_path, f"s{k}.npz")) for k in range(2)]
    for k in range(2):
        assert int(r[k]["steps"]) == 5
        for f in r[k].files:
            if f.startswith("e_"):
                np.testing.assert_array_equal(r[k]["c_" + f[2:]], r[k][f], err_msg=f"rank {k}: captured != eager in {f[2:]}")
        np.testing.assert_allclose(r[k]["tot_captured"], r[k]["tot_eager"], rtol=1e-6)
    for f in r[0].files:
        if f.startswith("c_"):
            np.testing.assert_array_equal(r[0][f], r[1][f], err_msg=f"replicas diverged in {f[2:]}")
