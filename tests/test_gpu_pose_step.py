"""Pose refinement inside the captured train step (`TrainStepGraph(poses=CameraDeltas(n))`, DESIGN.md "Poses in the captured step") on
the scene of tests/test_gpu_train_graph.py: off means off bit for bit; the captured step equals its own eager form; the 6-vector's
gradient is the eager path's (rasterization(_camera_grads=True) + autograd) to the project's gradient contract; the update is dense
Adam (tests/adam_ref.py); the step guard covers the deltas and their moments; the combinations; and it refines."""
import numpy as np
import pytest
import torch

import adam_ref as A
import pose_ref as R
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.pose import CameraDeltas
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
from test_gpu_train_graph import _assert_same, _setup

pytestmark = pytest.mark.gpu
GRAD_RTOL = 1e-3   # the project's gradient contract (tests/test_gpu_camgrad.py)
POSE_LR, POSE_BETAS, POSE_EPS = 1e-3, (0.9, 0.999), 1e-15


def _poses(dev, n_views=3, seed=None):
    """Zero corrections, or (seed) omega ~ 0.02 rand, tau ~ 0.05 rand: a Jacobian that is not the identity."""
    cd = CameraDeltas(n_views).to(dev)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        d = torch.cat([0.02 * (2 * torch.rand((n_views, 3), generator=g) - 1), 0.05 * (2 * torch.rand((n_views, 3), generator=g) - 1)], dim=1)
        with torch.no_grad():
            cd.deltas.copy_(d.to(dev))
    return cd


def _pose_state(runner):
    ps = runner.pose_state
    return runner.poses.deltas.detach().clone(), ps.exp_avg.clone(), ps.exp_avg_sq.clone()


def _assert_same_poses(ra, rb, what=""):
    for x, y, name in zip(_pose_state(ra), _pose_state(rb), ("deltas", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), (what, name)
    assert ra.pose_state.step == rb.pose_state.step


# ---- 0. the record and the compose entry on their own ---------------------------------------------------------------------------
def test_record_takes_the_raw_matrix_by_pointer_or_by_value_and_compose_matches_the_reference():
    import ctypes as ct
    from easy_gaussian_splatting_amd import _native as nat
    dev, L = torch.device("cuda:0"), nat.lib()
    rng = np.random.default_rng(2)
    n_views = 5
    deltas = np.stack([R.delta_at(rng, th) for th in R.THETAS]).astype(np.float32)
    deltas[0] = 0.0
    d_dev = torch.from_numpy(deltas).to(dev)
    rec = torch.zeros((nat.GS_POSE_REC_FLOATS,), dtype=torch.float32, device=dev)
    out = torch.zeros((16,), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    mats = [np.ascontiguousarray(R.random_rigid(rng).astype(np.float32)) for _ in range(n_views)]
    mats[0][0, 1] = -0.0
    for v in range(n_views):
        if v % 2:   # by value: the 16 floats travel as kernel arguments
            nat.check(L.gs_pose_step_inputs(st, v, n_views, None, mats[v].ctypes.data_as(ct.c_void_p), 1e-3, 0.9, 0.999, v + 1, rec.data_ptr()), "inputs")
        else:       # by device pointer
            src = torch.from_numpy(mats[v]).to(dev)
            nat.check(L.gs_pose_step_inputs(st, v, n_views, src.data_ptr(), None, 1e-3, 0.9, 0.999, v + 1, rec.data_ptr()), "inputs")
        nat.check(L.gs_pose_compose(st, n_views, rec.data_ptr(), d_dev.data_ptr(), out.data_ptr()), "compose")
        got, r = out.cpu().numpy().reshape(4, 4), rec.cpu().numpy()
        assert np.array_equal(r[:16].view(np.uint32), mats[v].reshape(-1).view(np.uint32)) and int(r[18:19].view(np.int32)[0]) == v
        bc1, bc2 = 1.0 - float(np.float32(0.9)) ** (v + 1), 1.0 - float(np.float32(0.999)) ** (v + 1)
        assert r[16] == np.float32(float(np.float32(1e-3)) / bc1) and r[17] == np.float32(1.0 / np.sqrt(bc2))
        ref = R.compose64(deltas[v], mats[v]).numpy()
        bound = np.maximum(np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64), 2.0 ** -24 * np.abs(ref).max(axis=1, keepdims=True))
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), v
        if v == 0:
            assert np.array_equal(got.view(np.uint32), mats[0].view(np.uint32))   # delta == 0: bit for bit, the -0 included
    # neither pointer nor values: the record keeps the matrix it holds, the view and the step count change
    nat.check(L.gs_pose_step_inputs(st, 2, n_views, None, None, 1e-3, 0.9, 0.999, 9, rec.data_ptr()), "inputs")
    r = rec.cpu().numpy()
    assert np.array_equal(r[:16], mats[n_views - 1].reshape(-1)) and int(r[18:19].view(np.int32)[0]) == 2
    for bad in ((-1, n_views), (n_views, n_views), (0, 0)):
        with pytest.raises(ValueError):
            nat.check(L.gs_pose_step_inputs(st, bad[0], bad[1], None, None, 1e-3, 0.9, 0.999, 1, rec.data_ptr()), "inputs")


# ---- 1. off means off ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_adam", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
def test_zero_poses_at_zero_rate_change_nothing(use_graph, fuse_adam):
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    poses = _poses(dev)
    ra = TrainStepGraph(ma, oa, lc, datas[0], gts[0], use_graph=use_graph, check_every=2, fuse_adam=fuse_adam)
    rb = TrainStepGraph(mb, ob, lc, datas[0], gts[0], use_graph=use_graph, check_every=2, fuse_adam=fuse_adam, poses=poses, pose_lr=0.0)
    assert "poses" not in ra.report() and rb.report()["poses"] is True   # (absent, not False: as "mcmc" and "scale_reg")
    assert not any("pose" in k or k in ("cam_partials", "w2c_raw", "v_viewmats", "v_campos", "v_delta") for k in ra.buf)
    for it in range(7):
        v = it % 3
        ma.update_learning_rate(it); mb.update_learning_rate(it)
        la = ra.step(datas[v], gts[v])["loss3"]
        out = rb.step(datas[v], gts[v], view_index=v)
        ra.finish(); rb.finish()
        assert torch.equal(la, out["loss3"]), it
        assert torch.equal(out["viewmat"], datas[v]["w2c"]), it
        _assert_same(ma, oa, mb, ob, f"step {it}")
    assert not poses.deltas.detach().any()
    assert rb.pose_state.step == 7 and set(rb.step(datas[0], gts[0], view_index=0)) >= {"viewmat", "v_delta"}
    rb.finish()


# ---- 2. captured == its own eager form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_adam", [True, False])
def test_captured_pose_step_equals_its_eager_form(fuse_adam):
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    kw = dict(check_every=2, fuse_adam=fuse_adam, pose_lr=POSE_LR)
    ra = TrainStepGraph(ma, oa, lc, datas[0], gts[0], use_graph=True, poses=_poses(dev, seed=5), **kw)
    rb = TrainStepGraph(mb, ob, lc, datas[0], gts[0], use_graph=False, poses=_poses(dev, seed=5), **kw)
    start = ra.poses.deltas.detach().clone()
    for it in range(7):
        v = it % 3
        ma.update_learning_rate(it); mb.update_learning_rate(it)
        oa_, ob_ = ra.step(datas[v], gts[v], view_index=v), rb.step(datas[v], gts[v], view_index=v)
        ra.finish(); rb.finish()
        assert torch.equal(oa_["v_delta"], ob_["v_delta"]) and bool(oa_["v_delta"].any()), it
        assert torch.equal(oa_["viewmat"], ob_["viewmat"]) and torch.equal(oa_["loss3"], ob_["loss3"]), it
    _assert_same(ma, oa, mb, ob, "captured vs eager form")
    _assert_same_poses(ra, rb, "captured vs eager form")
    assert bool((ra.poses.deltas.detach() != start).all())   # (dense Adam: every entry of every row has moved)
    assert ra.report()["graph"] and not rb.report()["graph"] and ra.report()["overflows"] == 0


# ---- 3. the gradient is the eager path's ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,with_mask", [(0, False), (3, False), (3, True)])
def test_v_delta_is_the_eager_camera_gradient_chained_to_the_six_vector(degree, with_mask):
    dev, make, datas, gts = _setup()
    (ma, oa), (mb, ob) = make(), make()
    ma.active_sh_degree = mb.active_sh_degree = degree
    lc = LossComputer(0.2, clamp_input=True)
    mask = None
    if with_mask:
        mask = torch.zeros((208, 320), device=dev)
        mask[40:150, 60:260] = 1.0
    poses = _poses(dev, seed=7)
    runner = TrainStepGraph(mb, ob, lc, datas[0], gts[0], mask, poses=poses, pose_lr=POSE_LR)
    worst = 0.0
    for v in (1, 2):
        delta = poses.deltas.detach()[v].cpu().numpy().astype(np.float64)
        params = {k: getattr(mb, k).detach().clone() for k in mb.param_names}   # (the model as the step is about to see it)
        out = runner.step(datas[v], gts[v], mask, view_index=v)
        runner.finish()
        with torch.no_grad():
            for k, p in params.items():
                getattr(ma, k).copy_(p)
        V = out["viewmat"].detach().clone().requires_grad_(True)
        res = ma({**datas[v], "w2c": V}, clamp=False)
        lc.get_loss_dict(res["render_img"], gts[v], mask)["total"].backward()
        for k in ma.param_names:
            getattr(ma, k).grad = None
        ref = R.vjp64(delta, datas[v]["w2c"].cpu().numpy(), V.grad[:3].cpu().numpy())
        got = out["v_delta"].cpu().numpy().astype(np.float64)
        ratio = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"degree {degree}, mask {with_mask}, view {v}: max |v_delta - ref| / max |ref| = {ratio:.3e}  (ref = {ref})")
        assert np.abs(ref).max() > 0
        worst = max(worst, ratio)
    assert worst <= GRAD_RTOL, worst


# ---- 4. the update is Adam ----------------------------------------------------------------------------------------------------
def test_the_update_is_dense_adam_on_all_rows():
    dev, make, datas, gts = _setup()
    m, o = make()
    lc = LossComputer(0.2, clamp_input=True)
    runner = TrainStepGraph(m, o, lc, datas[0], gts[0], poses=_poses(dev, seed=9), pose_lr=POSE_LR, pose_betas=POSE_BETAS, pose_eps=POSE_EPS)
    for t, v in enumerate((0, 1, 2), start=1):
        p0, m0, v0 = (x.cpu().numpy() for x in _pose_state(runner))
        out = runner.step(datas[v], gts[v], view_index=v)
        runner.finish()
        g = np.zeros((3, 6), dtype=np.float32)
        g[v] = out["v_delta"].cpu().numpy()
        p1, m1, v1 = (x.cpu().numpy() for x in _pose_state(runner))
        ref = A.adam_ref(p0, g, m0, v0, POSE_LR, t, POSE_BETAS[0], POSE_BETAS[1], POSE_EPS)
        ratios = A.error_ratios((p1, m1, v1), p0, ref)
        print(f"pose step {t} on view {v}: error / bound  p {ratios['p']:.3f}  m {ratios['m']:.3f}  v {ratios['v']:.3f}")
        assert ratios["p"] <= 1.0 and ratios["m"] <= 1.0 and ratios["v"] <= 1.0, ratios
        if t > 1:   # the rows of the views stepped before are idle now: their moments decay (and the rows still move)
            idle = [r for r in range(3) if r != v and m0[r].any()]
            assert idle
            for r in idle:
                assert (np.abs(m1[r]) < np.abs(m0[r])).all() and (v1[r] < v0[r]).all() and (p1[r] != p0[r]).all(), (t, r)
    assert runner.pose_state.step == 3


# ---- 5. the guard covers the poses ----------------------------------------------------------------------------------------------
def test_overflow_voids_the_pose_update_and_the_replay_applies_it():
    dev, make, datas, gts = _setup(n=30000, n_views=3, dist=4.0)
    far = dict(datas[0])
    w2c = far["w2c"].clone()
    w2c[2, 3] += 14.0   # camera pulled back: splats shrink, few intersections
    far["w2c"] = w2c
    seq = [(far, 0), (datas[1], 1), (datas[2], 2), (far, 0), (datas[0], 0), (datas[1], 1)]
    lc = LossComputer(0.2, clamp_input=True)
    done = []
    for (first, view), margin in (((far, 0), 1.02), ((datas[1], 1), 4.0)):
        m, o = make()
        r = TrainStepGraph(m, o, lc, {**first, "view_index": view}, gts[0], margin=margin, check_every=4, poses=_poses(dev, seed=5), pose_lr=POSE_LR)
        for it, (d, v) in enumerate(seq):   # no finish() in between: the host keeps enqueueing behind the overflow
            r.step(d, gts[it % 3], view_index=v)
        r.finish()
        done.append((m, o, r))
    (mt, ot, rt), (ma, oa, ra) = done
    print(f"[pose step] margin 1.02 overflowed {rt.report()['overflows']} x and replayed {rt.report()['replayed_steps']} steps; "
          f"margin 4 overflowed {ra.report()['overflows']} x")
    assert rt.report()["overflows"] >= 1 and rt.report()["replayed_steps"] >= 1 and rt.report()["steps"] == len(seq)
    assert ra.report()["overflows"] == 0 and ra.report()["steps"] == len(seq)
    _assert_same(mt, ot, ma, oa, "replayed != never overflowed")
    _assert_same_poses(rt, ra, "replayed != never overflowed")


# ---- 6. combinations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["mcmc", "scale_reg", "rounds"])
def test_combinations_captured_equals_eager_form(combo):
    dev, make, datas, gts = _setup()
    runs = []
    for use_graph in (True, False):
        m, o = make()
        kw, lc = {}, LossComputer(0.2, clamp_input=True)
        if combo == "mcmc":
            kw = dict(mcmc=M.MCMCStrategy(m, cap_max=m.nbr_gaussians, noise_lr=5e4, refine_start=10 ** 9, refine_stop=10 ** 9, refine_every=1,
                                          generator=torch.Generator(device=dev).manual_seed(5), noise="counter", seed=2 ** 63 + 12345),
                      mcmc_reg=(0.01, 0.01))
        elif combo == "scale_reg":
            m.USE_SCALE_REGULARIZATION, m.MAX_SCALE_RATIO = True, 2.0
            lc = LossComputer(0.2, clamp_input=True, model=m, lambda_scale=0.05)
        else:
            kw = dict(rounds="on")
        r = TrainStepGraph(m, o, lc, datas[0], gts[0], use_graph=use_graph, check_every=2, poses=_poses(dev, seed=5), pose_lr=POSE_LR, **kw)
        rep = r.report()
        assert rep["poses"] and rep["graph"] == use_graph and rep.get("mcmc", False) == (combo == "mcmc")
        assert rep.get("scale_reg", False) == (combo == "scale_reg") and rep["rounds"] == (combo == "rounds")
        deltas = []
        for it in range(4):
            m.update_learning_rate(it)
            out = r.step(datas[it % 3], gts[it % 3], view_index=it % 3)
            r.finish()
            deltas.append(out["v_delta"].clone())
        runs.append((m, o, r, deltas))
    (ma, oa, ra, da), (mb, ob, rb, db) = runs
    _assert_same(ma, oa, mb, ob, combo)
    _assert_same_poses(ra, rb, combo)
    for x, y in zip(da, db):
        assert torch.equal(x, y) and bool(x.any())


# ---- 7. it refines --------------------------------------------------------------------------------------------------------------
def test_sixty_captured_steps_pull_perturbed_cameras_towards_the_true_ones():
    dev, make, datas, gts = _setup()
    m, o = make()
    for grp in o.param_groups:   # the scene is frozen
        grp["lr"] = 0.0
    lc = LossComputer(0.2, clamp_input=True)
    rng = np.random.default_rng(4)
    with torch.no_grad():
        targets = [m(d, clamp=False)["render_img"].detach().clamp(0.0, 1.0).contiguous() for d in datas]
    start, truth = [], []
    for d in datas:   # w2c_start = P w2c_true with P = E(omega 0.01, tau 0.03); the true correction is P^-1
        axis, tdir = rng.standard_normal(3), rng.standard_normal(3)
        pert = np.concatenate([0.01 * axis / np.linalg.norm(axis), 0.03 * tdir / np.linalg.norm(tdir)])
        P = R.compose64(pert, np.eye(4)).numpy()
        start.append({**d, "w2c": torch.from_numpy((P @ d["w2c"].cpu().numpy().astype(np.float64)).astype(np.float32)).to(dev)})
        Rm = R.compose64(np.concatenate([-pert[:3], np.zeros(3)]), np.eye(4)).numpy()[:3, :3]
        truth.append(np.concatenate([-pert[:3], -Rm @ pert[3:]]))
    truth = np.stack(truth)
    poses = _poses(dev)
    runner = TrainStepGraph(m, o, lc, start[0], targets[0], poses=poses, pose_lr=POSE_LR)

    def losses():
        with torch.no_grad():
            return [float(lc.get_loss_dict(m({**start[v], "w2c": poses(start[v]["w2c"], v)}, clamp=False)["render_img"], targets[v], None)["total"])
                    for v in range(3)]
    before = {k: getattr(m, k).detach().clone() for k in m.param_names}
    l0, e0 = losses(), float(np.linalg.norm(truth, axis=1).mean())
    for it in range(60):
        runner.step(start[it % 3], targets[it % 3], view_index=it % 3)
    runner.finish()
    l1 = losses()
    e1 = float(np.linalg.norm(poses.deltas.detach().cpu().numpy().astype(np.float64) - truth, axis=1).mean())
    print(f"[pose step] loss per view {['%.5f' % x for x in l0]} -> {['%.5f' % x for x in l1]}; mean |delta - truth| {e0:.5f} -> {e1:.5f}")
    assert all(torch.equal(getattr(m, k).detach(), before[k]) for k in m.param_names)
    assert all(b < a for a, b in zip(l0, l1)), (l0, l1)
    assert e1 < e0, (e0, e1)
    assert runner.report()["steps"] == 60 and runner.report()["graph"]
