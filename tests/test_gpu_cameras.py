"""The HIP path under general cameras and non-default projection keywords (tests/cameras.py): rotations with roll, translations
with three components, fx != fy, a principal point off the image centre, one K per camera, cameras inside the cloud (Gaussians
behind them, footprints of thousands of pixels), and `near_plane` / `far_plane` / `radius_clip` / `eps2d` away from their
defaults.  Every check is an existing one of the neighbouring files with its bounds unchanged, on these cameras;
tests/test_oracle.py pins on the CPU that the configurations hold what is claimed here (culls that cull, no symmetric R, razor
fraction) and that the two oracles agree on them."""
import numpy as np
import pytest
import torch

import cameras
import parity_log
import test_gpu_camgrad as CG
import test_gpu_channels as CH
import test_gpu_sh4 as SH4
import test_gpu_train_graph as TG
from test_gpu_parity import check_backward, check_backward_unmasked, check_forward, dev, run_hip, run_oracle

pytestmark = pytest.mark.gpu
W, H = 160, 112
_ORACLE = {}


def _config(name):
    """(scene, projection keywords, fp64 oracle forward) of a named configuration at the suite's size: computed once."""
    if name not in _ORACLE:
        sc, proj = cameras.config_scene(name, W=W, H=H, C=2)
        _ORACLE[name] = (sc, proj, run_oracle(sc, **proj))
    return _ORACLE[name]


# ---- a. forward and backward parity against the fp64 C oracle ----------------------------------------------------------------
@pytest.mark.parametrize("culling", ["gsplat", "gsplat_eager", "tight"])
@pytest.mark.parametrize("name", list(cameras.CONFIGS))
def test_forward_backward_parity_under_general_cameras(name, culling):
    sc, proj, fw = _config(name)
    hip = run_hip(sc, culling=culling, fw=fw, **proj)
    check_forward(hip, fw, lists=culling != "tight")
    check_backward(hip, fw)
    if culling == "gsplat":
        check_backward_unmasked(sc, fw, culling, **proj)


# ---- b. cull boundaries, by construction -------------------------------------------------------------------------------------
NEAR, FAR = 0.5, 4.0   # exact in fp32


def _boundary_scene():
    """Identity view, isotropic Gaussians (unit quaternion, one scale), depths that fp32 and fp64 agree about: the view matrix
    is the identity, so the camera-space z IS the stored fp32 z in either precision.  Gaussians 0-3 sit at exactly near / one fp32
    step in front of it / exactly far / one fp32 step beyond it; 4-7 well inside the slab, with footprints of four sizes."""
    f = np.float32
    z = np.array([NEAR, np.nextafter(f(NEAR), f(0)), FAR, np.nextafter(f(FAR), f(np.inf)), 2.0, 2.0, 1.0, 3.0], f)
    assert z[1] < f(NEAR) and z[3] > f(FAR)
    u = np.array([-0.15, -0.05, 0.1, 0.2, -0.1, 0.15, 0.05, 0.0], f)   # x / z, y / z: spread over the image
    v = np.array([0.1, -0.1, 0.05, -0.05, -0.12, 0.12, 0.0, 0.02], f)
    means = np.stack([u * z, v * z, z], 1).astype(f)
    assert np.array_equal(means[:, 2], z)
    s = np.array([0.02, 0.02, 0.25, 0.25, 0.0625, 0.125, 0.05, 0.03125], f)
    N = z.size
    rng = np.random.default_rng(0)
    shs = np.zeros((N, 4, 3), f)
    shs[:, 0] = rng.uniform(-1.0, 1.7, (N, 3))
    shs[:, 1:] = rng.standard_normal((N, 3, 3)) * 0.1
    K = np.array([[[64.0, 0, 24.5], [0, 80.0, 30.5], [0, 0, 1]]], f)
    return dict(means=means, quats=np.tile(np.array([1, 0, 0, 0], f), (N, 1)), scales=np.repeat(s[:, None], 3, 1),
                opacities=np.array([0.9, 0.9, 0.8, 0.8, 0.7, 0.5, 0.6, 0.85], f), shs=shs, viewmats=np.eye(4, dtype=f)[None], Ks=K,
                backgrounds=np.array([[0.2, 0.4, 0.6]], f), width=64, height=48, sh_degree=1)


def _radius_margin(fw):
    """Distance of 3 sqrt(lambda_max) of every visible Gaussian to the nearest integer, from the oracle's conics: the ceil()
    that makes the radius must not itself sit on a rounding edge."""
    A, B, C = (fw["conics"][..., i] for i in range(3))
    vis = fw["radii"] > 0
    det = np.where(vis, A * C - B * B, 1.0)
    a, b, c = C / det, -B / det, A / det   # the blurred 2-D covariance
    mid = 0.5 * (a + c)
    lam = mid + np.sqrt(np.maximum(0.01, mid * mid - (a * c - b * b)))
    x = 3.0 * np.sqrt(lam)
    return np.abs(x - np.round(x))[vis].min()


def _boundary_check(sc, proj, kept, culled):
    fw = run_oracle(sc, **proj)
    assert (fw["radii"][0, kept] > 0).all() and (fw["radii"][0, culled] == 0).all(), fw["radii"]
    assert _radius_margin(fw) > 1e-3
    for culling in ("gsplat", "tight"):
        hip = run_hip(sc, culling=culling, fw=fw, **proj)
        assert np.array_equal(hip["meta"]["radii"].cpu().numpy(), fw["radii"]), (hip["meta"]["radii"], fw["radii"])
        assert check_forward(hip, fw, lists=culling != "tight"), "no rounding flip by construction: the lists are the oracle's"
        check_backward(hip, fw)
        for i, g in enumerate(hip["grads"]):   # the culled Gaussians: exactly zero, in every tensor
            assert float(g[torch.as_tensor(culled, device=g.device)].abs().max()) == 0.0
            if i != 1:   # (an isotropic Gaussian does not feel its rotation: v_quats is zero for all of them)
                assert float(g[torch.as_tensor(kept, device=g.device)].reshape(len(kept), -1).abs().amax(1).min()) > 0.0
        assert float(hip["meta"]["means2d"].absgrad[0, culled].abs().max()) == 0.0
    return fw


def test_depth_cull_keeps_both_planes_and_drops_one_step_beyond():
    """`z < near || z > far` culls: both ends are inclusive."""
    sc = _boundary_scene()
    _boundary_check(sc, dict(near_plane=NEAR, far_plane=FAR), kept=[0, 2, 4, 5, 6, 7], culled=[1, 3])
    # the default planes keep all eight (so it was the planes that culled)
    fw = run_oracle(sc)
    assert (fw["radii"] > 0).all()
    assert np.array_equal(run_hip(sc, bwd=False)["meta"]["radii"].cpu().numpy(), fw["radii"])


def test_radius_cull_drops_a_radius_equal_to_radius_clip():
    """`radius <= radius_clip` culls: a Gaussian of integer radius r goes at radius_clip = r and stays at r - 0.5."""
    sc = _boundary_scene()
    proj = dict(near_plane=NEAR, far_plane=FAR)
    r_all = run_oracle(sc, **proj)["radii"][0]
    r = int(r_all[4])
    smaller, larger = [i for i in (0, 2, 4, 5, 6, 7) if 0 < r_all[i] <= r], [i for i in (0, 2, 5, 6, 7) if r_all[i] > r]
    assert 4 in smaller and len(larger) >= 2 and r >= 4, r_all
    _boundary_check(sc, dict(radius_clip=float(r), **proj), kept=larger, culled=smaller + [1, 3])
    below = [i for i in smaller if r_all[i] < r]
    _boundary_check(sc, dict(radius_clip=r - 0.5, **proj), kept=larger + [i for i in smaller if r_all[i] == r], culled=below + [1, 3])


# ---- c. view-matrix gradients on general poses -------------------------------------------------------------------------------
CAM_KINDS = ("sh3", "sh3_split_act", "sh4", "feat4")


@pytest.mark.parametrize("name", ["inside", "outside"])
@pytest.mark.parametrize("kind", CAM_KINDS)
def test_view_matrix_gradient_on_general_poses(kind, name):
    """tests/test_gpu_camgrad.py's parity of dL/d viewmats with fp64 autograd of the torch oracle (1e-3 per camera, all 16
    entries), three cameras: no R is symmetric, so a transposed R in the camera-centre term or in the SH direction Jacobian
    shows, and t has x and y components.  Everything else stays bit-identical with the call without camera gradients."""
    i = CAM_KINDS.index(kind)
    seed = 90 + 2 * i + (name == "outside")
    cams = cameras.general_cameras(3, W, H, cameras.SEED, cameras.CONFIGS[name]["centre_box"])
    sc, geo, cols, kw, act = CG._case(kind, 3, seed, cameras=cams)
    assert (int(sc["width"]), int(sc["height"])) == (W, H)
    D = cols[0].shape[-1] if kw["sh_degree"] is None else 3
    vc, va = CG._upstream(sc, act, D, seed=i)
    culling = CG.CULLING[(i + (name == "outside")) % 3]
    with_cam = CG._gpu(sc, geo, cols, kw, vc, va, True, culling)
    plain = CG._gpu(sc, geo, cols, kw, vc, va, False, culling)
    CG._assert_nothing_else_moves(with_cam, plain)
    ref = CG._oracle_v_viewmats_degree4(sc, act, vc, va) if kind == "sh4" else CG._oracle_v_viewmats(sc, cols, kw, act, vc, va)
    errs = CG._check_cameras(with_cam["v_viewmats"], ref)
    parity_log.record(v_viewmats_rel_err_per_camera={f"camera{c}": e for c, e in enumerate(errs)})


def test_translation_gradient_identity_on_a_general_rotation():
    """Degree-0 colours: every dependence on `means` and on t goes through p_c = A p + t, so v_viewmats[0,:3,3] = A sum_n v_means[n].
    The bound of the 1 M test (tests/test_gpu_camgrad.py): each fp32 v_means entry carries a rounding of 2^-24 relative, |A_ij| <= 1
    and the fp32 A is orthonormal to a few 2^-24, so |difference| <= 8 * 2^-24 * sum_n |v_means[n]|_1 per component.  There A = I;
    here A is a general rotation, and its transpose in either gradient fails."""
    from easy_gaussian_splatting_amd.rendering import rasterization
    d = dev()
    sc = cameras.general_scene(20_000, W, H, 1, cameras.SEED, cameras.CONFIGS["outside"]["centre_box"], sh_degree=0)
    t = {k: torch.from_numpy(v).to(d) for k, v in sc.items() if isinstance(v, np.ndarray)}
    means, V = t["means"].clone().requires_grad_(True), t["viewmats"].clone().requires_grad_(True)
    img, _, meta = rasterization(means, t["quats"], t["scales"], t["opacities"], t["shs"], V, t["Ks"], W, H, sh_degree=0, packed=False,
                                 backgrounds=t["backgrounds"], _camera_grads=True)
    vc = torch.randn(img.shape, generator=torch.Generator().manual_seed(2)).to(d)
    v_means, v_V = torch.autograd.grad((img * vc).sum(), (means, V))
    torch.cuda.synchronize()
    assert means.shape[0] % 256 != 0 and int((meta["radii"] > 0).sum()) > 5000
    A = V.detach()[0, :3, :3].double().cpu()
    assert float((A - A.T).abs().max()) > 0.05
    vm = v_means.double().cpu()
    want, got = A @ vm.sum(0), v_V[0, :3, 3].double().cpu()
    bound = 8 * 2.0 ** -24 * float(vm.abs().sum())
    wrong = A.T @ vm.sum(0)
    print(f"v_t {got.tolist()}  A sum v_means {want.tolist()}  |diff| {(got - want).abs().tolist()}  bound {bound:.4g}  "
          f"|A^T sum v_means - A sum v_means| {(wrong - want).abs().tolist()}")
    parity_log.record(translation_identity_diff=float((got - want).abs().max()), translation_identity_bound=bound)
    assert float((wrong - want).abs().max()) > 100 * bound, "the scene would not tell A from its transpose"
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= bound, ((got - want).abs().tolist(), bound)
    assert float(v_V[0, 3].abs().max()) == 0.0   # (no SH direction: nothing reaches the bottom row)


# ---- d. colour features of 1, 2 and 4 channels -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 4])
def test_channels_under_general_cameras(D):
    """tests/test_gpu_channels.py's forward and gradient parity against the fp64 torch oracle, two `inside` cameras, per-camera
    colours and a background."""
    C = 2
    sc = CH._scene(C, seed=50 + D)
    sc["viewmats"], sc["Ks"] = cameras.general_cameras(C, int(sc["width"]), int(sc["height"]), cameras.SEED, cameras.CONFIGS["inside"]["centre_box"])
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(D)
    colors = torch.randn((C, N, D), generator=g, dtype=torch.float64)
    bg = torch.rand((C, D), generator=g, dtype=torch.float64)
    razor = CH._razor(sc)
    assert razor.mean() < 0.05, razor.mean()
    vc, va = CH._upstream(sc, D, razor, seed=100 + D)
    img, alpha, meta, gh = CH.hip(sc, colors, bg, vc=vc, va=va)
    assert img.shape == (C, int(sc["height"]), int(sc["width"]), D) and gh["colors"].shape == colors.shape
    ref_img, ref_alpha, gr = CH.oracle(sc, lambda *a: colors, bg, vc, va)
    CH._check_fwd(img, alpha, ref_img, ref_alpha, razor)
    for k in CH.NAMES + ("colors", "absgrad"):
        CH._check_grad(k, gh[k], gr[k])


# ---- e. depth rounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("culling", ["gsplat", "tight", "gsplat_eager"])
def test_depth_rounds_from_inside_the_cloud(culling):
    """Inference in two depth rounds is the one-round image bit for bit (tests/test_gpu_rounds.py) when the depth range starts at
    the near plane and image-covering footprints sit in the front slab."""
    from easy_gaussian_splatting_amd import rendering
    d = dev()
    sc = cameras.general_scene(4000, 160, 96, 1, cameras.SEED, cameras.CONFIGS["inside"]["centre_box"])
    t = {k: torch.from_numpy(v).to(d) for k, v in sc.items() if isinstance(v, np.ndarray)}
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["shs"], t["viewmats"], t["Ks"], 160, 96)
    kw = dict(sh_degree=3, packed=False, backgrounds=t["backgrounds"], _tile_culling=culling)
    with torch.no_grad():
        rendering.reset_hints()
        for _ in range(2):   # (second call: capacities learnt from the first)
            img_a, al_a, meta_a = rendering.rasterization(*args, _rounds="off", **kw)
        rendering.reset_hints()
        n0 = rendering.stats["round_calls"]
        for _ in range(3):
            img_b, al_b, meta_b = rendering.rasterization(*args, _rounds="on", **kw)
        torch.cuda.synchronize()
        assert rendering.stats["round_calls"] == n0 + 3
        assert int(meta_a["radii"].max()) > 1000 and float(al_a.max()) > 0.9998
        assert torch.equal(img_a, img_b) and torch.equal(al_a, al_b)
        for k in ("radii", "means2d", "depths", "conics", "tiles_per_gauss", "isect_offsets", "flatten_ids", "isect_ids"):
            assert torch.equal(meta_a[k], meta_b[k]), k
    rendering.reset_hints()


def test_depth_rounds_from_inside_the_cloud_with_four_channels():
    sc = cameras.general_scene(4000, 160, 96, 1, cameras.SEED, cameras.CONFIGS["inside"]["centre_box"], sh_degree=0)
    colors = torch.randn((4000, 4), generator=torch.Generator().manual_seed(1))
    bg = torch.rand((1, 4), generator=torch.Generator().manual_seed(2))
    on = CH.hip(sc, colors, bg, grad=False, rounds="on")
    off = CH.hip(sc, colors, bg, grad=False, rounds="off")
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and float(off[1].max()) > 0.9998


# ---- f. captured step equals eager step while the camera changes -------------------------------------------------------------
def test_captured_step_equals_eager_step_over_general_cameras():
    """TrainStepGraph stages `w2c` and `K` into device buffers between replays: three cameras with roll, each with its own K
    (fx != fy, principal point off the centre), standing inside the cloud -- bit for bit the eager loop."""
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    Wt, Ht = 128, 96
    d, make, datas, gts = TG._setup(n=4000, W=Wt, H=Ht, n_views=3)
    V, Ks = cameras.general_cameras(3, Wt, Ht, cameras.SEED, cameras.CONFIGS["inside"]["centre_box"])
    for v in range(3):
        datas[v]["w2c"], datas[v]["K"] = torch.from_numpy(V[v]).to(d), torch.from_numpy(Ks[v]).to(d)
    assert not torch.equal(datas[0]["K"], datas[1]["K"]) and not torch.equal(datas[1]["K"], datas[2]["K"])
    (ma, oa), (mb, ob) = make(), make()
    lc = LossComputer(0.2, clamp_input=True)
    runner = TrainStepGraph(mb, ob, lc, datas[0], gts[0], check_every=2)
    for it in range(6):
        v = it % 3
        ma.update_learning_rate(it); mb.update_learning_rate(it)
        l_ref = TG._eager_step(ma, oa, lc, datas[v], gts[v])
        out = runner.step(datas[v], gts[v])
        runner.finish()
        assert torch.equal(out["loss3"], l_ref), it
        TG._assert_same(ma, oa, mb, ob, f"step {it}")
    rep = runner.report()
    assert rep["steps"] == 6 and rep["graph"] and rep["captures"] >= 1


# ---- g. view-parallel SH kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [3, 4])
def test_sh_grad_views_under_general_cameras(deg):
    """gs_sh_grad_views rebuilds each view's SH gradient from the camera centre of a general view matrix (tests/test_gpu_sh4.py's
    check against the dense projection backward, which test a. holds to the oracle)."""
    sc = cameras.general_scene(2500, 176, 112, 3, cameras.SEED, cameras.CONFIGS["inside"]["centre_box"], sh_degree=deg)
    SH4._sh_grad_views_check(sc, deg, split=deg == 3)


@pytest.mark.parametrize("deg", [3, 4])
def test_sh_adam_views_under_general_cameras(deg):
    """gs_sh_adam_views reads the view matrix out of each view's record: rotations with roll instead of the identity."""
    V, _ = cameras.general_cameras(2, 176, 112, cameras.SEED, cameras.CONFIGS["outside"]["centre_box"])
    SH4._sh_adam_views_check(deg, cams=torch.from_numpy(V))
