"""csrc/gs_normals.h built with the host compiler -- the device's own text -- held to float64 restatements (tests/normals_ref.py), to
torch float64 autograd and to analytic surfaces: no GPU.

Gaussian normals: outside the *razor* Gaussians (normals_ref.gauss64: the two smallest scales within a relative 1e-6, or the facing
dot product within its own rounding of 0 -- decided by the float64 run alone, at most 2 % of the case) every component is within the
bound gauss64 derives; v_quats within gauss_vjp64's.  Depth normals, the loss value, v_Nb and v_d: within loss64's per-element
bounds of float64 autograd of `normal_consistency_loss(fused=False)`, which central differences validate once.  Every test prints
its worst error / bound ratio."""
import os
import subprocess

import numpy as np
import pytest
import torch

import normals_ref as NR
from easy_gaussian_splatting_amd import normals as NM


@pytest.fixture(scope="module")
def nm(tmp_path_factory):
    return NR.host_lib(tmp_path_factory.mktemp("normals"))


def _worst(err, bound):
    """the largest err / bound over the elements with a bound; an element without one must have no error"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert (err[bound == 0] == 0).all()
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---- the normal of a Gaussian ----

def test_axis_is_the_smallest_scale_and_the_lowest_index_wins_a_tie(nm):
    assert nm.nm_axis(1.0, 2.0, 3.0) == 0 and nm.nm_axis(2.0, 1.0, 3.0) == 1 and nm.nm_axis(3.0, 2.0, 1.0) == 2
    assert nm.nm_axis(1.0, 1.0, 2.0) == 0 and nm.nm_axis(2.0, 1.0, 1.0) == 1 and nm.nm_axis(1.0, 2.0, 1.0) == 0 and nm.nm_axis(1.0, 1.0, 1.0) == 0
    assert nm.nm_axis(-3.0, -4.0, -3.5) == 1   # (log-scales: the order alone)
    rng = np.random.default_rng(0)
    s = rng.normal(size=(200, 3)).astype(np.float32)
    assert [nm.nm_axis(*map(float, r)) for r in s] == np.argmin(s, 1).tolist() == np.argmin(np.exp(s.astype(np.float64)), 1).tolist()


@pytest.mark.parametrize("N,C,seed", ((2000, 2, 1), (257, 1, 2)))
def test_gaussian_normals_match_float64_outside_the_razor_cases(nm, N, C, seed):
    case = NR.gauss_case(N, C, seed)
    ref = NR.gauss64(case)
    got = NR.host_gauss_fwd(nm, case)
    share = ref["razor"].mean()
    ok = ~ref["razor"]
    ratio = _worst(np.abs(got - ref["normals"])[ok], ref["bound"][ok])
    qn = np.linalg.norm(case["quats"], axis=1)
    print(f"[normals host] N {N} C {C}: razor share {share:.4f}, flipped {ref['flipped'].mean():.3f}, |q| in [{qn.min():.3g}, {qn.max():.3g}], "
          f"axes {np.bincount(ref['k'], minlength=3).tolist()}, worst err / bound {ratio:.3f} (bound up to {ref['bound'].max():.3g})")
    assert share <= 0.02
    assert ref["flipped"][ok].any() and (~ref["flipped"][ok]).any()            # the flip happens, in both directions
    assert (np.bincount(ref["k"], minlength=3) > 0).all()
    assert qn.min() < 0.2 and qn.max() > 5.0
    assert ratio <= 1.0
    assert np.abs(np.linalg.norm(got, axis=-1) - 1).max() <= 64 * NR.U
    # facing the camera: dot(n_c, p_c) <= 0 outside the razor cases
    vm = case["viewmats"].astype(np.float64)
    pc = np.einsum("cij,nj->cni", vm[:, :3, :3], case["means"].astype(np.float64)) + vm[:, None, :3, 3]
    assert ((got * pc).sum(-1)[ok] <= 0).all()


def test_activated_and_raw_scales_give_the_same_normals(nm):
    case = NR.gauss_case(300, 1, 3)
    raw = NR.host_gauss_fwd(nm, case)
    act = NR.host_gauss_fwd(nm, dict(case, scales=np.exp(case["scales"].astype(np.float64)).astype(np.float32)))
    same = np.argmin(np.exp(case["scales"].astype(np.float64)).astype(np.float32), 1) == np.argmin(case["scales"], 1)   # (exp may round two to a tie)
    assert same.mean() > 0.99 and raw[:, same].tobytes() == act[:, same].tobytes()


@pytest.mark.parametrize("N,C,seed", ((500, 2, 4), (257, 1, 5)))
def test_v_quats_match_float64_autograd(nm, N, C, seed):
    case = NR.gauss_case(N, C, seed)
    v = np.random.default_rng(seed).normal(size=(C, N, 3)).astype(np.float32)
    fw = NR.gauss64(case)
    ok = ~fw["razor"].any(0)
    ref, bound = NR.gauss_vjp64(case, v)
    got = NR.host_gauss_bwd(nm, case, v)
    ratio = _worst(np.abs(got - ref)[ok], bound[ok])
    print(f"[normals host] v_quats N {N} C {C}: worst err / bound {ratio:.3f}, |v_q| up to {np.abs(ref).max():.3g}, razor {1 - ok.mean():.4f}")
    assert (1 - ok.mean()) <= 0.02 and ratio <= 1.0
    # the gradient is tangent to the quaternion: scaling q does not move the normal
    assert np.abs((got * case["quats"]).sum(1))[ok].max() <= 64 * NR.U * np.abs(got * case["quats"]).sum(1).max()


# ---- depth normals of analytic surfaces ----

def _depth_frame(d, K, alphas=None):
    H, W = d.shape
    r = np.zeros((H, W, 4), np.float32)
    r[..., 3] = d
    return dict(render4=r, alphas=np.ones((H, W), np.float32) if alphas is None else alphas, K=K, mask=None, min_alpha=0.5)


def test_a_tilted_plane_has_its_own_normal(nm):
    H, W = 23, 31
    K = NR.camera(H, W)
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    d = NR.plane_frame(H, W, n, n @ np.array([0.0, 0.0, 2.5]), K)
    frame = _depth_frame(d, K)
    got = NR.host_loss(nm, frame)["depth_normals"]
    ref = NR.loss64(frame)
    assert ref["valid"][1:-1, 1:-1].all() and not ref["valid"][0].any() and not ref["valid"][:, -1].any()
    # the float64 restatement on the exact (float64) depth is the plane's normal; on the float32 depth map the bound holds:
    # the depth's own rounding U |d| enters A and B like a rounding of P
    exact = NM.depth_to_normal(torch.tensor(d), torch.ones(H, W, dtype=torch.float64), torch.tensor(K.astype(np.float64)), fused=False).numpy()
    assert np.abs(exact[1:-1, 1:-1] - n).max() <= 1e-9
    err = np.abs(got - ref["depth_normals"])
    ratio = _worst(err, ref["dn_bound"])
    print(f"[normals host] plane: worst err / bound {ratio:.3f}; against the plane's own normal {np.abs(got[1:-1, 1:-1] - n).max():.3g}")
    assert ratio <= 1.0
    assert (got[0] == 0).all() and (got[-1] == 0).all() and (got[:, 0] == 0).all() and (got[:, -1] == 0).all()
    front = NR.host_loss(nm, _depth_frame(np.full((5, 7), 1.5), NR.camera(5, 7)))["depth_normals"]
    assert np.abs(front[1:-1, 1:-1] - np.array([0.0, 0.0, -1.0])).max() <= 8 * NR.U


def test_a_sphere_has_its_radial_normals(nm):
    """Central differences over a curved surface: the chord between the two neighbours is the tangent at the middle of their arc,
    which lies (s2 - s1) / 2 from the pixel's own point, s1, s2 the arcs to the neighbours.  With s <= p / cos(theta) the arc over
    one pixel (p = d / f its footprint, theta the angle of incidence) and |s2 - s1| <= 2 s^2 tan(theta) / R, the normal turns by at
    most (s / R)^2 tan(theta) per direction; both directions: twice that."""
    H, W, R = 48, 64, 1.0
    K = NR.camera(H, W)
    c = np.array([0.1, -0.05, 3.0])
    d, n = NR.sphere_frame(H, W, c, R, K)
    frame = _depth_frame(d, K)
    got = NR.host_loss(nm, frame)["depth_normals"].astype(np.float64)
    ref = NR.loss64(frame)
    assert _worst(np.abs(got - ref["depth_normals"]), ref["dn_bound"]) <= 1.0
    Kd = K.astype(np.float64)
    ray = np.stack(np.broadcast_arrays(((np.arange(W) + 0.5) - Kd[0, 2])[None, :] / Kd[0, 0], ((np.arange(H) + 0.5) - Kd[1, 2])[:, None] / Kd[1, 1],
                                       np.ones((H, W))), -1)
    cos = -(n * ray).sum(-1) / np.linalg.norm(ray, axis=-1)
    sel = ref["valid"] & (cos >= 0.5)
    s = (d / min(Kd[0, 0], Kd[1, 1])) / np.maximum(cos, 0.5)
    bound = 2 * (s / R) ** 2 * np.sqrt(1 - cos ** 2) / np.maximum(cos, 0.5) + 1e-5
    err = np.linalg.norm(got - n, axis=-1)
    print(f"[normals host] sphere: {int(sel.sum())} pixels, worst |n_d - n| {err[sel].max():.3g}, worst err / bound {(err[sel] / bound[sel]).max():.3f}")
    assert sel.sum() > 200 and (err[sel] <= bound[sel]).all()
    assert (got[~ref["valid"]] == 0).all() and (d == 0).sum() > 100   # the rays that miss have no depth: no normal there or next to them


# ---- the loss and its gradients ----

def test_the_torch_expression_is_validated_by_central_differences():
    frame = NR.frame_case(7, 9, 21)
    r0 = frame["render4"].astype(np.float64)
    _, grad = NR.loss_autograd64(frame)
    ref = NR.loss64(frame)
    assert ref["valid"].sum() >= 5
    h, worst = 1e-6, 0.0
    for (y, x, k) in [(y, x, k) for y in range(7) for x in range(9) for k in range(4)]:
        if not np.isfinite(r0[y, x, k]) or (k == 3 and not r0[y, x, 3] > 0):
            continue
        rp, rm = r0.copy(), r0.copy()
        rp[y, x, k] += h
        rm[y, x, k] -= h
        worst = max(worst, abs((_value64(frame, rp) - _value64(frame, rm)) / (2 * h) - grad[y, x, k]))
    print(f"[normals host] central differences: worst |fd - autograd| {worst:.3g}, |grad| up to {np.abs(grad).max():.3g}")
    assert worst <= 1e-6 * max(1.0, np.abs(grad).max())


def _value64(frame, r):
    return float(NM.normal_consistency_loss(torch.tensor(r), torch.tensor(frame["alphas"].astype(np.float64)), torch.tensor(frame["K"].astype(np.float64)),
                                            mask=torch.tensor(frame["mask"].astype(np.float64)), min_alpha=float(np.float32(frame["min_alpha"])), fused=False))


FRAMES = ((37, 53, 31), (3, 3, 32), (9, 65, 33), (17, 127, 34))


@pytest.mark.parametrize("H,W,seed", FRAMES)
@pytest.mark.parametrize("detach", (False, True))
def test_loss_and_gradients_match_float64_autograd(nm, H, W, seed, detach):
    frame = NR.frame_case(H, W, seed, holes=H > 3, bad_depths=H > 3, mask=H > 3)
    v_loss = 0.7
    ref = NR.loss64(frame, detach_depth=detach, v_loss=v_loss)
    value, grad = NR.loss_autograd64(frame, detach_depth=detach, v_loss=v_loss)
    got = NR.host_loss(nm, frame, detach_depth=detach, v_loss=v_loss)
    # the explicit float64 chain of normals_ref is the autograd of the torch expression
    assert abs(ref["value"] - value) <= 1e-12 * max(1.0, abs(value))
    assert np.abs(ref["v_render4"] - grad).max() <= 1e-9 * max(1e-30, np.abs(grad).max())
    rv = abs(float(got["value"]) - value) / ref["value_bound"]
    rn = _worst(np.abs(got["depth_normals"] - ref["depth_normals"]), ref["dn_bound"])
    rg = _worst(np.abs(got["v_render4"] - grad)[..., :3], ref["v_bound"][..., :3])
    rd = _worst(np.abs(got["v_render4"] - grad)[..., 3], ref["v_bound"][..., 3])
    print(f"[normals host] {H}x{W} detach {detach}: {int(ref['valid'].sum())} valid of {H * W}, counted {ref['w'].sum():.0f}, min |c| {ref['min_len']:.3g}, "
          f"value {value:.6f} err / bound {rv:.3f}; n_d {rn:.3f}; v_Nb {rg:.3f}; v_d {rd:.3f} (|v_d| up to {np.abs(grad[..., 3]).max():.3g}, "
          f"bound up to {ref['v_bound'][..., 3].max():.3g})")
    assert ref["valid"].sum() >= 1 and (H <= 3 or 0 < ref["w"].sum() < ref["valid"].sum() < (H - 2) * (W - 2))
    assert rv <= 1.0 and rn <= 1.0 and rg <= 1.0 and rd <= 1.0
    assert float(got["sums"][1]) == ref["w"].sum()                 # the same pixels count
    if detach:
        assert not got["v_render4"][..., 3].view(np.uint32).any()
    else:
        assert np.abs(grad[..., 3]).max() > 0
        assert got["v_render4"][..., 3].any()


def test_detached_depth_keeps_the_normal_channels_bits(nm):
    frame = NR.frame_case(37, 53, 31)
    a, b = NR.host_loss(nm, frame)["v_render4"], NR.host_loss(nm, frame, detach_depth=True)["v_render4"]
    assert a[..., :3].tobytes() == b[..., :3].tobytes() and a[..., 3].any() and not b[..., 3].view(np.uint32).any()


def test_a_lone_centre_sends_to_its_four_neighbours_only(nm):
    frame = NR.frame_case(9, 9, 41, holes=False, mask=False, bad_depths=False)
    al = np.zeros((9, 9), np.float32)
    for y, x in ((4, 4), (3, 4), (5, 4), (4, 3), (4, 5)):
        al[y, x] = 1.0
    frame["alphas"] = al
    got = NR.host_loss(nm, frame)
    assert float(got["sums"][1]) == 1.0 and float(got["inv_w"]) == 1.0
    nz = np.argwhere(got["v_render4"][..., 3] != 0).tolist()
    assert nz == [[3, 4], [4, 3], [4, 5], [5, 4]]
    assert np.argwhere(got["v_render4"][..., :3].any(-1)).tolist() == [[4, 4]]
    assert np.argwhere(got["depth_normals"].any(-1)).tolist() == [[4, 4]]


@pytest.mark.parametrize("kind", ("H2", "W1", "alpha", "mask", "depth"))
def test_a_frame_with_no_valid_pixel_gives_exact_zeros(nm, kind):
    H, W = {"H2": (2, 40), "W1": (12, 1)}.get(kind, (12, 40))
    frame = NR.frame_case(H, W, 51)
    if kind == "alpha":
        frame["alphas"] = np.minimum(frame["alphas"], np.float32(0.49))
    elif kind == "mask":
        frame["mask"] = np.ones((H, W), np.float32)
    elif kind == "depth":
        frame["render4"][..., 3] = np.where(np.arange(W)[None, :] % 2 == 0, np.nan, -1.0)
    got = NR.host_loss(nm, frame)
    assert got["value"].tobytes() == np.float32(0).tobytes() and got["inv_w"].tobytes() == np.float32(0).tobytes()
    assert not got["v_render4"].view(np.uint32).any()
    value, grad = NR.loss_autograd64(frame)
    assert value == 0.0 and not grad.any()
    if kind != "mask":
        assert not got["depth_normals"].view(np.uint32).any()
    else:
        assert got["depth_normals"].any()   # depth_to_normal leaves the mask out


def test_every_valid_pixel_of_the_border_case_has_a_neighbour_in_another_tile(nm):
    frame = NR.border_case(24, 130, 61)
    ref = NR.loss64(frame)
    y, x = np.nonzero(ref["valid"])
    assert len(y) > 20
    assert ((x % NR.TILE_W == 0) | (x % NR.TILE_W == NR.TILE_W - 1) | (y % NR.TILE_H == 0) | (y % NR.TILE_H == NR.TILE_H - 1)).all()
    got = NR.host_loss(nm, frame)
    value, grad = NR.loss_autograd64(frame)
    assert abs(float(got["value"]) - value) <= ref["value_bound"]
    assert _worst(np.abs(got["v_render4"] - grad), ref["v_bound"]) <= 1.0


# ---- the Python surface ----

def test_torch_form_runs_on_any_dtype_and_refuses_what_does_not_fit():
    frame = NR.frame_case(12, 15, 71)
    r, a, K, m = (torch.tensor(frame[k]) for k in ("render4", "alphas", "K", "mask"))
    v32 = NM.normal_consistency_loss(r, a, K, mask=m, fused=False)
    v64 = NM.normal_consistency_loss(r.double(), a.double(), K.double(), mask=m.double(), fused=False)
    assert v32.dtype == torch.float32 and v32.dim() == 0 and abs(float(v32) - float(v64)) <= 1e-4
    dn = NM.depth_to_normal(r[..., 3], a, K, fused=False)
    assert tuple(dn.shape) == (12, 15, 3) and NR.loss64(frame, with_mask=False)["valid"].tolist() == (dn.abs().sum(-1) > 0).tolist()
    with pytest.raises(ValueError):
        NM.normal_consistency_loss(r, a, K, fused=True)                       # CPU tensors on the fused path
    with pytest.raises(ValueError):
        NM.normal_consistency_loss(r[..., :3], a, K, fused=False)
    with pytest.raises(ValueError):
        NM.normal_consistency_loss(r, a[:5], K, fused=False)
    with pytest.raises(ValueError):
        NM.normal_consistency_loss(r, a, K, mask=m[:, :3], fused=False)
    with pytest.raises(ValueError):
        NM.depth_to_normal(r[..., 3], a, K, fused=True)
    with pytest.raises(NotImplementedError):
        NM.gaussian_normals(torch.zeros(4, 3), torch.ones(4, 4), torch.zeros(4, 3), torch.eye(4)[None].requires_grad_(True))
    with pytest.raises(NotImplementedError):
        NM.gaussian_normals(torch.zeros(4, 3), torch.ones(4, 4), torch.zeros(4, 3), torch.eye(4)[None])    # no CPU fallback
    with pytest.raises(NotImplementedError):
        NM.render_normals(None, {"camera_model": "fisheye"})
    import easy_gaussian_splatting_amd as E
    assert E.normal_consistency_loss is NM.normal_consistency_loss and E.render_normals is NM.render_normals
    assert E.gaussian_normals is NM.gaussian_normals and E.depth_to_normal is NM.depth_to_normal


# ---- the sanitizers ----

def test_host_build_under_asan_ubsan(tmp_path):
    """tests/hostmath/normals_san.cpp: a stand-alone program over exact-size heap buffers, nothing preloaded anywhere"""
    exe = str(tmp_path / "normals_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(NR.HERE, "hostmath", "normals_san.cpp")], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, f"{p.stdout[-2000:]}\n{p.stderr[-6000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-6000:]
    assert "sanitizer leg ok" in p.stdout and p.stdout.count("checksum") == 11
