"""The viewer service (easy_gaussian_splatting_amd/viewer.py), host side: the declarations and refusals of the frame kernels'
entry points, `finish_frame` on CPU tensors against numpy statements written here, the SE(3) log / exp and the camera-path
interpolation, and the video export with stub renderers and writers.  Nothing here launches a kernel."""
import ctypes as ct
import re

import numpy as np
import pytest
import torch

from easy_gaussian_splatting_amd import viewer as V
from easy_gaussian_splatting_amd.checkpoint import CameraState
from easy_gaussian_splatting_amd.viewer import camera_interpolation, export_video, finish_frame, se3_exp, se3_log, write_ppm_frames


# ---- the C ABI ----

def test_the_entry_points_are_declared_and_refuse_bad_arguments_before_a_launch():
    from easy_gaussian_splatting_amd import _native as nat
    P, I, F = ct.c_void_p, ct.c_int, ct.c_float
    assert nat.SIGNATURES["gs_frame_workspace_floats"] == (ct.c_size_t, [I, I])
    assert nat.SIGNATURES["gs_frame_range"] == (ct.c_int, [P, I, I, I, P, P, F, P, P])
    assert nat.SIGNATURES["gs_frame_finish"] == (ct.c_int, [P, I, I, I, P, I, I, P, P, F, I, I, P])
    assert (nat.GS_FRAME_F32, nat.GS_FRAME_U8, nat.GS_FRAME_RGB, nat.GS_FRAME_DEPTH) == (0, 1, 0, 1)
    L = nat.lib()
    assert L.gs_version() >= 340
    raw = (ct.c_float * 16)()
    p = (ct.addressof(raw) + 15) & ~15   # 16-byte aligned, never dereferenced: every call below is refused first
    err = lambda: L.gs_last_error().decode()
    RGB, DEPTH, F32, U8 = nat.GS_FRAME_RGB, nat.GS_FRAME_DEPTH, nat.GS_FRAME_F32, nat.GS_FRAME_U8

    def finish(H=4, W=4, cin=3, render=p, mode=RGB, fmt=U8, alpha=None, rng=None, oH=None, oW=None, out=p):
        return L.gs_frame_finish(None, H, W, cin, render, mode, fmt, alpha, rng, 0.5, H if oH is None else oH, W if oW is None else oW, out)

    for kw in (dict(H=0), dict(W=0), dict(H=-3)):
        assert finish(**kw) == -1 and "size must be positive" in err(), kw
    for kw in (dict(oH=3), dict(oW=3)):
        assert finish(**kw) == -1 and "smaller than the render" in err(), kw
    for kw in (dict(cin=1), dict(cin=2), dict(cin=5), dict(cin=0)):
        assert finish(**kw) == -1 and "cin is 3 or 4" in err(), kw
    for kw in (dict(cin=3), dict(cin=2)):
        assert finish(mode=DEPTH, alpha=p, rng=p, **kw) == -1 and "cin is 1 or 4" in err(), kw
    assert finish(mode=2) == -1 and "unknown mode" in err()
    assert finish(mode=-1) == -1 and "unknown mode" in err()
    assert finish(fmt=2) == -1 and "unknown format" in err()
    for kw in (dict(render=None), dict(out=None), dict(mode=DEPTH, cin=4, alpha=None, rng=p), dict(mode=DEPTH, cin=1, alpha=p, rng=None)):
        assert finish(**kw) == -1 and "null pointer" in err(), kw
    assert finish(render=p + 4) == -1 and "16-byte aligned" in err()
    # byte counts past 31 bits: the render's (H * W * cin * 4) and the output's
    assert finish(H=16384, W=16384, cin=4) == -1 and "too large" in err()
    assert finish(H=4, W=4, fmt=F32, oH=20000, oW=20000) == -1 and "too large" in err()
    assert finish(H=4, W=4, fmt=U8, oH=30000, oW=30000) == -1 and "too large" in err()

    def rng(H=4, W=4, cin=4, render=p, alpha=p, ws=p, out=p):
        return L.gs_frame_range(None, H, W, cin, render, alpha, 0.5, ws, out)

    assert rng(H=0) == -1 and "size must be positive" in err()
    assert rng(W=-1) == -1 and "size must be positive" in err()
    for cin in (0, 2, 3, 5):
        assert rng(cin=cin) == -1 and "cin is 1 or 4" in err(), cin
    for kw in (dict(render=None), dict(alpha=None), dict(ws=None), dict(out=None)):
        assert rng(**kw) == -1 and "null pointer" in err(), kw
    assert rng(H=16384, W=16384, cin=4) == -1 and "too large" in err()
    # one {min, max} pair per launched block: 256 threads of four pixels each, 1024 blocks at the most
    assert L.gs_frame_workspace_floats(1, 1) == 2 and L.gs_frame_workspace_floats(32, 32) == 2
    assert L.gs_frame_workspace_floats(32, 33) == 4 and L.gs_frame_workspace_floats(1080, 1920) == 2 * 1024
    assert L.gs_frame_workspace_floats(0, 5) == 0 and L.gs_frame_workspace_floats(5, -1) == 0


def test_the_package_exports_the_viewer_service():
    import easy_gaussian_splatting_amd as pkg
    for name in ("FrameRenderer", "finish_frame", "camera_interpolation", "export_video", "viewer_render_func"):
        assert getattr(pkg, name) is getattr(V, name) and name in pkg.__all__


# ---- finish_frame on CPU tensors ----

def np_clamp(x):
    """clamp(x, 0, 1) with a NaN left a NaN and -0 made +0"""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.minimum(x, np.float32(1)), np.where(np.isnan(x), x, np.float32(0))).astype(np.float32)


def np_finish(render, mode, fmt, pad_to=None, alphas=None, rng=None, alpha_min=0.5):
    """The frame in numpy: every product and quotient a float32 operation of its own."""
    render = np.asarray(render, dtype=np.float32)
    H, W = render.shape[:2]
    if mode == "rgb":
        x = render[..., :3]
    else:
        d, a = render[..., -1], np.asarray(alphas, dtype=np.float32).reshape(H, W)
        lo, hi = np.float32(rng[0]), np.float32(rng[1])
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.zeros_like(d) if hi == lo else ((d - lo) / (hi - lo)).astype(np.float32)
        g = np.where(a >= np.float32(alpha_min), np.float32(1) - np_clamp(t), np.float32(0)).astype(np.float32)
        x = np.repeat(g[..., None], 3, axis=2)
    c = np_clamp(x)
    if fmt == "uint8":
        c = np.floor(np.where(np.isnan(c), np.float32(0), c) * np.float32(255)).astype(np.uint8)
    oH, oW = (H, W) if pad_to is None else pad_to
    out = np.zeros((oH, oW, 3), dtype=c.dtype)
    out[:H, :W] = c
    return out


def np_range(render, alphas, alpha_min=0.5):
    d, a = np.asarray(render)[..., -1], np.asarray(alphas).reshape(render.shape[:2])
    m = (a >= alpha_min) & ~np.isnan(d)
    return (np.float32(d[m].min()), np.float32(d[m].max())) if m.any() else (np.float32(0), np.float32(0))


def planted_values():
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    edge = np.array([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan],
                    dtype=np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)), edge])


def noisy_render(H, W, C, seed, plant=True):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 1.5, (H, W, C)).astype(np.float32)
    if plant:   # into the displayed channels; an image too small for all of them gets a seeded choice
        pv = rng.permutation(planted_values())
        pix = x.reshape(-1, C)[:, :3]
        idx = rng.permutation(pix.size)[:pv.size]
        pix[idx // 3, idx % 3] = pv[:idx.size]
    return x


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


PADS = [None, (0, 0), (1, 0), (0, 3), (2, 5)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fmt", ["uint8", "float32"])
@pytest.mark.parametrize("C", [3, 4])
def test_finish_frame_rgb_on_cpu_tensors_equals_numpy(C, fmt, pad):
    H, W = 17, 33
    x = noisy_render(H, W, C, 11)
    pad_to = None if pad is None else (H + pad[0], W + pad[1])
    got = finish_frame(torch.from_numpy(x), mode="rgb", fmt=fmt, pad_to=pad_to)
    want = np_finish(x, "rgb", fmt, pad_to)
    assert got.dtype == (torch.uint8 if fmt == "uint8" else torch.float32) and same_bits(got.numpy(), want)
    if fmt == "float32":
        assert np.isnan(want).sum() == 1 and not np.signbit(want[want == 0]).any()
    else:
        assert set(np.unique(want)) == set(range(256))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fmt", ["uint8", "float32"])
@pytest.mark.parametrize("C", [1, 4])
def test_finish_frame_depth_on_cpu_tensors_equals_numpy(C, fmt, pad):
    H, W = 17, 33
    rng = np.random.default_rng(5)
    x = noisy_render(H, W, C, 12, plant=False)
    x[..., -1] = rng.uniform(1.0, 9.0, (H, W)).astype(np.float32)
    x[3, 4, -1] = np.nan
    alphas = rng.uniform(0, 1, (H, W)).astype(np.float32)
    pad_to = None if pad is None else (H + pad[0], W + pad[1])
    lo, hi = np_range(x, alphas)
    a_t = torch.from_numpy(alphas)
    got = finish_frame(torch.from_numpy(x), mode="depth", fmt=fmt, pad_to=pad_to, alphas=a_t if C == 1 else a_t[..., None])
    want = np_finish(x, "depth", fmt, pad_to, alphas, (lo, hi))
    assert same_bits(got.numpy(), want)
    covered = alphas >= 0.5
    assert (want[:H, :W][~covered] == 0).all() and want[:H, :W][covered].max() == (255 if fmt == "uint8" else 1.0)
    # a given range, as numbers and as a tensor; a degenerate one gives white where covered
    for r in ((2.0, 6.5), torch.tensor([2.0, 6.5])):
        got = finish_frame(torch.from_numpy(x), mode="depth", fmt=fmt, pad_to=pad_to, alphas=a_t, depth_range=r)
        assert same_bits(got.numpy(), np_finish(x, "depth", fmt, pad_to, alphas, (2.0, 6.5)))
    flat = finish_frame(torch.from_numpy(x), mode="depth", fmt="uint8", alphas=a_t, depth_range=(3.0, 3.0)).numpy()
    assert (flat[covered] == 255).all() and (flat[~covered] == 0).all()
    none = finish_frame(torch.from_numpy(x), mode="depth", fmt="uint8", alphas=torch.zeros(H, W)).numpy()
    assert not none.any()


def test_finish_frame_out_and_refusals():
    x = torch.rand(5, 7, 3)
    out = torch.full((6, 9, 3), 0xA5, dtype=torch.uint8)
    assert finish_frame(x, pad_to=(6, 9), out=out) is out and same_bits(out.numpy(), np_finish(x.numpy(), "rgb", "uint8", (6, 9)))
    with pytest.raises(ValueError, match="mode"):
        finish_frame(x, mode="normal")
    with pytest.raises(ValueError, match="fmt"):
        finish_frame(x, fmt="float16")
    with pytest.raises(ValueError, match=r"\[H, W, C\]"):
        finish_frame(x[0])
    with pytest.raises(ValueError, match="3 or 4 channels"):
        finish_frame(torch.rand(5, 7, 1))
    with pytest.raises(ValueError, match="1 or 4 channels"):
        finish_frame(x, mode="depth", alphas=torch.rand(5, 7))
    with pytest.raises(ValueError, match="smaller than the render"):
        finish_frame(x, pad_to=(4, 7))
    with pytest.raises(ValueError, match="needs alphas"):
        finish_frame(torch.rand(5, 7, 1), mode="depth")
    with pytest.raises(ValueError, match="alphas has shape"):
        finish_frame(torch.rand(5, 7, 1), mode="depth", alphas=torch.rand(7, 5))
    with pytest.raises(ValueError, match="out must be"):
        finish_frame(x, out=torch.zeros(5, 7, 3))   # float32 where uint8 is asked for
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.FrameRenderer(torch.nn.Linear(1, 1))


def test_aspect_size_is_the_references_arithmetic():
    assert V.aspect_size(112, 176, None) == (112, 176)
    assert V.aspect_size(112, 176, 176 / 112) == (112, 176)
    assert V.aspect_size(112, 176, 2.0) == (112, 224) and V.aspect_size(112, 176, 1.0) == (176, 176)
    assert V.aspect_size(48, 64, 1.77) == (48, int(48 * 1.77)) and V.aspect_size(48, 64, 0.9) == (int(64 / 0.9), 64)


# ---- SE(3) and the camera path ----

def rotation(axis, theta):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    Wm = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(theta) * Wm + (1 - np.cos(theta)) * (Wm @ Wm)


def rigid(rng, theta, scale=3.0):
    T = np.eye(4)
    T[:3, :3] = rotation(rng.standard_normal(3), theta)
    T[:3, 3] = scale * rng.standard_normal(3)
    return T


def test_exp_of_log_is_the_identity_on_rigid_transforms():
    rng = np.random.default_rng(2024)
    thetas = [0.0, 1e-9, np.pi - 1e-6, 1e-5, V.SMALL_ANGLE - 1e-9, V.SMALL_ANGLE + 1e-9] + list(rng.uniform(0, np.pi, 193))
    transforms = [rigid(rng, t) for t in thetas]
    pure = np.eye(4)
    pure[:3, 3] = [1.5, -2.0, 0.25]
    transforms.append(pure)
    assert len(transforms) == 200
    for T in transforms:
        assert np.abs(se3_exp(se3_log(T)) - T).max() <= 1e-12
    assert np.array_equal(se3_log(pure), [1.5, -2.0, 0.25, 0, 0, 0]) and np.array_equal(se3_exp(np.zeros(6)), np.eye(4))
    # the angle comes back: the rotation vector's length, also next to pi
    for t in (1e-9, 0.1, 2.0, np.pi - 1e-6):
        assert abs(np.linalg.norm(se3_log(rigid(rng, t))[3:]) - t) <= 1e-12


def keys(rng, n, theta_max=2.0, size=(176, 112)):
    out = []
    for i in range(n):
        c2w = rigid(rng, rng.uniform(0.05, theta_max), 2.0)
        K = np.array([[200.0 + i, 0, size[0] / 2], [0, 210.0 + i, size[1] / 2], [0, 0, 1]], dtype=np.float32)
        out.append(CameraState(np.linalg.inv(c2w), K, size[0] + i, size[1] + i))
    return out


def segment_shares(cams, total):
    c = [np.linalg.inv(cs.w2c)[:3, 3] for cs in cams]
    d = np.array([np.linalg.norm(c[i] - c[i + 1]) for i in range(len(cams) - 1)])
    return [int(v) for v in d / d.sum() * total]


def test_the_camera_path_counts_frames_ends_on_the_keys_and_moves_on_constant_screws():
    rng = np.random.default_rng(7)
    cams = keys(rng, 5)
    # two keys almost on top of each other: their segment's share truncates to 0 and contributes its end key alone
    near = np.linalg.inv(cams[2].w2c)
    near[:3, 3] += 1e-4
    cams.insert(3, CameraState(np.linalg.inv(near), cams[2].K, 99, 98))
    duration, fps = 2.0, 30.0
    shares = segment_shares(cams, int(duration * fps))
    assert 0 in shares
    path = camera_interpolation(cams, duration, fps)
    assert len(path) == 1 + sum(max(s, 1) for s in shares)
    assert path[0] is cams[0]
    at = 1
    for i, s in enumerate(shares):
        seg = path[at:at + max(s, 1)]
        at += max(s, 1)
        assert np.abs(seg[-1].w2c - cams[i + 1].w2c).max() <= 1e-12   # (c) the segment ends on the next key
        if s == 0:
            continue
        c2w = [np.linalg.inv(cams[i].w2c)] + [np.linalg.inv(cs.w2c) for cs in seg]
        steps = [np.linalg.inv(c2w[j]) @ c2w[j + 1] for j in range(s)]
        for st in steps[1:]:
            assert np.abs(st - steps[0]).max() <= 1e-10               # (d) one screw step, again and again
    assert at == len(path)
    for cs in path[1:]:                                               # (e) the first key's intrinsics and size
        assert np.array_equal(cs.K, cams[0].K) and (cs.width, cs.height) == (cams[0].width, cams[0].height)
        assert cs.K is not cams[0].K
    # fewer frames than keys: the keys as they are
    assert camera_interpolation(cams, 0.1, 30.0) is cams


def test_the_camera_path_equals_scipys_matrix_exponential():
    sl = pytest.importorskip("scipy.linalg")
    rng = np.random.default_rng(8)
    cams = keys(rng, 4, theta_max=np.deg2rad(179.0) / 2)   # (relative rotations stay below 179 degrees)
    shares = segment_shares(cams, 40)
    path = camera_interpolation(cams, 2.0, 20.0)
    at = 1
    for i, s in enumerate(shares):
        start, end = np.linalg.inv(cams[i].w2c), np.linalg.inv(cams[i + 1].w2c)
        rel = np.linalg.inv(start) @ end
        angle = np.arccos(np.clip((np.trace(rel[:3, :3]) - 1) / 2, -1, 1))
        assert s > 0 and angle < np.deg2rad(179.0)
        log = sl.logm(rel)
        for j in range(1, s + 1):
            want = start @ sl.expm(log * j / s)
            assert np.abs(np.linalg.inv(path[at].w2c) - np.real(want)).max() <= 1e-9
            at += 1
    assert at == len(path)


# ---- export_video ----

def stub_render(cs):
    """an image that depends on the camera, with values on both sides of the codes' edges"""
    rng = np.random.default_rng(int(abs(cs.w2c[0, 3]) * 1e6) % (2 ** 31))
    return rng.uniform(0, 1, (cs.height, cs.width, 3)).astype(np.float32)


def test_export_video_hands_floor_255_frames_of_the_whole_path_to_the_writer(tmp_path, capsys):
    rng = np.random.default_rng(3)
    cams = keys(rng, 3, size=(12, 8))
    got = {}

    def writer(path, frames, fps):
        assert not isinstance(frames, (list, tuple))   # consumed as they arrive
        got["path"], got["fps"] = path, fps
        got["frames"] = [f.copy() for f in frames]

    out = export_video(stub_render, cams, 1.0, 12.0, tmp_path / "videos", writer=writer)
    path = camera_interpolation(cams, 1.0, 12.0)
    assert out == got["path"] and got["fps"] == 12.0 and out.parent == tmp_path / "videos" and out.parent.is_dir()
    assert re.fullmatch(r"\d\d-\d\d_\d\d-\d\d-\d\d\.mp4", out.name)
    assert len(got["frames"]) == len(path) > len(cams)
    for f, cs in zip(got["frames"], path):
        assert f.dtype == np.uint8 and f.shape == (cams[0].height, cams[0].width, 3)
        assert np.array_equal(f, np.floor(stub_render(cs) * 255.0).astype(np.uint8))
    assert f"{len(path)} frames written to {out}" in capsys.readouterr().out


@pytest.mark.parametrize("n", [0, 1])
def test_export_video_refuses_fewer_than_two_key_cameras(tmp_path, capsys, n):
    cams = keys(np.random.default_rng(4), n, size=(12, 8))
    called = []
    assert export_video(stub_render, cams, 1.0, 12.0, tmp_path / "v", writer=lambda *a: called.append(a)) is None
    assert not called and not (tmp_path / "v").exists() and "refused" in capsys.readouterr().out


def test_the_ppm_writer_reads_back_to_the_same_bytes(tmp_path):
    rng = np.random.default_rng(5)
    cams = keys(rng, 2, size=(13, 7))
    out = export_video(stub_render, cams, 0.5, 10.0, tmp_path, writer=write_ppm_frames)
    path = camera_interpolation(cams, 0.5, 10.0)
    assert out.is_dir() and re.fullmatch(r"\d\d-\d\d_\d\d-\d\d-\d\d", out.name)
    files = sorted(p.name for p in out.glob("*.ppm"))
    assert files == [f"frame_{i:05d}.ppm" for i in range(len(path))]
    for i, cs in enumerate(path):
        raw = (out / f"frame_{i:05d}.ppm").read_bytes()
        head = b"P6\n%d %d\n255\n" % (cams[0].width, cams[0].height)
        assert raw.startswith(head)
        img = np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(cams[0].height, cams[0].width, 3)
        assert np.array_equal(img, np.floor(stub_render(cs) * 255.0).astype(np.uint8))
    readme = (out / "README.txt").read_text()
    assert readme.count("\n") == 1 and readme.startswith("ffmpeg -framerate 10 -i frame_%05d.ppm") and readme.rstrip().endswith(out.name + ".mp4")
