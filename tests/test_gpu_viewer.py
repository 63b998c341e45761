"""The viewer service on the device: gs_frame_finish / gs_frame_range (csrc/gs_frame.hip) and the FrameRenderer built on them.

Colour frames are held to the numpy statements of tests/test_viewer_host.py BIT FOR BIT in both formats: the float32 frame is a
clamp, the uint8 frame one rounded float32 product and a floor, so there is no tolerance to give.  The depth grey has one float32
division whose last bit numpy may round differently: uint8 greys within one code at every pixel, float32 greys within 2^-23 (t
lies in [0, 1], where an ulp is at most 2^-24; 1 - t rounds once more).  The shapes are the smallest at which the kernel's paths
differ: one pixel, fewer pixels than a four-pixel group, rows that are no multiple of four, several blocks."""
import threading
import time

import numpy as np
import pytest
import torch

import test_viewer_host as TH
from easy_gaussian_splatting_amd import viewer as V
from easy_gaussian_splatting_amd.checkpoint import CameraState
from easy_gaussian_splatting_amd.viewer import FrameRenderer, finish_frame, frame_depth_range

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(1, 1), (1, 5), (2, 3), (3, 7), (16, 16), (17, 33), (64, 48)]
PADS = [None, (1, 0), (0, 3), (2, 5)]   # between them: 3 out_W odd, = 2 mod 4 and = 0 mod 4; byte totals no multiple of 4
GUARD = 64


def guarded(shape, dtype, fill=0xA5):
    """-> (the whole buffer as bytes, `shape` / `dtype` view of its front): GUARD bytes behind the frame, everything `fill`"""
    n = int(np.prod(shape)) * (4 if dtype == torch.float32 else 1)
    buf = torch.full((n + GUARD,), fill, dtype=torch.uint8, device=DEV)
    return buf, buf[:n].view(dtype).view(shape)


def bits(t):
    return t.cpu().contiguous().view(torch.uint8).numpy().tobytes() if t.dtype == torch.float32 else t.cpu().numpy().tobytes()


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_colour_frames_equal_numpy_bit_for_bit(H, W, C):
    x = TH.noisy_render(H, W, C, 100 * H + W + C)
    xd = torch.from_numpy(x).to(DEV)
    for pad in PADS:
        pad_to = None if pad is None else (H + pad[0], W + pad[1])
        shape = (H, W, 3) if pad_to is None else (pad_to[0], pad_to[1], 3)
        for fmt, dtype in (("uint8", torch.uint8), ("float32", torch.float32)):
            want = TH.np_finish(x, "rgb", fmt, pad_to)
            buf, out = guarded(shape, dtype)
            assert finish_frame(xd, mode="rgb", fmt=fmt, pad_to=pad_to, out=out) is out
            got = out.cpu().numpy()
            assert TH.same_bits(got, want), (pad, fmt, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
            assert (buf[-GUARD:] == 0xA5).all(), (pad, fmt, "bytes behind the frame were written")
            first = bits(out)
            finish_frame(xd, mode="rgb", fmt=fmt, pad_to=pad_to, out=out)     # again: identical bytes
            assert bits(out) == first
            buf0, out0 = guarded(shape, dtype, fill=0x00)                       # what the buffer held before does not matter
            finish_frame(xd, mode="rgb", fmt=fmt, pad_to=pad_to, out=out0)
            assert bits(out0) == first and not buf0[-GUARD:].any()
            fresh = finish_frame(xd, mode="rgb", fmt=fmt, pad_to=pad_to)       # (and without `out`)
            assert bits(fresh) == first


def test_float_frames_equal_torch_clamp_on_the_device():
    x = TH.noisy_render(64, 48, 3, 9)
    x = np.where(np.isnan(x) | (x == 0), np.float32(0.25), x)   # (finite and not a zero: those two are stated by the numpy statement)
    xd = torch.from_numpy(x).to(DEV)
    assert torch.equal(finish_frame(xd, fmt="float32"), torch.clamp(xd, 0.0, 1.0))


# ---- gs_frame_range ----

def alpha_pattern(name, H, W):
    a = torch.zeros(H, W)
    if name == "all":
        a += 0.9
    elif name == "last":
        a[-1, -1] = 0.5   # (exactly alpha_min: covered)
    elif name == "checker":
        a[(torch.arange(H)[:, None] + torch.arange(W)[None]) % 2 == 0] = 0.75
    return a


def depth_case(H, W, C, seed, nan=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(H, W, C, generator=g) * 3.0 - 1.0
    x[..., -1] = torch.rand(H, W, generator=g) * 8.0 + 0.5
    if nan and H * W > 2:
        x.view(-1, C)[(H * W) // 2, -1] = float("nan")
        x.view(-1, C)[0, -1] = float("nan")
    return x


@pytest.mark.parametrize("pattern", ["all", "none", "last", "checker"])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 7), (17, 33), (64, 48), (130, 70)])
def test_the_depth_range_is_the_min_and_max_of_the_covered_depths(H, W, C, pattern):
    x, a = depth_case(H, W, C, 7 * H + W), alpha_pattern(pattern, H, W)
    d = x[..., -1]
    m = (a >= 0.5) & ~torch.isnan(d)
    want = torch.stack([d[m].min(), d[m].max()]) if m.any() else torch.zeros(2)
    xd, ad = x.to(DEV), a.to(DEV)
    got = frame_depth_range(xd, ad)
    assert torch.equal(got.cpu(), want), (got, want)
    # the workspace's old contents do not matter
    st = torch.cuda.current_stream(DEV).cuda_stream
    for fill in (float("nan"), -1e30, 1e30):
        V._WORKSPACES[(DEV, st)].fill_(fill)
        assert torch.equal(frame_depth_range(xd, ad).cpu(), want), fill
    if pattern == "none":
        assert torch.equal(got.cpu(), torch.zeros(2))


# ---- depth frames ----

@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 7), (17, 33), (64, 48)])
def test_depth_frames_are_within_one_code_of_numpy(H, W, C):
    x, a = depth_case(H, W, C, 3 * H + W, nan=False), torch.rand(H, W, generator=torch.Generator().manual_seed(H))
    a.view(-1)[-1] = 0.9
    xd, ad = x.to(DEV), a.to(DEV)
    rng = frame_depth_range(xd, ad)
    lo, hi = (float(v) for v in rng.cpu())
    assert (lo, hi) == tuple(float(v) for v in TH.np_range(x.numpy(), a.numpy()))
    covered = a.numpy() >= 0.5
    for pad in PADS:
        pad_to = None if pad is None else (H + pad[0], W + pad[1])
        want8 = TH.np_finish(x.numpy(), "depth", "uint8", pad_to, a.numpy(), (lo, hi)).astype(np.int32)
        got8 = finish_frame(xd, mode="depth", fmt="uint8", pad_to=pad_to, alphas=ad)
        diff = np.abs(got8.cpu().numpy().astype(np.int32) - want8)
        print(f"depth u8 {H}x{W} C={C} pad={pad}: max |code difference| {diff.max()}, differing {int((diff > 0).sum())}")
        assert diff.max() <= 1
        assert (got8.cpu().numpy()[:H, :W][~covered] == 0).all() and not got8.cpu().numpy()[H:].any() and not got8.cpu().numpy()[:, W:].any()
        # a range chosen on the host gives the bytes of the same pair left on the device by gs_frame_range
        assert bits(finish_frame(xd, mode="depth", fmt="uint8", pad_to=pad_to, alphas=ad, depth_range=(lo, hi))) == bits(got8)
        assert bits(finish_frame(xd, mode="depth", fmt="uint8", pad_to=pad_to, alphas=ad, depth_range=rng)) == bits(got8)
        want32 = TH.np_finish(x.numpy(), "depth", "float32", pad_to, a.numpy(), (lo, hi))
        got32 = finish_frame(xd, mode="depth", fmt="float32", pad_to=pad_to, alphas=ad[..., None]).cpu().numpy()
        err = np.abs(got32.astype(np.float64) - want32.astype(np.float64)).max()
        print(f"depth f32 {H}x{W} C={C} pad={pad}: max |difference| {err:.3g}")
        assert err <= 2.0 ** -23
    # hi == lo: every covered pixel is white
    flat = finish_frame(xd, mode="depth", fmt="uint8", alphas=ad, depth_range=(2.5, 2.5)).cpu().numpy()
    assert (flat[covered] == 255).all() and (flat[~covered] == 0).all()
    # a NaN depth: skipped by the range, 0 as a code, a NaN as a float
    if H * W > 2:
        xn = x.clone()
        xn.view(-1, C)[-1, -1] = float("nan")
        xnd = xn.to(DEV)
        assert torch.equal(frame_depth_range(xnd, ad).cpu(), torch.tensor(TH.np_range(xn.numpy(), a.numpy())))
        assert finish_frame(xnd, mode="depth", fmt="uint8", alphas=ad).cpu().numpy()[-1, -1].tolist() == [0, 0, 0]
        assert np.isnan(finish_frame(xnd, mode="depth", fmt="float32", alphas=ad).cpu().numpy()[-1, -1]).all()


def test_a_depth_channel_view_is_read_in_place_like_its_copy():
    x = depth_case(17, 33, 4, 1, nan=False).to(DEV)
    a = torch.rand(17, 33, 1, device=DEV)
    view = x[..., 3:]
    assert not view.is_contiguous()
    for fmt in ("uint8", "float32"):
        want = bits(finish_frame(view.contiguous(), mode="depth", fmt=fmt, alphas=a))
        assert bits(finish_frame(view, mode="depth", fmt=fmt, alphas=a)) == want == bits(finish_frame(x, mode="depth", fmt=fmt, alphas=a))
    assert torch.equal(frame_depth_range(view, a), frame_depth_range(view.contiguous(), a))


# ---- FrameRenderer ----

LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
_SCENES = {}


def scene(W, H, n=2000, n_views=9, seed=3):
    """-> (make() -> (model, optimizer), camera states of the views, the scene dict); built once per size"""
    if (W, H) not in _SCENES:
        from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
        from easy_gaussian_splatting_amd.synthetic import make_scene
        sc = make_scene(n, W, H, sh_degree=3, n_views=n_views, seed=seed, scale_range=(0.02, 0.12), dist=4.0)
        T = torch.from_numpy
        op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
        shs = T(sc["shs"])

        def make():
            m = GaussianModel(means=T(sc["means"]), log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=shs[:, :1].contiguous(),
                              sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                              white_background=True, means_lr_schedule_max_steps=40).to(DEV)
            return m, build_optimizers(m, *LRS, fused="hip")

        cams = [CameraState(sc["viewmats"][v].astype(np.float64), sc["Ks"][v].copy(), W, H) for v in range(n_views)]
        _SCENES[(W, H)] = (make, cams, sc)
    return _SCENES[(W, H)]


def reference_frame(model, cs):
    """the reference's gs_render_func, line for line in effect: two uploads, model(data), the float32 image on the host"""
    data = {"w2c": torch.tensor(cs.w2c, dtype=torch.float32, device=DEV), "K": torch.tensor(cs.K, dtype=torch.float32, device=DEV),
            "height": cs.height, "width": cs.width}
    with torch.no_grad():
        return model(data)["render_img"].cpu().numpy()


def pad_like_the_reference(image, aspect):
    """adjust_image_aspect in numpy"""
    h, w = image.shape[:2]
    new_h, new_w = (h, int(h * aspect)) if w / h < aspect else ((int(w / aspect), w) if w / h > aspect else (h, w))
    out = np.zeros((new_h, new_w, 3), dtype=image.dtype)
    out[:h, :w] = image
    return out


@pytest.mark.parametrize("W,H", [(176, 112), (64, 48)])
def test_render_gives_the_references_frame(W, H):
    make, cams, _ = scene(W, H)
    model, _ = make()
    model.eval()
    r = FrameRenderer(model)
    cs = cams[1]
    want = reference_frame(model, cs)
    assert 0.0 < want.mean() < 1.0 and want.std() > 0.01
    got = r.render(cs)
    assert got.dtype == np.float32 and TH.same_bits(got, want)
    assert TH.same_bits(r.render(cs, fmt="uint8"), np.floor(want * 255.0).astype(np.uint8))
    for aspect in (2.0, 1.1):   # wider and taller than 176 x 112 and 64 x 48
        padded = pad_like_the_reference(want, aspect)
        assert padded.shape != want.shape
        assert TH.same_bits(r.render(cs, aspect=aspect), padded)
        assert TH.same_bits(r.render(cs, aspect=aspect, fmt="uint8"), np.floor(padded * 255.0).astype(np.uint8))
    assert TH.same_bits(r.render(cs, aspect=W / H), want)
    # depth: the model's own expected depth and opacity through finish_frame
    data = {"w2c": torch.tensor(cs.w2c, dtype=torch.float32, device=DEV), "K": torch.tensor(cs.K, dtype=torch.float32, device=DEV),
            "height": H, "width": W}
    with torch.no_grad():
        out = model(data, clamp=False, depth="ED", alphas=True)
    assert out["render_alpha"].shape == (H, W, 1) and TH.same_bits(torch.clamp(out["render_img"], 0, 1).cpu().numpy(), want)
    for fmt in ("uint8", "float32"):
        want_d = finish_frame(out["render_depth"], mode="depth", fmt=fmt, alphas=out["render_alpha"]).cpu().numpy()
        got_d = r.render(cs, mode="depth", fmt=fmt)
        assert TH.same_bits(got_d, want_d)
        assert (got_d[..., 0] == got_d[..., 1]).all() and got_d.max() == (255 if fmt == "uint8" else 1.0) and got_d.min() == 0
    # the returned array is a ring slot: valid for ring - 1 further frames; copy=True is private
    a = r.render(cs, fmt="uint8")
    keep = a.copy()
    b, c = r.render(cams[2], fmt="uint8"), r.render(cams[3], fmt="uint8")
    assert np.array_equal(a, keep) and not np.array_equal(b, keep) and not np.shares_memory(a, b) and not np.shares_memory(a, c)
    d = r.render(cams[4], fmt="uint8")
    assert np.shares_memory(a, d)
    e = r.render(cs, fmt="uint8", copy=True)
    assert np.array_equal(e, keep) and not any(np.shares_memory(e, s) for s in (a, b, c))


def test_render_leaves_the_model_in_the_mode_it_found():
    make, cams, _ = scene(64, 48)
    model, _ = make()
    r = FrameRenderer(model)
    model.train()
    seen = []
    hook = model.register_forward_pre_hook(lambda m, args: seen.append(m.training))
    a = r.render(cams[0])
    assert model.training and seen == [False]
    model.eval()
    b = r.render(cams[0])
    assert not model.training and seen == [False, False] and TH.same_bits(a, b)
    model.train()
    assert len(list(r.render_path(cams[:3]))) == 3 and model.training and seen == [False] * 5
    hook.remove()
    from easy_gaussian_splatting_amd.viewer import viewer_render_func
    f = viewer_render_func(model)
    assert TH.same_bits(f(cams[0]), a) and model.training


@pytest.mark.parametrize("sleep", [0.0, 0.02])
def test_the_path_ring_hands_every_frame_over_intact(sleep):
    make, cams, _ = scene(64, 48)
    model, _ = make()
    model.eval()
    r = FrameRenderer(model, ring=2)
    assert len(cams) == 9
    want = [r.render(cs, fmt="uint8", copy=True) for cs in cams]
    assert len({w.tobytes() for w in want}) == 9
    got = []
    for frame in r.render_path(cams, fmt="uint8"):
        if sleep:
            time.sleep(sleep)   # the next frame is in flight meanwhile: it must not land in this one's buffer
        got.append(frame.copy())
    assert len(got) == 9
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), i
    # float32 frames through the default ring, and an export through a renderer
    r3 = FrameRenderer(model)
    for g, w in zip(r3.render_path(cams[:4], fmt="float32"), want):
        assert np.array_equal(np.floor(g * 255.0).astype(np.uint8), w)


def test_export_video_renders_a_path_through_the_renderer(tmp_path):
    make, cams, _ = scene(64, 48)
    model, _ = make()
    r = FrameRenderer(model.eval())
    out = V.export_video(r, cams[:3], 0.5, 12.0, tmp_path, writer=V.write_ppm_frames)
    path = V.camera_interpolation(cams[:3], 0.5, 12.0)
    files = sorted(out.glob("*.ppm"))
    assert len(files) == len(path) > 3
    for f, cs in list(zip(files, path))[::2]:
        raw = f.read_bytes()
        img = np.frombuffer(raw[len(b"P6\n64 48\n255\n"):], dtype=np.uint8).reshape(48, 64, 3)
        assert np.array_equal(img, r.render(cs, fmt="uint8"))


def test_four_threads_share_one_renderer():
    make, cams, _ = scene(64, 48)
    model, _ = make()
    r = FrameRenderer(model.eval())
    want = [r.render(cs, copy=True) for cs in cams[:4]]
    results, errors = {}, []

    def work(t):
        try:
            results[t] = [r.render(cams[(t + k) % 4], copy=True) for k in range(5)]
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(4):
        for k in range(5):
            assert TH.same_bits(results[t][k], want[(t + k) % 4]), (t, k)


def test_rendering_between_captured_steps_leaves_the_run_bit_identical():
    """Six TrainStepGraph steps with a render() after every step -- from a camera the training views do not contain, on the
    caller's stream: the next step waits for it on entry -- end on the parameters and Adam moments of the same six steps
    without the renders, and the frame after step k is an eager model(data) of the parameters after step k."""
    from easy_gaussian_splatting_amd.loss import LossComputer
    from easy_gaussian_splatting_amd.train_graph import TrainStepGraph
    make, cams, sc = scene(64, 48)
    target, _ = make()
    with torch.no_grad():
        target.means.add_(0.03 * torch.randn(target.means.shape, generator=torch.Generator().manual_seed(5)).to(DEV))
    datas = [{"w2c": torch.tensor(cs.w2c, dtype=torch.float32, device=DEV), "K": torch.tensor(cs.K, dtype=torch.float32, device=DEV),
              "width": 64, "height": 48} for cs in cams[:4]]
    with torch.no_grad():
        gts = [target(d)["render_img"].clone() for d in datas]
    lc = LossComputer(0.2, clamp_input=True)
    free = cams[7]

    def run(with_render):
        model, opt = make()
        runner = TrainStepGraph(model, opt, lc, datas[0], gts[0])
        renderer = FrameRenderer(model)
        frames, saved = [], []
        for it in range(6):
            model.update_learning_rate(it)
            runner.step(datas[it % 4], gts[it % 4])
            if with_render:
                frames.append(renderer.render(free, copy=True))
                assert model.training
                saved.append({k: getattr(model, k).detach().clone() for k in model.param_names})
        runner.finish()
        assert runner.report()["overflows"] == 0
        return model, opt, frames, saved

    ma, oa, frames, saved = run(True)
    mb, ob, _, _ = run(False)
    for k in ma.param_names:
        assert torch.equal(getattr(ma, k).detach(), getattr(mb, k).detach()), k
        for x, y in zip(oa.moments_of(getattr(ma, k)), ob.moments_of(getattr(mb, k))):
            assert torch.equal(x, y), (k, "moment")
    assert len(frames) == 6 and not np.array_equal(frames[0], frames[5])
    for got, params in zip(frames, saved):
        copy, _ = make()
        with torch.no_grad():
            for k, v in params.items():
                getattr(copy, k).copy_(v)
        assert TH.same_bits(got, reference_frame(copy.eval(), free))
