"""Colour features of 1 .. 4 channels, host side: the front end's refusals and the argument checks of the channel entry points
(include/gs_raster.h: gs_rec_colors, gs_blend_fwd_ch, gs_blend_bwd_ch, gs_channel_grads) -- nothing here launches a kernel."""
import ctypes as ct
import os

import pytest
import torch


@pytest.fixture(scope="module")
def native():
    from easy_gaussian_splatting_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _inputs(N=8, C=2, D=4):
    quats = torch.zeros(N, 4)
    quats[:, 0] = 1.0
    return dict(means=torch.zeros(N, 3), quats=quats, scales=torch.full((N, 3), 0.1), opacities=torch.full((N,), 0.5),
                colors=torch.zeros(N, D), viewmats=torch.eye(4)[None].repeat(C, 1, 1), Ks=torch.eye(3)[None].repeat(C, 1, 1))


def _call(t, **kw):
    from easy_gaussian_splatting_amd.rendering import rasterization
    return rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"], 32, 32,
                         sh_degree=None, packed=False, **kw)


@pytest.mark.parametrize("per_cam", [False, True])
def test_more_than_four_channels_raise_not_implemented(per_cam):
    t = _inputs(D=5)
    if per_cam:
        t["colors"] = torch.zeros(2, 8, 5)
    with pytest.raises(NotImplementedError, match="4"):
        _call(t)


def test_backgrounds_must_have_the_channel_count():
    t = _inputs(D=4)
    with pytest.raises(AssertionError):
        _call(t, backgrounds=torch.zeros(2, 3))
    t = _inputs(D=1)
    with pytest.raises(AssertionError):
        _call(t, backgrounds=torch.zeros(2, 3))


def test_supported_channel_counts_pass_the_front_end_checks():
    # D = 1, 2, 4 get past every argument check: on CPU tensors the call then stops at the device check
    for D in (1, 2, 4):
        t = _inputs(D=D)
        with pytest.raises(RuntimeError, match="GPU only"):
            _call(t, backgrounds=torch.zeros(2, D))


class _Buf:
    """A zeroed host buffer with a 256-byte aligned address (the entry points check alignment before they look further)."""
    def __init__(self, n=4096):
        self.raw = (ct.c_uint8 * (n + 256))()
        a = ct.addressof(self.raw)
        self.p = a + ((-a) % 256)


@pytest.mark.parametrize("bad", [0, 5, -1])
def test_channel_entry_points_refuse_channel_counts(native, bad):
    L = native.lib()
    b = _Buf()
    p = b.p
    assert L.gs_rec_colors(None, 1, 8, bad, p, 0, p, p) == -1
    assert b"channels" in L.gs_last_error()
    assert L.gs_blend_fwd_ch(None, 1, 16, 16, bad, p, None, p, None, p, None, 64, p, p, None, None, None, None, None, 0, None, 0,
                             None, None) == -1
    assert b"channels" in L.gs_last_error()
    assert L.gs_blend_bwd_ch(None, 1, 16, 16, bad, p, p, p, p, 256, p, p, p, p, p, p, p, None, p, None, p) == -1
    assert b"channels" in L.gs_last_error()
    assert L.gs_channel_grads(None, 1, 8, bad, 0, p, p, p, p, p, p, p) == -1
    assert b"channels" in L.gs_last_error()


def test_channel_entry_points_refuse_missing_pointers(native):
    L = native.lib()
    b = _Buf()
    p = b.p
    assert L.gs_rec_colors(None, 1, 8, 2, None, 0, p, p) == -1
    assert b"null" in L.gs_last_error()
    assert L.gs_blend_fwd_ch(None, 1, 16, 16, 4, p, None, None, None, p, None, 64, p, p, None, None, None, None, None, 0, None, 0,
                             None, None) == -1
    assert b"null" in L.gs_last_error()
    assert L.gs_blend_bwd_ch(None, 1, 16, 16, 1, p, p, p, p, 256, p, p, p, p, None, p, p, None, p, None, None) == -1
    assert b"null" in L.gs_last_error()
    assert L.gs_channel_grads(None, 1, 8, 4, 1, p, p, p, None, p, p, p) == -1
    assert b"null" in L.gs_last_error()


def test_four_channel_training_needs_the_checkpoint_plane(native):
    L = native.lib()
    bufs = [_Buf(1 << 16) for _ in range(10)]
    ck, ql, qc, qm, ud, rb, ws, rc, ra, ids = (x.p for x in bufs)
    # a training forward with every list output but no ckpt_ext: refused before anything is launched
    assert L.gs_blend_fwd_ch(None, 1, 16, 16, 4, rc, None, ids, None, ids, ids, 64, rc, ra, ck, ql, qc, qm, ud, 256, rb, 4096,
                             ws, None) == -1
    assert b"ckpt_ext" in L.gs_last_error()
    # ... and the backward of four channels
    assert L.gs_blend_bwd_ch(None, 1, 16, 16, 4, rc, ql, qc, ud, 256, ck, qm, rb, ws, rc, ra, rc, None, ra, None, None) == -1
    assert b"ckpt_ext" in L.gs_last_error()
