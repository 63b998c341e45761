"""Colour features of more than four channels, host side: the chunking, the front end's refusals and the argument checks of the
chunk entry points (include/gs_raster.h: gs_rec_colors_chunk, gs_channel_grads_chunk, gs_rows_accumulate, gs_chunk_scatter,
gs_chunk_gather) -- nothing here launches a kernel."""
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


def test_channel_chunks():
    from easy_gaussian_splatting_amd.rendering import channel_chunks
    assert channel_chunks(5) == [(0, 4), (4, 1)]
    assert channel_chunks(8) == [(0, 4), (4, 4)]
    assert channel_chunks(9) == [(0, 4), (4, 4), (8, 1)]
    assert channel_chunks(32) == [(4 * j, 4) for j in range(8)]
    assert channel_chunks(7)[-1] == (4, 3) and channel_chunks(3) == [(0, 3)]
    for D in range(1, 40):   # the chunks tile [0, D) in order, four wide up to the tail
        ch = channel_chunks(D)
        assert [f for f, _ in ch] == list(range(0, D, 4)) and sum(c for _, c in ch) == D and all(c == 4 for _, c in ch[:-1])
    with pytest.raises(ValueError):
        channel_chunks(0)


def _inputs(N=8, C=2, D=5, per_cam=False):
    quats = torch.zeros(N, 4)
    quats[:, 0] = 1.0
    return dict(means=torch.zeros(N, 3), quats=quats, scales=torch.full((N, 3), 0.1), opacities=torch.full((N,), 0.5),
                colors=torch.zeros((C, N, D) if per_cam else (N, D)), viewmats=torch.eye(4)[None].repeat(C, 1, 1),
                Ks=torch.eye(3)[None].repeat(C, 1, 1))


def _call(t, **kw):
    from easy_gaussian_splatting_amd.rendering import rasterization
    return rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"], 32, 32,
                         sh_degree=None, packed=False, **kw)


@pytest.mark.parametrize("D", [5, 9])
@pytest.mark.parametrize("per_cam", [False, True])
def test_more_than_four_channels_on_cpu_tensors_name_the_gpu(D, per_cam):
    # past every front-end check: the refusal is the device's, no longer the channel count's -- and still a NotImplementedError
    t = _inputs(D=D, per_cam=per_cam)
    for kw in (dict(), dict(backgrounds=torch.zeros(2, D)), dict(channel_chunk=7)):
        with pytest.raises(NotImplementedError, match="GPU only") as e:
            _call(t, **kw)
        assert "chunks of 4" in str(e.value) and "no CPU fallback" in str(e.value) and isinstance(e.value, RuntimeError)
    with pytest.raises(AssertionError):   # (backgrounds carry all D channels)
        _call(t, backgrounds=torch.zeros(2, 4))


@pytest.mark.parametrize("mode", ["D", "ED", "RGB+D", "RGB+ED"])
def test_more_than_four_channels_with_a_depth_mode_stay_refused(mode):
    with pytest.raises(NotImplementedError, match="render_mode"):
        _call(_inputs(D=5), render_mode=mode)
    with pytest.raises(NotImplementedError, match="4"):   # (four features + depth: as before)
        _call(_inputs(D=4), render_mode="RGB+D")


@pytest.mark.parametrize("D", [5, 9])
def test_more_than_four_channels_refuse_absgrad(D):
    with pytest.raises(NotImplementedError, match="absgrad"):
        _call(_inputs(D=D), absgrad=True)
    with pytest.raises(RuntimeError, match="GPU only"):   # (D = 4 has it)
        _call(_inputs(D=4), absgrad=True)


@pytest.mark.parametrize("kw", [dict(_sh_grads="colors_pre"), dict(_grad_out={"means": torch.zeros(8, 3)}),
                                dict(_sh_grads="colors_pre", _view_payload=torch.zeros(64)), dict(_rounds="on")])
def test_view_parallel_keywords_and_rounds_as_for_narrow_features(kw):
    # D > 4 is refused or accepted exactly where D = 1, 2, 4 are: on CPU tensors both stop at the device check
    outcomes = []
    for D in (1, 2, 4, 5, 9):
        with pytest.raises(Exception) as e:
            _call(_inputs(D=D), **kw)
        outcomes.append((isinstance(e.value, ValueError), isinstance(e.value, RuntimeError), "GPU only" in str(e.value)))
    assert len(set(outcomes)) == 1, outcomes


class _Buf:
    """A zeroed host buffer with a 256-byte aligned address (the entry points check alignment before they look further)."""
    def __init__(self, n=4096):
        self.raw = (ct.c_uint8 * (n + 256))()
        a = ct.addressof(self.raw)
        self.p = a + ((-a) % 256)


def _entry_points(L, p, D, first, count, over=None):
    """Every chunk entry point on the chunk (first, count) of D channels, all pointers `p` but those named in `over`
    ({parameter name: address})."""
    o = over or {}
    g = lambda name: o.get(name, p)
    return {
        "gs_rec_colors_chunk": lambda: L.gs_rec_colors_chunk(None, 1, 8, D, first, count, g("colors"), 0, g("radii"), g("rec")),
        "gs_channel_grads_chunk": lambda: L.gs_channel_grads_chunk(None, 1, 8, D, first, count, 0, g("radii"), g("tiles_per_gauss"),
                                                                   g("cum_tiles"), g("rows"), g("row_base"), g("qmask"), g("v_colors")),
        "gs_chunk_scatter": lambda: L.gs_chunk_scatter(None, 16, D, first, count, g("src"), g("dst")),
        "gs_chunk_gather": lambda: L.gs_chunk_gather(None, 16, D, first, count, g("src"), g("dst")),
    }


BAD_CHUNKS = [(0, 0, 1), (-3, 0, 1),      # D >= 1
              (8, -4, 4), (8, 2, 2), (8, 5, 1),   # first >= 0, a multiple of 4
              (8, 0, 0), (8, 0, 5), (8, 4, -1),   # 1 <= count <= 4
              (5, 4, 2), (8, 8, 1), (4, 4, 4), (7, 4, 4)]   # first + count <= D


@pytest.mark.parametrize("D,first,count", BAD_CHUNKS)
def test_chunk_entry_points_refuse_bad_chunks(native, D, first, count):
    L = native.lib()
    b = _Buf()
    for name, call in _entry_points(L, b.p, D, first, count).items():
        assert call() == -1, name
        assert b"channels" in L.gs_last_error(), (name, L.gs_last_error())


def test_chunk_entry_points_refuse_missing_pointers(native):
    L = native.lib()
    b = _Buf()
    pointers = {"gs_rec_colors_chunk": ("colors", "radii", "rec"),
                "gs_channel_grads_chunk": ("radii", "tiles_per_gauss", "cum_tiles", "rows", "row_base", "qmask", "v_colors"),
                "gs_chunk_scatter": ("src", "dst"), "gs_chunk_gather": ("src", "dst")}
    for name, params in pointers.items():
        for param in params:
            assert _entry_points(L, b.p, 9, 8, 1, {param: None})[name]() == -1, (name, param)
            assert b"null" in L.gs_last_error(), (name, param, L.gs_last_error())
    assert L.gs_rows_accumulate(None, 4, None, b.p, 1) == -1 and b"null" in L.gs_last_error()
    assert L.gs_rows_accumulate(None, 4, b.p, None, 0) == -1 and b"null" in L.gs_last_error()


def test_chunk_entry_points_refuse_misaligned_pointers(native):
    L = native.lib()
    b = _Buf()
    p = b.p
    # whole quads of a D that is a multiple of 4 move as float4: the D-wide and the dense arrays are 16-byte aligned then
    quads = {"gs_rec_colors_chunk": ("colors", "rec"), "gs_channel_grads_chunk": ("rows", "qmask", "v_colors"),
             "gs_chunk_scatter": ("src", "dst"), "gs_chunk_gather": ("src", "dst")}
    for name, params in quads.items():
        for param in params:
            assert _entry_points(L, p, 8, 4, 4, {param: p + 4})[name]() == -1, (name, param)
            assert b"aligned" in L.gs_last_error(), (name, param, L.gs_last_error())
    # a tail, or a D that is no multiple of 4: floats -- but the records, the rows and the masks stay 16-byte aligned
    always16 = {"gs_rec_colors_chunk": ("rec",), "gs_channel_grads_chunk": ("rows", "qmask")}
    floats = {"gs_rec_colors_chunk": ("colors",), "gs_channel_grads_chunk": ("v_colors",), "gs_chunk_scatter": ("src", "dst"),
              "gs_chunk_gather": ("src", "dst")}
    for D, first, count in ((9, 8, 1), (9, 4, 4), (7, 4, 3)):
        for name, params in always16.items():
            for param in params:
                assert _entry_points(L, p, D, first, count, {param: p + 4})[name]() == -1, (name, param)
                assert b"aligned" in L.gs_last_error(), (name, param, L.gs_last_error())
        for name, params in floats.items():
            for param in params:
                assert _entry_points(L, p, D, first, count, {param: p + 2})[name]() == -1, (name, param)
                assert b"aligned" in L.gs_last_error(), (name, param, L.gs_last_error())
    for rows, acc in ((p + 4, p + 256), (p, p + 256 + 8)):
        assert L.gs_rows_accumulate(None, 4, rows, acc, 1) == -1 and b"aligned" in L.gs_last_error()


def test_rows_accumulate_refuses_bad_sizes_and_aliases(native):
    L = native.lib()
    b = _Buf()
    assert L.gs_rows_accumulate(None, -1, b.p, b.p + 256, 1) == -1 and b"n_rows" in L.gs_last_error()
    assert L.gs_rows_accumulate(None, 1 << 31, b.p, b.p + 256, 1) == -1 and b"n_rows" in L.gs_last_error()
    assert L.gs_rows_accumulate(None, 4, b.p, b.p, 0) == -1 and b"two buffers" in L.gs_last_error()
    # nothing to do: accepted without a launch
    assert L.gs_rows_accumulate(None, 0, b.p, b.p + 256, 1) == 0
    assert L.gs_chunk_scatter(None, 0, 8, 4, 4, b.p, b.p + 256) == 0 and L.gs_chunk_gather(None, 0, 5, 4, 1, b.p, b.p + 256) == 0
    assert L.gs_chunk_scatter(None, -1, 8, 4, 4, b.p, b.p + 256) == -1 and b"n_pixels" in L.gs_last_error()


def test_four_channel_entry_points_keep_refusing_wider_counts(native):
    L = native.lib()
    b = _Buf()
    p = b.p
    for bad in (5, 8, 9):
        assert L.gs_rec_colors(None, 1, 8, bad, p, 0, p, p) == -1 and b"channels" in L.gs_last_error()
        assert L.gs_channel_grads(None, 1, 8, bad, 0, p, p, p, p, p, p, p) == -1 and b"channels" in L.gs_last_error()


def test_the_new_file_is_built_and_declared(native):
    here = os.path.dirname(os.path.abspath(__file__))
    mk = open(os.path.join(here, "..", "easy_gaussian_splatting_amd", "csrc", "Makefile")).read()
    assert "gs_wide.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    for name in ("gs_rec_colors_chunk", "gs_channel_grads_chunk", "gs_rows_accumulate", "gs_chunk_scatter", "gs_chunk_gather"):
        assert hasattr(native.lib(), name), name
