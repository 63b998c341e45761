"""The list and blend stage calls (rendering.stage_count / stage_lists / stage_blend_fwd / stage_blend_bwd), host side: every argument of
the eight entry points they reach lands under its own parameter NAME of include/gs_raster.h -- the order of a call, which the call-site
count of test_native_header.py cannot see (every pointer is a void*: two swapped neighbours load and run).  Stand-ins for the library and
the lease; no GPU, no built library."""
import ast
import os

import pytest

from easy_gaussian_splatting_amd import _native as nat
from easy_gaussian_splatting_amd import rendering as R
from easy_gaussian_splatting_amd import workspace as WS

# parameter name -> the workspace slot whose address it takes
SLOT_OF = {"rec": WS.REC, "isect_offsets": WS.ISECT_OFFSETS, "bucket_offsets": WS.BUCKET_OFFSETS, "tile_order": WS.TILE_ORDER,
           "cum_tiles": WS.CUM_TILES, "coarse_keys": WS.COARSE_KEYS, "keys_tmp": WS.KEYS_TMP, "slot_gid": WS.SLOT_GID, "isect_ids": WS.ISECT_IDS,
           "flatten_ids": WS.FLATTEN_IDS, "slots": WS.SLOTS, "ckpt": WS.CKPT, "qlist": WS.QLIST, "qcnt": WS.QCNT, "qmask": WS.QMASK,
           "unit_desc": WS.UNIT_DESC, "row_base": WS.ROW_BASE, "walk_state": WS.WALK_STATE, "rows": WS.ROWS, "workspace": WS.BIN, "info_dev": WS.INFO}
# what only a training layout holds (gs_workspace_query): the walk arena and the walk's share of the other two
TRAIN_ONLY = {WS.QCNT, WS.SH_JAC, WS.SLOT_GID, WS.SLOTS, WS.QMASK, WS.ROW_BASE, WS.WALK_STATE, WS.CKPT, WS.QLIST, WS.UNIT_DESC, WS.ROWS}
CKPT_EXT = 0xE47000
ST, C, N, TW, TH, W, H = 0x57, 2, 1001, 7, 5, 111, 79
COARSE_CAP, SHIFT, CAP_UNITS, CAP_ROWS = 30011, 1, 771, 90001


def _address(slot, train, ids=False):
    """What the stand-in lease gives for a slot: None where its layout does not hold it (the sorted keys: only a layout that asks for them)."""
    if (slot == WS.ISECT_IDS and not ids) or (slot in TRAIN_ONLY and not train):
        return None
    return 0x1000 * (slot + 1)


class _Layout:
    def __init__(self, train, two_level):
        flags = (WS.F_TRAIN if train else 0) | (WS.F_TWO_LEVEL if two_level else 0)
        self.key = (C, N, W, H, 50021, COARSE_CAP if two_level else 0, SHIFT if two_level else 0, flags, CAP_UNITS, CAP_ROWS)
        self.cap_units, self.cap_rows = CAP_UNITS, CAP_ROWS

    def extent(self, slot):
        return 0xB10000 + slot


class _Lease:
    def __init__(self, train, two_level, ids):
        self.layout, self.train, self.ids = _Layout(train, two_level), train, ids

    def ptr(self, slot):
        return _address(slot, self.train, self.ids)

    def ckpt_ext(self):
        return CKPT_EXT


class _Library:
    """Records the positional arguments of every gs_* call; every call succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gs_"):
            raise AttributeError(name)

        def entry(*args, **kw):
            assert not kw
            self.calls.append((name, args))
            return 0
        return entry


def _run(fn, train, two_level, *args, ids=False):
    """One stage call on the stand-ins: (entry point, {parameter name: argument}); the wrapper saw its return code under its name."""
    L, checked = _Library(), []
    fn(L, ST, _Lease(train, two_level, ids), *args, check=lambda rc, what: checked.append((rc, what)))
    assert len(L.calls) == 1
    name, got = L.calls[0]
    assert checked == [(0, name)]
    assert len(got) == len(nat.PARAMS[name]), (name, len(got), nat.PARAMS[name])
    return name, dict(zip(nat.PARAMS[name], got))


def _compare(name, got, train, given, ids=False):
    """Every parameter of the call: a slot's address for the parameters named after one, else what the caller handed in."""
    for param, value in got.items():
        if param in SLOT_OF:
            want = _address(SLOT_OF[param], train, ids)
        else:
            assert param in given, f"{name}: no expectation for parameter {param!r}"
            want = given[param]
        assert value == want and type(value) is type(want), f"{name}({param}) received {value!r}, expected {want!r}"


_LAYOUTS = [(train, two_level) for train in (True, False) for two_level in (False, True)]


@pytest.mark.parametrize("train,two_level", _LAYOUTS)
def test_count_arguments_land_under_their_names(train, two_level):
    bbox, depths, coarse_list_cap = 0xBB0, 0xDE0, 313
    name, got = _run(R.stage_count, train, two_level, (C, N, TW, TH), bbox, depths, coarse_list_cap)
    assert name == ("gs_bins_count" if two_level else "gs_bin_count")
    _compare(name, got, train, dict(stream=ST, C=C, N=N, tile_w=TW, tile_h=TH, bin_shift=SHIFT, bbox=bbox, depths=depths,
                                    workspace_bytes=0xB10000 + WS.BIN, coarse_cap=COARSE_CAP, coarse_list_cap=coarse_list_cap, info_host=None))


@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("train,two_level", _LAYOUTS)
def test_list_arguments_land_under_their_names(train, two_level, ids):
    bbox, depths, n_isects, max_tile_count = 0xBB0, 0xDE0, 40009, 4096
    name, got = _run(R.stage_lists, train, two_level, (C, N, TW, TH), bbox, depths, n_isects, max_tile_count, ids=ids)
    assert name == ("gs_bins_lists" if two_level else "gs_bin_emit_sort")
    _compare(name, got, train, dict(stream=ST, C=C, N=N, tile_w=TW, tile_h=TH, bin_shift=SHIFT, bbox=bbox, depths=depths,
                                    workspace_bytes=0xB10000 + WS.BIN, coarse_cap=COARSE_CAP, n_isects=n_isects, max_tile_count=max_tile_count), ids)


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("train,two_level", _LAYOUTS)
def test_blend_forward_arguments_land_under_their_names(train, two_level, ch):
    backgrounds, n_isects, colors, alphas = 0xB60, 40009, 0xC01, 0xA1F
    name, got = _run(R.stage_blend_fwd, train, two_level, C, W, H, ch, backgrounds, n_isects, colors, alphas)
    assert name == ("gs_blend_fwd" if ch == 3 else "gs_blend_fwd_ch")
    _compare(name, got, train, dict(stream=ST, C=C, width=W, height=H, channels=ch, backgrounds=backgrounds, n_isects=n_isects, render_colors=colors,
                                    render_alphas=alphas, cap_units=CAP_UNITS, cap_rows=CAP_ROWS, ckpt_ext=CKPT_EXT if (train and ch == 4) else None))


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("train,two_level", _LAYOUTS)
def test_blend_backward_arguments_land_under_their_names(train, two_level, ch):
    colors, alphas, v_colors, v_alphas, unit_classes = 0xC01, 0xA1F, 0x7C0, 0x7A1, 0xC15
    name, got = _run(R.stage_blend_bwd, train, two_level, C, W, H, ch, colors, alphas, v_colors, v_alphas, unit_classes)
    assert name == ("gs_blend_bwd" if ch == 3 else "gs_blend_bwd_ch")
    _compare(name, got, train, dict(stream=ST, C=C, width=W, height=H, channels=ch, render_colors=colors, render_alphas=alphas, v_render_colors=v_colors,
                                    v_render_alphas=v_alphas, cap_units=CAP_UNITS, unit_classes=unit_classes,
                                    ckpt_ext=CKPT_EXT if (train and ch == 4) else None))


def test_every_fused_projection_backward_entry_has_a_row_in_the_variant_matrix():
    """The `VARIANTS` table of tests/fused_variants.py, which tests/test_gpu_fused_variants.py runs row by row at every SH degree,
    against the header: every gs_project_bwd_adam* entry point is reached by at least one row, and every row names an entry point the
    header declares -- one added later cannot arrive without a row in the matrix.  Names only."""
    import fused_variants as FV
    declared = {name for name in nat.SIGNATURES if name.startswith(FV.ENTRY_PREFIX)}
    reached = {v.entry for v in FV.VARIANTS}
    assert declared, "the header declares no fused projection backward at all"
    assert declared - reached == set(), f"no row of fused_variants.VARIANTS reaches {sorted(declared - reached)}"
    assert reached - declared == set(), f"fused_variants.VARIANTS names {sorted(reached - declared)}, which the header does not declare"
    # the matrix itself: 18 rows with tags of their own, the four regulariser masks where a family has the budget kernels
    assert len(FV.VARIANTS) == len(FV.BY_TAG) == 18
    for family, n_masks in (("plain", 4), ("poses", 4), ("depth", 4), ("ortho", 2), ("fisheye", 2), ("aa", 2)):
        rows = [v for v in FV.VARIANTS if v.family == family]
        assert [(v.scale, v.budget) for v in rows] == list(FV.MASKS[:n_masks]), family
        assert len({v.kernel for v in rows}) == n_masks, family   # (a kernel of its own per row)


def test_the_blend_and_the_captured_step_are_spelled_in_the_stage_functions_alone():
    """The four blend entry points are named once each in the package, in rendering.py; train_graph.py names none of the eight.  (The
    list builders of rendering.py that run on exact-size tensors of their own keep their count / emit calls.)"""
    eight = {"gs_bin_count", "gs_bins_count", "gs_bin_emit_sort", "gs_bins_lists", "gs_blend_fwd", "gs_blend_fwd_ch", "gs_blend_bwd", "gs_blend_bwd_ch"}
    pkg = os.path.dirname(os.path.abspath(R.__file__))
    named = {}
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            for node in ast.walk(ast.parse(open(os.path.join(pkg, f)).read())):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in eight:
                    named.setdefault(node.func.attr, []).append(f)
    assert set(named) == eight
    for name in ("gs_blend_fwd", "gs_blend_fwd_ch", "gs_blend_bwd", "gs_blend_bwd_ch"):
        assert named[name] == ["rendering.py"], (name, named[name])
    assert all(files.count("train_graph.py") == 0 for files in named.values()), named


def test_protect_pending_snapshots_the_named_fields_that_alias_a_static_buffer():
    """A queued step that was issued with "the camera the static buffer holds" keeps that camera when a later step overwrites the buffer:
    `_protect_pending` gives every pending record whose `w2c`, `K`, `gt` or `mask` is the buffer (or its row) ONE shared snapshot, in the
    shape the record had, and touches nothing else.  CPU tensors, a runner without its constructor."""
    import torch
    from easy_gaussian_splatting_amd import train_graph as TG
    static = torch.arange(16, dtype=torch.float32).reshape(1, 4, 4)
    old = static.clone()
    own = {name: torch.full(shape, fill) for name, shape, fill in (("w2c", (4, 4), 7.0), ("K", (3, 3), 2.0), ("gt", (6, 8, 3), 0.5), ("mask", (6, 8), 1.0))}
    whole = TG._Pending(1, [1e-3], static, own["K"], own["gt"], own["mask"])
    row = TG._Pending(2, [1e-3], static[0], own["K"], own["gt"], None, pose=(1, 2))
    apart = TG._Pending(3, [1e-3], own["w2c"], own["K"], own["gt"], own["mask"])
    runner = object.__new__(TG.TrainStepGraph)
    runner.pending = TG.deque([whole, row, apart])
    runner._protect_pending(static)
    static.fill_(-1.0)
    assert whole.w2c.shape == (1, 4, 4) and row.w2c.shape == (4, 4)
    assert torch.equal(whole.w2c, old) and torch.equal(row.w2c, old[0])
    assert whole.w2c.data_ptr() == row.w2c.data_ptr() != static.data_ptr()   # one snapshot for both
    assert apart.w2c is own["w2c"] and torch.equal(apart.w2c, torch.full((4, 4), 7.0))
    for e in (whole, row, apart):   # what does not alias the buffer stays the caller's own tensor
        assert e.K is own["K"] and e.gt is own["gt"] and e.mask is (None if e is row else own["mask"])
    assert (whole.t, row.t, apart.t) == (1, 2, 3) and row.pose == (1, 2) and whole.pose is None
    runner._protect_pending(own["K"])   # ... and so for a buffer that another field names: every record's K, nothing else
    assert whole.K is row.K is apart.K and whole.K is not own["K"] and torch.equal(whole.K, own["K"])
    assert apart.w2c is own["w2c"] and whole.gt is own["gt"]
