"""Tile binning and list sorts (csrc/gs_binning.hip) through the C ABI, against the plain NumPy reference of
tests/binning_ref.py: every size-class boundary of the sort, depth ties in every class, skipped radix passes, and the
hand-off structures of both pipelines.  Every comparison is an exact integer comparison.

Per-tile pipeline: gs_bin_count + gs_bin_emit_sort.  Two-level pipeline: gs_bins_count + gs_bins_lists, 2x2- and 4x4-tile
bins.  Each once with training lists (gradient-row slots) and once with inference lists (keys carry the flatten id), always
with an explicit isect_ids buffer and with capacities taken from the reference, so that no call is a guarded no-op.
"""
import contextlib
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import binning_ref as BR
from scenes import dense_scene

pytestmark = pytest.mark.gpu

PIPELINES = ("tiles", "bins1", "bins2")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ driving the C ABI
def run_pipeline(pipeline, train, C, N, tw, th, bbox, bits, ref):
    """One pass of a pipeline on footprint records `bbox` [C*N, 4] uint32 and depth bit patterns `bits` [C*N] uint32.  Output
    buffers are sized from the reference and pre-filled with -1; workspace and key buffers start as zeros, so that a sort which
    loses a key hands on flatten id 0 -- a wrong list the test reports -- rather than whatever the memory held.  Returns the
    arrays as int64 NumPy + the info words."""
    from easy_gaussian_splatting_amd import _native as nat
    L, d = nat.lib(), dev()
    tiles, I = tw * th, ref["I"]
    i32 = dict(dtype=torch.int32, device=d)
    P = lambda x: None if x is None else x.data_ptr()
    bb = torch.from_numpy(np.array(bbox, dtype=np.uint32).view(np.int32)).to(d)
    dep = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32)).to(d)
    off = torch.full((C * tiles + 1,), -1, **i32); boff = torch.full((C * tiles + 1,), -1, **i32)
    order = torch.full((C * tiles,), -1, **i32); cum = torch.full((C * N,), -1, **i32)
    fid = torch.full((max(I, 1),), -1, **i32); ids = torch.full((max(I, 1),), -1, dtype=torch.int64, device=d)
    slots = torch.full((max(I, 1),), -1, **i32) if train else None
    slot_gid = None
    info = torch.zeros((nat.GS_INFO_WORDS,), dtype=torch.int64, device=d)
    host = (ct.c_int64 * 8)()
    st = torch.cuda.current_stream().cuda_stream
    if pipeline == "tiles":
        ws = torch.zeros((int(L.gs_bin_workspace_bytes(C, N, tw, th)),), dtype=torch.uint8, device=d)
        nat.check(L.gs_bin_count(st, C, N, tw, th, P(bb), P(ws), ws.numel(), P(off), P(boff), P(order), P(info), host), "gs_bin_count")
        assert host[3] == 0 and host[0] == I and host[2] == ref["longest"], list(host)
        keys = torch.zeros((max(I, 1),), dtype=torch.int64, device=d)
        slot_gid = torch.full((max(I, 1),), -1, **i32) if train else None
        nat.check(L.gs_bin_emit_sort(st, C, N, tw, th, P(bb), P(dep), P(ws), ws.numel(), P(off), I, ref["longest"], P(keys), P(slot_gid),
                                     P(cum), P(ids), P(fid), P(slots)), "gs_bin_emit_sort")
    else:
        shift = int(pipeline[-1])
        coarse = BR.coarse_counts(C, N, tw, th, shift, bbox)
        cap, list_cap = int(coarse.sum()), int(coarse.max())
        keys = torch.zeros((max(cap, 1),), dtype=torch.int64, device=d)
        ws = torch.zeros((int(L.gs_bins_workspace_bytes(C, N, tw, th, shift, cap)),), dtype=torch.uint8, device=d)
        nat.check(L.gs_bins_count(st, C, N, tw, th, shift, P(bb), P(dep), P(ws), ws.numel(), P(keys), cap, list_cap, P(cum), P(off), P(boff),
                                  P(order), P(info), host), "gs_bins_count")
        assert host[3] == 0 and host[0] == I and host[4] == cap and host[5] == list_cap, list(host)
        nat.check(L.gs_bins_lists(st, C, N, tw, th, shift, P(bb), P(ws), ws.numel(), P(keys), cap, P(cum), P(off), P(ids), P(fid), P(slots),
                                  P(info)), "gs_bins_lists")
    torch.cuda.synchronize()
    npy = lambda t: None if t is None else t.cpu().numpy().astype(np.int64)
    return dict(isect_offsets=npy(off), bucket_offsets=npy(boff), tile_order=npy(order), cum_tiles=npy(cum), flatten_ids=npy(fid)[:I],
                isect_ids=npy(ids)[:I], slots=None if slots is None else npy(slots)[:I],
                slot_gid=None if slot_gid is None else npy(slot_gid)[:I], info=npy(info))


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return f"{bad.size} of {want.size} differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}" if bad.size else ""


def check_against_reference(out, ref, what):
    assert out["info"][3] == 0, (what, out["info"])
    assert [int(v) for v in out["info"][:3]] == [ref["I"], ref["n_buckets"], ref["longest"]], (what, out["info"])
    for k in ("isect_offsets", "bucket_offsets", "cum_tiles", "flatten_ids", "isect_ids"):
        assert out[k].shape == ref[k].shape and np.array_equal(out[k], ref[k]), (what, k, first_difference(out[k], ref[k]))
    assert np.array_equal(np.sort(out["tile_order"]), np.arange(out["tile_order"].size)), (what, "tile_order is a permutation of the lists")
    if out["slots"] is not None:
        assert np.array_equal(out["slots"], ref["slots"]), (what, "slots", first_difference(out["slots"], ref["slots"]))
        assert np.array_equal(np.sort(out["slots"]), np.arange(ref["I"])), (what, "slots are a permutation of 0 .. I-1")
    if out["slot_gid"] is not None:
        assert np.array_equal(out["slot_gid"][out["slots"]], out["flatten_ids"]), (what, "slot_gid[slots] == flatten_ids")


def check_pipeline(pipeline, C, N, tw, th, bbox, bits, ref, what):
    for train in (True, False):
        out = run_pipeline(pipeline, train, C, N, tw, th, bbox, bits, ref)
        check_against_reference(out, ref, (what, pipeline, "training lists" if train else "inference lists"))


# ------------------------------------------------------------------------------------------------ A: boundary lengths
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385, 24577, 65535, 65536,
           65537, 70001)
A_TW, A_TH = 19, 18   # 5 x 5 bins of 4 x 4 tiles, 10 x 9 of 2 x 2: ragged at both bin sizes


@functools.lru_cache(maxsize=1)
def scene_a():
    """One list per boundary length: one-tile footprints, one populated tile per 4x4-tile bin (hence per 2x2-tile bin) at a
    position inside the bin that changes from bin to bin; the Gaussians of every list are spread over the whole index range
    (a random permutation), so every binning group feeds every list."""
    tile_of = []
    for b in range(len(LENGTHS)):
        bx, by = b % 5, b // 5
        px, py = (3 * b + by) % min(4, A_TW - 4 * bx), (4 * b + 1 + b // 3) % min(4, A_TH - 4 * by)   # (all 16 positions occur)
        tile_of.append((4 * by + py) * A_TW + 4 * bx + px)
    tile = np.random.default_rng(2024).permutation(np.repeat(np.asarray(tile_of), LENGTHS))
    bbox = BR.one_tile_footprints(tile, A_TW)
    bbox.setflags(write=False)
    return tile.size, bbox, tile_of


@functools.lru_cache(maxsize=2)
def scene_a_reference(pattern):
    N, bbox, _ = scene_a()
    bits = BR.depth_bits(pattern, N, np.random.default_rng(BR.DEPTH_PATTERNS.index(pattern)))
    ref = BR.reference(1, N, A_TW, A_TH, bbox, bits)
    for v in list(ref.values()) + [bits]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return bits, ref


def test_boundary_scene_holds_every_length_in_both_pipelines():
    """The generator's promise, from the reference's own counts: per-tile lists AND the bin lists of both bin sizes have
    exactly the boundary lengths, the populated tile moves inside its bin, and every list draws on the whole index range."""
    N, bbox, tile_of = scene_a()
    _, ref = scene_a_reference("equal")
    assert sorted(ref["counts"][ref["counts"] > 0]) == sorted(LENGTHS) and N == sum(LENGTHS)
    for shift in (1, 2):
        coarse = BR.coarse_counts(1, N, A_TW, A_TH, shift, bbox)
        assert sorted(coarse[coarse > 0]) == sorted(LENGTHS), shift
        B = 1 << shift
        assert len({(t % A_TW % B, t // A_TW % B) for t in tile_of}) == B * B, "every position inside a bin occurs"
    chunks1, chunks2 = {-(-n // 1024) for n in LENGTHS}, {-(-n // 2048) for n in LENGTHS}
    assert {1, 2} < chunks1 and {1, 2} < chunks2, "refinement chunk counts of 1, 2 and many"
    off, fid = ref["isect_offsets"], ref["flatten_ids"]
    for t in np.flatnonzero(ref["counts"] >= 255):
        ids = fid[off[t]: off[t + 1]]
        assert ids.min() < N // 8 and ids.max() > N - N // 8, "a list's Gaussians are spread over the index range"


@pytest.mark.parametrize("pattern", BR.DEPTH_PATTERNS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_every_boundary_length_sorts_exactly(pipeline, pattern):
    """Lists of exactly 1 .. 70001 keys (the edges of the wave slices, of the three LDS radix classes, of the 8192-key segments
    and of the rank merge, and the global network beyond) under every depth pattern: all equal, few distinct values, one or
    two varying bytes (radix passes skipped singly, in a row, after a pass that moved the keys), uniform, descending."""
    N, bbox, _ = scene_a()
    bits, ref = scene_a_reference(pattern)
    check_pipeline(pipeline, 1, N, A_TW, A_TH, bbox, bits, ref, pattern)


# ------------------------------------------------------------------------------------------------ B: mixed footprints
@functools.lru_cache(maxsize=None)
def scene_b_footprints(C, N, tw, th):
    rng = np.random.default_rng(1000 * C + N + tw)
    per_cam = [BR.mixed_footprints(rng, N, tw, th, zero_frac=0.3 if N > 1 else 0.0, zero_ends=True) for _ in range(C)]
    bbox, kind = np.concatenate([b for b, _ in per_cam]), np.concatenate([k for _, k in per_cam])
    if N == 1 and C == 2:   # (a single Gaussian can not be both listed and the zero-count first and last one: it is listed by
        bbox[1] = 0         #  camera 0 and not by camera 1, whose lists are all empty)
    bbox.setflags(write=False)
    return bbox, kind


# (7 x 13: room for 4 x 8 masks; 25 x 23: 13 x 12 bins of 2 x 2 tiles, 7 x 6 of 4 x 4 -- ragged at both sizes, and room for
#  footprints of more than 32 BINS, which the wave-cooperative branch of the coarse walk takes)
B_CASES = [(C, N, 13, 7) for N in (1, 4095, 4096, 4097, 8193) for C in (1, 2)] + [(2, 4097, 7, 13), (1, 4097, 25, 23), (2, 1025, 25, 23)]


def bins_touched(bbox, shift):
    """Bins of (1 << shift)^2 tiles that the rectangle of every listed footprint touches."""
    x0, x1, y0, y1, _, cnt = BR.unpack(bbox)
    r = (1 << shift) - 1
    return ((((x1 + r) >> shift) - (x0 >> shift)) * (((y1 + r) >> shift) - (y0 >> shift)))[cnt > 0]


@pytest.mark.parametrize("pattern", ["k7", "uniform"])
@pytest.mark.parametrize("C,N,tw,th", B_CASES)
def test_mixed_footprints_hand_off_structures(C, N, tw, th, pattern):
    """Every footprint kind (one tile, sparse masks up to exactly 32 tiles, full rectangles from 33 tiles, the whole grid, 30 % of
    zero-count records with the first and the last Gaussian among them), N at the binning-group edges, tile grids that neither
    bin size divides (25 x 23: footprints of more than 32 coarse bins at both bin sizes), one and two cameras with footprints and
    depths of their own: each pipeline and list kind against the reference -- offsets, bucket offsets, {I, n_buckets, longest}, cum_tiles, slots, slot_gid, flatten ids, isect ids."""
    bbox, kind = scene_b_footprints(C, N, tw, th)
    if N > 1:
        kinds = {BR.FOOTPRINT_KINDS[k] for k in kind}
        assert kinds >= {"one", "mask", "full", "grid", "zero"} and ("mask_8x4" in kinds or "mask_4x8" in kinds)
        cnt = bbox[:, 3].reshape(C, N)
        assert np.all(cnt[:, 0] == 0) and np.all(cnt[:, -1] == 0) and 0.25 < (cnt == 0).mean() < 0.35
        assert (cnt[:, 1:-1] == 0).any() and ((bbox[:, 3] == 32) | (bbox[:, 3] == 33)).any()
        for shift in (1, 2):   # a grid of more than 32 bins: both branches of the coarse walk (a lane's own loop, the whole wave)
            if -(-tw >> shift) * -(-th >> shift) > BR.MASK_TILES:
                nb = bins_touched(bbox, shift)
                assert (nb > BR.MASK_TILES).any() and ((nb >= 2) & (nb <= BR.MASK_TILES)).any(), (shift, nb.max())
    bits = BR.depth_bits(pattern, C * N, np.random.default_rng(7 * N + C))
    ref = BR.reference(C, N, tw, th, bbox, bits)
    if C == 2 and N > 1:
        assert not np.array_equal(bbox[:N], bbox[N:]) and ref["isect_ids"].max() >> (32 + (tw * th).bit_length()) == 1
    for pipeline in PIPELINES:
        check_pipeline(pipeline, C, N, tw, th, bbox, bits, ref, (C, N, pattern))


# ------------------------------------------------------------------------------------------------ C: the group cap
def test_group_cap_one_more_gaussian_than_256_full_groups():
    """N = 256 * 4096 + 1: the smallest N at which the number of binning groups stays at its cap and the Gaussians per group grow
    past 4096 instead.  One-tile footprints over 16 x 16 tiles, 300 distinct depths; inference lists of both pipelines."""
    from easy_gaussian_splatting_amd import _native as nat
    N, tw, th = 256 * 4096 + 1, 16, 16
    assert nat.lib().gs_bin_groups(N) == nat.lib().gs_bin_groups(N - 1) == 256 and nat.lib().gs_bin_groups(255 * 4096) == 255
    rng = np.random.default_rng(256)
    bbox = BR.one_tile_footprints(rng.integers(0, tw * th, N), tw)
    bits = BR.depth_bits("k300", N, rng)
    ref = BR.reference(1, N, tw, th, bbox, bits, stable_passes=True)
    for pipeline in PIPELINES:
        out = run_pipeline(pipeline, False, 1, N, tw, th, bbox, bits, ref)
        assert out["info"][3] == 0
        for k in ("isect_offsets", "flatten_ids"):
            assert np.array_equal(out[k], ref[k]), (pipeline, k, first_difference(out[k], ref[k]))


# ------------------------------------------------------------------------------------------------ D: the public path
VARIANTS = ("clones", "depths_snapped_to_8", "depth_bytes_0_and_2")


def cloned_scene(n, variant):
    """dense_scene concatenated with itself: every Gaussian has an exact clone n indices later, as after a densification, so
    every depth occurs (at least) twice in every list.  The camera has the identity rotation and sits 4 behind the origin, so
    the depth of a mean is z + 4, exactly where that sum is exact.  "depths_snapped_to_8": z rounded to 8 values, the depths
    take 8 values (ties between neighbours in index, not only between a clone and its parent: a parent is emitted before its
    clone whatever the kernel does, neighbours are not).  "depth_bytes_0_and_2": z = d - 4 for depths d in [4, 4.5) whose bit
    patterns differ in bytes 0 and 2 only -- the radix pass on byte 1 is skipped AFTER the pass on byte 0 moved the keys."""
    sc = dense_scene(n, 100 + n)
    assert np.array_equal(sc["viewmats"][0], np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4], [0, 0, 0, 1]], np.float32))
    sc["means"] = sc["means"].copy()
    z = sc["means"][:, 2].astype(np.float64)
    if variant == "depths_snapped_to_8":
        lo, hi = z.min(), z.max()
        sc["means"][:, 2] = (lo + np.round((z - lo) / (hi - lo) * 7) * (hi - lo) / 7).astype(np.float32)
    elif variant == "depth_bytes_0_and_2":
        rng = np.random.default_rng(n)
        bits = 0x40805B00 | (rng.integers(0, 16, n, dtype=np.int64) << 16) | rng.integers(0, 256, n, dtype=np.int64)
        sc["means"][:, 2] = bits.astype(np.uint32).view(np.float32) - np.float32(4.0)   # (exact: Sterbenz)
    per_gaussian = ("means", "quats", "scales", "opacities", "shs")
    return {k: (np.concatenate([v, v]) if k in per_gaussian else v) for k, v in sc.items()}


@pytest.mark.parametrize("grad", [True, False], ids=["training_lists", "no_grad"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,lo,hi", [(1500, 1024, 4096), (5000, 8192, 16384), (10000, 16384, 65536)])
def test_cloned_gaussians_through_rasterization(n, lo, hi, variant, grad, monkeypatch):
    """Exact depth ties as a densification leaves them, through rasterization(): the doubled lists fall in the 4096 class, in two
    8192-key segments and in three; per-tile and two-level binning, training and inference lists.  Inside every tile the ids
    are strictly ordered by (depth bits, flatten id), and both binning modes render the same image bit for bit.  (See
    cloned_scene for what each variant reaches.)"""
    from easy_gaussian_splatting_amd import rendering
    monkeypatch.setenv("GS_EAGER_ISECT_IDS", "1")   # the kernels write isect_ids (default: meta derives them on demand)
    sc = cloned_scene(n, variant)
    d = dev()
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(d) for k, v in sc.items() if isinstance(v, np.ndarray)}
    images = {}
    for binning in ("tiles", "bins"):
        monkeypatch.setenv("GS_BINNING", binning)
        rendering.reset_hints()
        ins = [t[k].clone().requires_grad_(grad) for k in ("means", "quats", "scales", "opacities", "shs")]
        with contextlib.nullcontext() if grad else torch.no_grad():
            img, alpha, meta = rendering.rasterization(*ins, t["viewmats"], t["Ks"], int(sc["width"]), int(sc["height"]), sh_degree=0,
                                                       packed=False, backgrounds=t["backgrounds"], _tile_culling="gsplat")
        assert img.requires_grad == grad and rendering.last_binning(d) == binning
        off = meta["isect_offsets"].reshape(-1).cpu().numpy().astype(np.int64)
        fid = meta["flatten_ids"].cpu().numpy().astype(np.int64)
        ids = meta["isect_ids"].cpu().numpy()
        counts = np.diff(np.append(off, fid.size))
        assert lo < counts.max() <= hi, counts.max()
        depth_bits = meta["depths"].reshape(-1).cpu().numpy().view(np.int32).astype(np.int64)
        assert np.array_equal(depth_bits[:n], depth_bits[n:]), "a clone has its parent's depth"
        listed = depth_bits[meta["radii"].reshape(-1).cpu().numpy() > 0]
        if variant == "depths_snapped_to_8":
            assert np.unique(listed).size <= 8
        if variant == "depth_bytes_0_and_2":
            assert np.unique(listed & 0xFF00FF00).size == 1 and np.unique(listed & 0xFF).size > 200 and np.unique(listed >> 16 & 0xFF).size == 16
        assert fid.size == int(meta["tiles_per_gauss"].sum())
        for tl in range(off.size):
            seg = fid[off[tl]: off[tl] + counts[tl]]
            key = depth_bits[seg] * (1 << 32) + seg
            assert np.all(np.diff(key) > 0), f"{binning}: tile {tl} not in (depth, id) order"
            assert np.array_equal(ids[off[tl]: off[tl] + counts[tl]] & 0xFFFFFFFF, depth_bits[seg])
        images[binning] = (img.detach(), alpha.detach(), fid)
    assert torch.equal(images["tiles"][0], images["bins"][0]) and torch.equal(images["tiles"][1], images["bins"][1])
    assert np.array_equal(images["tiles"][2], images["bins"][2])
