"""tests/binning_ref.py (the NumPy reference the GPU binning tests compare with) against a brute-force Python loop and
against the lists stored in the committed fixtures.  CPU only."""
import glob
import os

import numpy as np
import pytest

import binning_ref as BR

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# gsplat_*.npz (gsplat's own outputs, tests/golden/make_gsplat_golden.py) join the list the day they are committed; the
# oracle_scene_*.npz fixtures store the same arrays in the same layout
FIXTURES = sorted(os.path.basename(p) for pat in ("oracle_scene_*.npz", "gsplat_*.npz") for p in glob.glob(os.path.join(GOLD, pat)))


def _check_against_brute_force(C, N, tw, th, bbox, bits):
    ref = BR.reference(C, N, tw, th, bbox, bits)
    bf = BR.brute_force(C, N, tw, th, bbox, bits)
    for k in ("isect_offsets", "flatten_ids", "isect_ids", "slots", "cum_tiles"):
        assert np.array_equal(ref[k], np.asarray(bf[k], np.int64)), k
    st = BR.reference(C, N, tw, th, bbox, bits, stable_passes=True)
    for k in ref:
        assert np.array_equal(ref[k], st[k]), k
    I = ref["I"]
    assert I == int(bbox[:, 3].sum()) == ref["isect_offsets"][-1] and ref["longest"] == np.diff(ref["isect_offsets"]).max()
    assert np.array_equal(np.sort(ref["slots"]), np.arange(I)), "the slots are a permutation of the gradient rows"
    assert ref["n_buckets"] == ref["bucket_offsets"][-1] == sum(-(-int(c) // BR.GS_BUCKET) for c in ref["counts"])
    return ref


@pytest.mark.parametrize("pattern", ["equal", "k7", "uniform", "descending_runs5", "byte3"])
@pytest.mark.parametrize("C", [1, 2])
def test_reference_equals_brute_force(C, pattern):
    """~300 Gaussians per camera over a 5 x 3 grid, every footprint kind that fits it, zero-count records, tied depths."""
    rng = np.random.default_rng(11 + C)
    N, tw, th = 301, 5, 3
    bbox, kind = BR.mixed_footprints(rng, C * N, tw, th, zero_frac=0.3, zero_ends=True)
    assert {"one", "mask", "grid", "zero"} <= {BR.FOOTPRINT_KINDS[k] for k in kind}
    _check_against_brute_force(C, N, tw, th, bbox, BR.depth_bits(pattern, C * N, rng))


def test_reference_equals_brute_force_with_every_footprint_kind():
    """A 13 x 9 grid holds what 5 x 3 can not: 8 x 4 and 4 x 8 masks (exactly 32 tiles), full rectangles of >= 33 tiles and a
    whole-grid footprint that is a full rectangle rather than a mask."""
    rng = np.random.default_rng(5)
    C, N, tw, th = 2, 150, 13, 9
    bbox, kind = BR.mixed_footprints(rng, C * N, tw, th, zero_frac=0.2, zero_ends=True)
    assert set(kind) == set(range(len(BR.FOOTPRINT_KINDS)))
    x0, x1, y0, y1, mask, cnt = BR.unpack(bbox)
    rect = (x1 - x0) * (y1 - y0)
    assert ((rect == 32) & (cnt > 0) & (cnt < 32)).any() and ((rect > 32) & (rect < tw * th)).any() and (rect == tw * th).any()
    assert ((cnt == 0) & (rect > 0)).any() and ((cnt == 0) & (rect == 0)).any(), "both forms of a zero-count record"
    ref = _check_against_brute_force(C, N, tw, th, bbox, BR.depth_bits("k2", C * N, rng))
    # the coarse-bin counts, against a loop over the rectangles
    for shift in (1, 2):
        B = 1 << shift
        bw, bh = -(-tw // B), -(-th // B)
        want = np.zeros(C * bw * bh, np.int64)
        for f in range(C * N):
            if cnt[f]:
                for by in range(y0[f] >> shift, ((y1[f] - 1) >> shift) + 1):
                    for bx in range(x0[f] >> shift, ((x1[f] - 1) >> shift) + 1):
                        want[(f // N) * bw * bh + by * bw + bx] += 1
        assert np.array_equal(BR.coarse_counts(C, N, tw, th, shift, bbox), want)
    assert ref["I"] > 0


def test_depth_patterns_are_what_they_say():
    rng = np.random.default_rng(3)
    n = 5000
    byte = lambda v, b: (v.astype(np.int64) >> (8 * b)) & 0xFF
    for p in BR.DEPTH_PATTERNS:
        v = BR.depth_bits(p, n, rng)
        assert v.dtype == np.uint32 and v.min() >= BR.DEPTH_LO and v.max() <= BR.DEPTH_HI
        f = v.view(np.float32)
        assert np.all(np.isfinite(f)) and np.all(f >= np.finfo(np.float32).tiny), p
    assert np.unique(BR.depth_bits("equal", n, rng)).size == 1
    for k in (2, 7, 300):
        assert np.unique(BR.depth_bits(f"k{k}", n, rng)).size == k
    for p, moving in (("byte0", {0}), ("byte1", {1}), ("byte2", {2}), ("byte3", {3}), ("bytes02", {0, 2}), ("bytes13", {1, 3})):
        v = BR.depth_bits(p, n, rng)
        for b in range(4):
            distinct = np.unique(byte(v, b)).size
            assert (distinct > 100) if b in moving else (distinct == 1), (p, b)
    d = BR.depth_bits("descending", n, rng).astype(np.int64)
    assert np.all(np.diff(d) < 0)
    d = BR.depth_bits("descending_runs5", n, rng).astype(np.int64)
    assert np.all(np.diff(d)[np.arange(n - 1) % 5 != 4] == 0) and np.all(np.diff(d)[4::5] < 0)


def _gsplat_rectangles(z, tile=16):
    """The 3-sigma tile rectangles as gsplat's projection cuts them (isect_tiles): centre and radius in tile units, floor /
    ceil, clipped to the grid; radius 0 = not listed."""
    W, H = int(z["width"]), int(z["height"])
    tw, th = -(-W // tile), -(-H // tile)
    m2, radii = z["means2d"], z["radii"].reshape(-1)
    ft = m2.dtype.type
    xy = m2.reshape(-1, 2) / ft(tile)
    r = radii.astype(m2.dtype) / ft(tile)
    x0 = np.clip(np.floor(xy[:, 0] - r), 0, tw).astype(np.int64); x1 = np.clip(np.ceil(xy[:, 0] + r), 0, tw).astype(np.int64)
    y0 = np.clip(np.floor(xy[:, 1] - r), 0, th).astype(np.int64); y1 = np.clip(np.ceil(xy[:, 1] + r), 0, th).astype(np.int64)
    bbox = BR.pack(x0, x1, y0, y1)
    bbox[radii <= 0] = 0
    return tw, th, bbox


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_reproduces_the_fixture_lists(name):
    """Footprints rebuilt from the stored radii / means2d (they must reproduce the stored tiles_per_gauss), depths as stored:
    flatten_ids and isect_offsets bit for bit, and isect_ids where the fixture has them."""
    z = dict(np.load(os.path.join(GOLD, name)))
    C, N = z["radii"].shape
    tw, th, bbox = _gsplat_rectangles(z)
    assert np.array_equal(bbox[:, 3].astype(np.int64), z["tiles_per_gauss"].reshape(-1)), "rebuilt rectangles differ from the fixture's"
    bits = z["depths"].astype(np.float32).reshape(-1).view(np.uint32)
    ref = BR.reference(C, N, tw, th, bbox, bits)
    assert ref["I"] == z["flatten_ids"].size
    assert np.array_equal(ref["flatten_ids"], z["flatten_ids"].astype(np.int64))
    assert np.array_equal(ref["isect_offsets"][:-1], z["isect_offsets"].reshape(-1).astype(np.int64))
    if "isect_ids" in z:
        assert np.array_equal(ref["isect_ids"], z["isect_ids"].astype(np.int64))
