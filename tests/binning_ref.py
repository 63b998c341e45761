"""Plain NumPy reference of the tile binning (csrc/gs_binning.hip) and the generators of its edge-case inputs.

No import of the project: the footprint record layout is restated here (the projection's: x0 | x1 << 16, y0 | y1 << 16,
tile mask, count; a rectangle of <= 32 tiles carries a row-major bit per tile and count = popcount, a larger one is
full and count = its area, count = 0 is not listed) and GS_BUCKET is read from include/gs_raster.h.

The contract: every (Gaussian, tile) pair exactly once; lists ordered by (camera, tile), inside a tile by
(depth bits, flatten id) -- what ONE stable sort of (camera | tile | depth) keys emitted in flatten order yields.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "gs_raster.h")) as _f:
    GS_BUCKET = int(re.search(r"^#define\s+GS_BUCKET\s+(\d+)", _f.read(), re.M).group(1))

MASK_TILES = 32   # rectangles up to this many tiles carry a bit mask
DEPTH_LO, DEPTH_HI = 0x00800000, 0x7F7FFFFF   # positive normal floats, as bit patterns


# ------------------------------------------------------------------------------------------------ reference
def unpack(bbox):
    b = np.asarray(bbox).astype(np.int64) & 0xFFFFFFFF
    return b[:, 0] & 0xFFFF, b[:, 0] >> 16, b[:, 1] & 0xFFFF, b[:, 1] >> 16, b[:, 2], b[:, 3]


def _popcount(v):
    v = v.astype(np.uint64)
    n = np.zeros(v.shape, np.int64)
    for i in range(32):
        n += ((v >> np.uint64(i)) & np.uint64(1)).astype(np.int64)
    return n


def expand_pairs(C, N, tw, th, bbox):
    """Every (Gaussian, tile) pair of the footprints: flatten id, tile (inside its camera), rank of the tile inside the
    footprint (row-major over the rectangle, or over the set mask bits).  Unordered."""
    x0, x1, y0, y1, mask, cnt = unpack(bbox)
    assert x0.size == C * N
    w, rect = x1 - x0, (x1 - x0) * (y1 - y0)
    live = cnt > 0
    assert np.all(x1[live] <= tw) and np.all(y1[live] <= th) and np.all(rect[live] > 0), "footprint outside the tile grid"
    small = live & (rect <= MASK_TILES)
    big = live & (rect > MASK_TILES)
    assert np.array_equal(cnt[big], rect[big]), "a rectangle of more than 32 tiles is full"
    assert np.all(mask[small] < (np.int64(1) << rect[small])) and np.array_equal(_popcount(mask[small]), cnt[small]), \
        "count = popcount of a mask inside the rectangle"
    fs, ts, ks = [], [], []
    sf = np.flatnonzero(small)
    below = np.zeros(sf.size, np.int64)   # set bits below bit i
    for i in range(MASK_TILES):
        hit = ((mask[sf] >> i) & 1).astype(bool)
        f = sf[hit]
        fs.append(f); ts.append((y0[f] + i // w[f]) * tw + x0[f] + i % w[f]); ks.append(below[hit])
        below = below + hit
    bf = np.flatnonzero(big)
    f = np.repeat(bf, rect[bf])
    i = np.arange(f.size, dtype=np.int64) - np.repeat(np.cumsum(rect[bf]) - rect[bf], rect[bf])
    fs.append(f); ts.append((y0[f] + i // w[f]) * tw + x0[f] + i % w[f]); ks.append(i)
    return np.concatenate(fs), np.concatenate(ts), np.concatenate(ks)


def reference(C, N, tw, th, bbox, depth_bits, stable_passes=False):
    """The arrays the binning hands on.  `stable_passes`: three stable single-key sorts instead of one three-key lexsort
    (the same order, faster on a million entries)."""
    tiles = tw * th
    depth_bits = np.asarray(depth_bits).astype(np.int64) & 0xFFFFFFFF
    f, t, k = expand_pairs(C, N, tw, th, bbox)
    cam = f // max(N, 1)
    list_id = cam * tiles + t
    if stable_passes:
        order = np.argsort(f, kind="stable")
        order = order[np.argsort(depth_bits[f[order]], kind="stable")]
        order = order[np.argsort(list_id[order], kind="stable")]
    else:
        order = np.lexsort((f, depth_bits[f], list_id))
    f, t, k, cam, list_id = f[order], t[order], k[order], cam[order], list_id[order]
    counts = np.bincount(list_id, minlength=C * tiles).astype(np.int64)
    cnt = unpack(bbox)[5]
    cum = np.cumsum(cnt) - cnt
    tile_bits = int(tiles).bit_length()
    return {
        "counts": counts,
        "isect_offsets": np.concatenate([[0], np.cumsum(counts)]),
        "bucket_offsets": np.concatenate([[0], np.cumsum((counts + GS_BUCKET - 1) // GS_BUCKET)]),
        "I": int(counts.sum()),
        "n_buckets": int(((counts + GS_BUCKET - 1) // GS_BUCKET).sum()),
        "longest": int(counts.max()) if counts.size else 0,
        "flatten_ids": f,
        "isect_ids": (cam << (32 + tile_bits)) | (t << 32) | depth_bits[f],
        "cum_tiles": cum,
        "slots": cum[f] + k,
    }


def coarse_counts(C, N, tw, th, shift, bbox):
    """Entries of every coarse bin ((1 << shift)^2 tiles) of the two-level pipeline: a Gaussian enters every bin its
    RECTANGLE touches, mask or not."""
    x0, x1, y0, y1, _, cnt = unpack(bbox)
    B = 1 << shift
    bw, bh = (tw + B - 1) // B, (th + B - 1) // B
    live = np.flatnonzero(cnt > 0)
    cx0, cy0 = x0[live] >> shift, y0[live] >> shift
    cw, chh = ((x1[live] + B - 1) >> shift) - cx0, ((y1[live] + B - 1) >> shift) - cy0
    n = cw * chh
    g = np.repeat(np.arange(live.size), n)
    i = np.arange(g.size, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    b = (live[g] // max(N, 1)) * (bw * bh) + (cy0[g] + i // cw[g]) * bw + cx0[g] + i % cw[g]
    return np.bincount(b, minlength=C * bw * bh).astype(np.int64)


def brute_force(C, N, tw, th, bbox, depth_bits):
    """The same lists by a plain Python loop (per tile, `sorted` on tuples): the reference's reference, small inputs only."""
    tiles = tw * th
    lists = [[] for _ in range(C * tiles)]
    cum, run = [], 0
    for f in range(C * N):
        bx, by, mask, cnt = (int(v) & 0xFFFFFFFF for v in bbox[f])
        cum.append(run)
        run += cnt
        if cnt == 0:
            continue
        x0, x1, y0, y1 = bx & 0xFFFF, bx >> 16, by & 0xFFFF, by >> 16
        w, rect, k = x1 - x0, (x1 - x0) * (y1 - y0), 0
        for i in range(rect):
            if rect > MASK_TILES or (mask >> i) & 1:
                tile = (y0 + i // w) * tw + x0 + i % w
                lists[(f // N) * tiles + tile].append((int(depth_bits[f]) & 0xFFFFFFFF, f, cum[f] + k))
                k += 1
        assert k == cnt
    offsets, fid, ids, slots = [0], [], [], []
    tile_bits = tiles.bit_length()
    for li, entries in enumerate(lists):
        for d, f, s in sorted(entries):
            fid.append(f); slots.append(s)
            ids.append(((li // tiles) << (32 + tile_bits)) | ((li % tiles) << 32) | d)
        offsets.append(len(fid))
    return {"isect_offsets": offsets, "flatten_ids": fid, "isect_ids": ids, "slots": slots, "cum_tiles": cum}


# ------------------------------------------------------------------------------------------------ footprints
def pack(x0, x1, y0, y1, mask=None):
    """Footprint records of rectangles [x0, x1) x [y0, y1); `mask`: the row-major tile bits of the rectangles of <= 32 tiles
    (default: all of the rectangle)."""
    x0, x1, y0, y1 = (np.asarray(v, np.int64) for v in (x0, x1, y0, y1))
    rect = (x1 - x0) * (y1 - y0)
    full = (np.int64(1) << np.minimum(rect, MASK_TILES)) - 1
    m = full if mask is None else np.asarray(mask, np.int64) & full
    m = np.where(rect > MASK_TILES, 0xFFFFFFFF, m)
    cnt = np.where(rect > MASK_TILES, rect, _popcount(m))
    return np.stack([x0 | (x1 << 16), y0 | (y1 << 16), m, cnt], axis=1).astype(np.uint32)


def one_tile_footprints(tile, tw):
    tile = np.asarray(tile, np.int64)
    return pack(tile % tw, tile % tw + 1, tile // tw, tile // tw + 1)


FOOTPRINT_KINDS = ("one", "mask", "mask_8x4", "mask_4x8", "full", "grid", "zero")


def mixed_footprints(rng, n, tw, th, zero_frac=0.0, zero_ends=False):
    """`n` records over every footprint kind: one tile; sparse masks in rectangles of <= 32 tiles (8x4 and 4x8 -- exactly 32
    -- among them); full rectangles of >= 33 tiles; the whole grid; zero-count records (all-zero words, or a rectangle
    whose mask is empty).  Returns the records and the kind of each."""
    live_kinds = [k for k in FOOTPRINT_KINDS[:-1]
                  if not (k == "mask_8x4" and (tw < 8 or th < 4)) and not (k == "mask_4x8" and (tw < 4 or th < 8))
                  and not (k == "full" and tw * th <= MASK_TILES)]
    kind = rng.choice(len(live_kinds), n)
    kind = np.array([FOOTPRINT_KINDS.index(live_kinds[i]) for i in kind])
    zero = rng.random(n) < zero_frac
    if zero_ends and n >= 3:
        zero[0] = zero[-1] = True
    kind[zero] = FOOTPRINT_KINDS.index("zero")
    w, h = np.ones(n, np.int64), np.ones(n, np.int64)
    mask = rng.integers(1, 1 << 32, n, dtype=np.int64)   # (never empty after the cut to the rectangle: see below)
    for i in range(n):
        k = FOOTPRINT_KINDS[kind[i]]
        if k in ("mask", "zero"):
            w[i] = rng.integers(1, min(tw, MASK_TILES) + 1)
            h[i] = rng.integers(1, min(th, MASK_TILES // w[i]) + 1)
        elif k == "mask_8x4":
            w[i], h[i] = 8, 4
        elif k == "mask_4x8":
            w[i], h[i] = 4, 8
        elif k == "full":
            while w[i] * h[i] <= MASK_TILES:
                w[i], h[i] = rng.integers(1, tw + 1), rng.integers(1, th + 1)
        elif k == "grid":
            w[i], h[i] = tw, th
    x0 = (rng.random(n) * (tw - w + 1)).astype(np.int64)
    y0 = (rng.random(n) * (th - h + 1)).astype(np.int64)
    rect = w * h
    full = (np.int64(1) << np.minimum(rect, MASK_TILES)) - 1
    mask &= full
    mask = np.where(mask == 0, np.int64(1) << (rect - 1).clip(max=31), mask)   # a live masked footprint keeps >= 1 tile
    mask = np.where((rng.random(n) < 0.25) | (kind == FOOTPRINT_KINDS.index("grid")), full, mask)   # some masks are full
    is_zero = kind == FOOTPRINT_KINDS.index("zero")
    mask = np.where(is_zero, 0, mask)
    out = pack(x0, x0 + w, y0, y0 + h, mask)
    blank = is_zero & (rng.random(n) < 0.5)   # the other form of "not listed": what an invisible Gaussian leaves
    out[blank] = 0
    assert np.all(out[is_zero, 3] == 0) and np.all(out[~is_zero, 3] > 0)
    return out, kind


# ------------------------------------------------------------------------------------------------ depth patterns
DEPTH_PATTERNS = ("equal", "k2", "k7", "k300", "byte0", "byte1", "byte2", "byte3", "bytes02", "bytes13", "uniform",
                  "descending", "descending_runs5")
_BASE = 0x41925B37   # 18.29...: byte 2 has its top bit set, so any byte 3 in 0 .. 0x7e leaves a positive normal float


def _vary(rng, n, which):
    bits = np.full(n, _BASE, np.int64)
    for b in which:
        v = rng.integers(0, 0x7F if b == 3 else 0x100, n, dtype=np.int64)
        bits = (bits & ~(np.int64(0xFF) << (8 * b))) | (v << (8 * b))
    return bits


def depth_bits(pattern, n, rng):
    """`n` depths as raw uint32 bit patterns, all of them positive normal floats."""
    if pattern == "equal":
        bits = np.full(n, 0x40000000, np.int64)
    elif pattern in ("k2", "k7", "k300"):
        vals = rng.choice(DEPTH_HI - DEPTH_LO + 1, int(pattern[1:]), replace=False).astype(np.int64) + DEPTH_LO
        bits = vals[rng.integers(0, vals.size, n)]
    elif pattern.startswith("byte"):
        bits = _vary(rng, n, [int(c) for c in pattern.lstrip("bytes")])
    elif pattern == "uniform":
        bits = rng.integers(DEPTH_LO, DEPTH_HI + 1, n, dtype=np.int64)
    elif pattern == "descending":       # strictly, in flatten id; the step moves bytes 0 and 1 (and 2, more slowly)
        bits = 0x7F000000 - 257 * np.arange(n, dtype=np.int64)
    elif pattern == "descending_runs5":
        bits = 0x7F000000 - 257 * (np.arange(n, dtype=np.int64) // 5)
    else:
        raise ValueError(pattern)
    assert bits.size == n and (n == 0 or (bits.min() >= DEPTH_LO and bits.max() <= DEPTH_HI)), pattern
    return bits.astype(np.uint32)
