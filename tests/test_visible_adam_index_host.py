"""The quad-to-Gaussians index of the visible Adam step (csrc/gs_visible_index.h) built with the host compiler -- the device's own text --
and held to a walk over the elements: widths {1, 3, 4, 9, 24, 45, 72} (the six groups at SH degrees 0-4 and two widths of other
models), every n_rows in 0..70, every quad -- no GPU."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (1, 3, 4, 9, 24, 45, 72)


@pytest.fixture(scope="module")
def vi(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vi") / "libvisible_index.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "visible_index.cpp")], check=True)
    L = ct.CDLL(so)
    L.vi_quad_rows_all.argtypes, L.vi_quad_rows_all.restype = [ct.c_int64, ct.c_uint32, ct.c_int64, ct.c_void_p], None
    L.vi_quad_rows_one.argtypes, L.vi_quad_rows_one.restype = [ct.c_int64, ct.c_uint32, ct.c_int64, ct.c_void_p], None
    L.vi_quad_row_step.argtypes, L.vi_quad_row_step.restype = [ct.c_uint32, ct.c_uint32, ct.c_uint32], ct.c_uint32
    return L


def _walk(w, n_rows):
    """[(first, last, r, pad)] per quad, from the elements: element e < n_rows * w belongs to Gaussian e // w, the rest to nobody."""
    length = n_rows * w
    out = []
    for q in range((length + 3) // 4):
        owners = [e // w for e in range(4 * q, 4 * q + 4) if e < length]
        out.append((min(owners), max(owners), (4 * q) % w, int(4 * q + 4 > length)))
    return out


@pytest.mark.parametrize("w", WIDTHS)
def test_every_quad_of_every_small_segment(vi, w):
    for n_rows in range(71):
        want = _walk(w, n_rows)
        got = np.full((len(want) + 1, 4), -7, dtype=np.int64)   # (one row of canaries behind the last quad)
        vi.vi_quad_rows_all(len(want), w, n_rows, got.ctypes.data)
        assert (got[-1] == -7).all()
        assert [tuple(r) for r in got[:-1].tolist()] == want, (w, n_rows)
        if want:
            assert got[:-1, 0].min() >= 0 and got[:-1, 1].max() < n_rows, (w, n_rows)   # nobody beyond the last Gaussian
            assert (got[:-1, 1] - got[:-1, 0]).max() <= (3 if w == 1 else 1)
            assert got[:-1, 3].sum() == (1 if (n_rows * w) % 4 else 0) and not got[:-2, 3].any()   # the pad: the last quad's alone


@pytest.mark.parametrize("w", WIDTHS + (2,))
def test_the_owner_of_every_element(vi, w):
    """first + quad_row_step(r, i, w) is the Gaussian of element 4 q + i."""
    for q in range(80):
        e = 4 * q
        for i in range(4):
            assert e // w + vi.vi_quad_row_step(e % w, i, w) == (e + i) // w, (w, q, i)


def test_segments_beyond_32_bits(vi):
    """A segment longer than 2^32 floats takes the 64-bit division: the same answers."""
    for w, n_rows in ((72, 70_000_000), (45, 100_000_003)):
        length = n_rows * w
        assert length > 2 ** 32
        for q in (0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 5, (length + 3) // 4 - 2, (length + 3) // 4 - 1):
            owners = [e // w for e in range(4 * q, 4 * q + 4) if e < length]
            out = np.zeros(4, dtype=np.int64)
            vi.vi_quad_rows_one(q, w, n_rows, out.ctypes.data)
            assert tuple(out.tolist()) == (min(owners), max(owners), (4 * q) % w, int(4 * q + 4 > length)), (w, n_rows, q)
