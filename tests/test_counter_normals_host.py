"""The device's own text of the counter-based draw (csrc/gs_counter_normals.h) built with the host compiler and driven over chosen
arguments: Philox against the published answers and the reference's packing; `log_unit` and `sincos_turn` against numpy over the
edge words (0, 2^32 - 1), the mantissa split, the quadrant boundaries and random arguments; the normals of chosen words against
tests/mcmc_step_ref.py.  A Philox output reaches each of those words once in 2^32 draws, so no GPU test meets them."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import mcmc_step_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ULP = 2.0 ** -52
EDGE_WORDS = [0, 1, 2, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 3 * 2 ** 30 - 1, 3 * 2 ** 30, 3 * 2 ** 30 + 1,
              2 ** 29, 7 * 2 ** 29 - 1, 7 * 2 ** 29, 2 ** 32 - 2, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def cn(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cn") / "libcounter_normals.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "counter_normals.cpp")], check=True)
    L = ct.CDLL(so)
    P, Q, U, D = ct.c_void_p, ct.c_int64, ct.c_uint64, ct.c_double
    L.cn_philox.argtypes, L.cn_philox.restype = [U, U, U, P], None
    L.cn_counter_normals.argtypes, L.cn_counter_normals.restype = [U, U, U, P], None
    L.cn_log_unit_many.argtypes, L.cn_log_unit_many.restype = [Q, P, P], None
    L.cn_sincos_turn_many.argtypes, L.cn_sincos_turn_many.restype = [Q, P, P, P], None
    L.cn_normals_of_words_many.argtypes, L.cn_normals_of_words_many.restype = [Q, P, P], None
    return L


def philox(L, n, t, seed):
    out = (ct.c_uint32 * 4)()
    L.cn_philox(n, t, seed, out)
    return tuple(out)


def unit_of(x):
    return (np.asarray(x, dtype=np.float64) + 0.5) * 2.0 ** -32


def test_device_philox_known_answers_and_packing(cn):
    h = lambda w: " ".join(f"{x:08x}" for x in w)   # noqa: E731
    f = 2 ** 64 - 1
    assert h(philox(cn, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert h(philox(cn, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert h(philox(cn, 0x85A308D3243F6A88, 0x0370734413198A2E, 0x299F31D0A4093822)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    for n, t, seed in ((7, 2 ** 32 + 5, 2 ** 63 + 12345), (2 ** 32 + 9, 1, 3), (4099, 2 ** 32 - 1, 0)):
        assert philox(cn, n, t, seed) == R.philox4x32_10(*R.counter_key(n, t, seed)), (n, t, seed)


def test_log_unit_against_numpy(cn):
    """fdlibm's log is below 1 ulp, numpy's too: 2 ulp between them, relative (ln u never comes near 0 more than 2^-33)."""
    g = np.random.default_rng(0)
    split = 0.70710678118654752440   # where the mantissa is doubled
    words = np.concatenate([np.array(EDGE_WORDS, dtype=np.float64), 2.0 ** np.arange(1, 32), 2.0 ** np.arange(1, 32) - 1,
                            np.floor(split * 2.0 ** np.arange(20, 33)), np.floor(split * 2.0 ** np.arange(20, 33)) + 1,
                            g.integers(0, 2 ** 32, 200_000).astype(np.float64)])
    u = np.ascontiguousarray(unit_of(words))
    assert u.min() == 2.0 ** -33 and u.max() == 1.0 - 2.0 ** -33
    got = np.empty_like(u)
    cn.cn_log_unit_many(u.size, u.ctypes.data, got.ctypes.data)
    err = np.abs(got - np.log(u)) / np.abs(np.log(u))
    print(f"[counter normals] log_unit: {err.max() / ULP:.2f} ulp from numpy at worst over {u.size} arguments")
    assert err.max() <= 2 * ULP


def test_sincos_turn_against_numpy(cn):
    """a = fl(2 pi u) as the draw forms it.  fdlibm's kernels and numpy are below 1 ulp each and the two-constant reduction adds
    less than one: 3 ulp, relative to the value -- near a zero of the function too (the smallest |cos| a word can reach is 7e-10)."""
    g = np.random.default_rng(1)
    words = np.concatenate([np.array(EDGE_WORDS, dtype=np.float64), 2.0 ** 29 * np.arange(1, 8) - 1, 2.0 ** 29 * np.arange(1, 8),
                            g.integers(0, 2 ** 32, 200_000).astype(np.float64)])
    a = np.ascontiguousarray(2.0 * np.pi * unit_of(words))
    sn, cs = np.empty_like(a), np.empty_like(a)
    cn.cn_sincos_turn_many(a.size, a.ctypes.data, sn.ctypes.data, cs.ctypes.data)
    e_s, e_c = np.abs(sn - np.sin(a)) / np.abs(np.sin(a)), np.abs(cs - np.cos(a)) / np.abs(np.cos(a))
    print(f"[counter normals] sincos_turn: sin {e_s.max() / ULP:.2f} ulp, cos {e_c.max() / ULP:.2f} ulp from numpy at worst over {a.size}")
    assert np.abs(np.cos(a)).min() < 1e-9 and np.abs(np.sin(a)).min() < 1e-9   # (the zeros are among the arguments)
    assert e_s.max() <= 3 * ULP and e_c.max() <= 3 * ULP


def test_normals_of_chosen_words_against_the_reference(cn):
    """Every pair of edge words as (x0, x1) and as (x2, x3), then random words: at most 1 float32 ulp from the reference."""
    g = np.random.default_rng(2)
    e = np.array(EDGE_WORDS, dtype=np.uint32)
    a, b = np.meshgrid(e, e, indexing="ij")
    pairs = np.stack([a.ravel(), b.ravel()], 1)
    x = np.ascontiguousarray(np.concatenate([np.concatenate([pairs, pairs[::-1]], 1),
                                             g.integers(0, 2 ** 32, (200_000, 4), dtype=np.uint64).astype(np.uint32)]))
    z = np.empty((x.shape[0], 3), dtype=np.float32)
    cn.cn_normals_of_words_many(x.shape[0], x.ctypes.data, z.ctypes.data)
    ref = R.normals_of_words(x)

    def key(v):
        i = np.ascontiguousarray(v).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(z) - key(ref))
    print(f"[counter normals] {int((d != 0).sum())} of {d.size} normals differ from the reference, by at most {int(d.max())} ulp; "
          f"largest |z| {np.abs(z).max():.3f}")
    assert np.isfinite(z).all() and d.max() <= 1
    assert abs(float(np.abs(z).max()) - np.sqrt(-2.0 * np.log(2.0 ** -33))) < 1e-5   # x0 = 0: the longest radius a draw can have


def test_counter_normals_is_philox_then_normals_of_words(cn):
    for n, t, seed in ((0, 1, 0), (4099, 2 ** 32 + 5, 2 ** 63 + 12345)):
        z = (ct.c_float * 3)()
        cn.cn_counter_normals(n, t, seed, z)
        got, ref = np.array(z[:], dtype=np.float32), R.normals(1, t, seed, n_first=n)[0]
        assert np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max() <= 1
