"""The captured budget step without a GPU: the reference of the counter-based draws (tests/mcmc_step_ref.py) against published
Philox4x32-10 answers, the counter / key packing, the C ABI of the new entry points, and the refusals of the Python layer."""
import ctypes as ct
import os
import types

import numpy as np
import pytest
import torch

import mcmc_step_ref as R
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.train_graph import TrainStepGraph, ViewParallelGraphStep

ENTRIES = ("gs_mcmc_normals", "gs_mcmc_step_inputs", "gs_mcmc_noise_step", "gs_mcmc_reg_workspace_floats", "gs_mcmc_reg",
           "gs_project_bwd_adam_mcmc")


def _hex(words):
    return " ".join(f"{w:08x}" for w in words)


def test_philox_known_answers():
    assert _hex(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(R.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_counter_and_key_packing_with_high_words():
    t, seed = 2 ** 32 + 5, 2 ** 63 + 12345
    assert R.counter_key(7, t, seed) == ((7, 0, 5, 1), (12345, 0x80000000))
    assert R.counter_key(2 ** 32 + 9, 1, 3) == ((9, 1, 1, 0), (3, 0))
    # the high words reach the output: the block of (n, t, seed) differs from the one with its high word dropped
    assert R.philox4x32_10(*R.counter_key(7, t, seed)) != R.philox4x32_10(*R.counter_key(7, 5, seed))
    assert R.philox4x32_10(*R.counter_key(7, t, seed)) != R.philox4x32_10(*R.counter_key(7, t, 12345))
    assert R.philox4x32_10(*R.counter_key(7, t, seed)) == R.philox4x32_10((7, 0, 5, 1), (12345, 0x80000000))


def test_reference_normals_are_standard_normal():
    z = R.normals(34000, 3, 11).astype(np.float64).reshape(-1)   # 102000 draws
    assert z.size >= 100_000 and np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.02, (z.mean(), z.var())


def test_reference_normals_formula_on_one_block():
    x = np.array([[0, 2 ** 31, 2 ** 32 - 1, 2 ** 30]], dtype=np.uint32)
    u = (x.astype(np.float64) + 0.5) / 2.0 ** 32
    z = R.normals_of_words(x)[0]
    r01, r23 = np.sqrt(-2 * np.log(u[0, 0])), np.sqrt(-2 * np.log(u[0, 2]))
    want = np.array([r01 * np.cos(2 * np.pi * u[0, 1]), r01 * np.sin(2 * np.pi * u[0, 1]), r23 * np.cos(2 * np.pi * u[0, 3])])
    assert z.dtype == np.float32 and np.array_equal(z, want.astype(np.float32)) and np.isfinite(z).all()


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    from easy_gaussian_splatting_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat, nat.lib()


def test_the_entry_points_are_declared_bound_and_exported(lib):
    nat, L = lib
    P, I, Q, U, D, F = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_uint64, ct.c_double, ct.c_float
    assert nat.SIGNATURES["gs_mcmc_normals"] == (ct.c_int, [P, Q, Q, U, P])
    assert nat.SIGNATURES["gs_mcmc_step_inputs"] == (ct.c_int, [P, D, Q, U, P])
    assert nat.SIGNATURES["gs_mcmc_noise_step"] == (ct.c_int, [P, Q, P, P, P, P, P])
    assert nat.SIGNATURES["gs_mcmc_reg_workspace_floats"] == (ct.c_size_t, [Q])
    assert nat.SIGNATURES["gs_mcmc_reg"] == (ct.c_int, [P, Q, P, P, D, D, P, P, P, P])
    plain = nat.SIGNATURES["gs_project_bwd_adam"]
    assert nat.SIGNATURES["gs_project_bwd_adam_mcmc"] == (ct.c_int, plain[1] + [I, F, F, D, D])
    assert nat.PARAMS["gs_project_bwd_adam_mcmc"][-5:] == ["scale_reg", "max_ratio", "lambda", "a", "b"]
    for name in ENTRIES:
        assert getattr(L, name).argtypes == nat.SIGNATURES[name][1] and getattr(L, name).restype == nat.SIGNATURES[name][0], name
    assert nat.GS_MCMC_REC_WORDS == 4
    assert L.gs_version() >= 360
    import easy_gaussian_splatting_amd as pkg
    assert pkg.counter_normals is M.counter_normals and "counter_normals" in pkg.__all__


def test_workspace_size_of_the_regulariser(lib):
    _, L = lib
    ws = L.gs_mcmc_reg_workspace_floats
    assert [ws(n) for n in (-1, 0, 1, 256, 257, 20000)] == [2, 2, 6, 6, 10, 2 + 4 * 79]


def test_the_new_entries_refuse_bad_arguments_before_a_launch(lib):
    _, L = lib
    raw = (ct.c_float * 16)()
    p = (ct.addressof(raw) + 15) & ~15   # never dereferenced: every call below is refused first, or has nothing to do
    err = lambda: L.gs_last_error().decode()   # noqa: E731
    big = 2 ** 31
    assert L.gs_mcmc_normals(None, -1, 1, 0, p) == -1 and "0 <= n < 2^31" in err()
    assert L.gs_mcmc_normals(None, big, 1, 0, p) == -1 and "0 <= n < 2^31" in err()
    assert L.gs_mcmc_normals(None, 4, -1, 0, p) == -1 and "step >= 0" in err()
    assert L.gs_mcmc_normals(None, 4, 1, 0, None) == -1 and "z_out" in err()
    assert L.gs_mcmc_normals(None, 4, 1, 0, p + 4) == -1 and "16-byte aligned" in err()
    assert L.gs_mcmc_normals(None, 0, 1, 0, None) == 0
    assert L.gs_mcmc_step_inputs(None, float("nan"), 1, 0, p) == -1 and "NaN" in err()
    assert L.gs_mcmc_step_inputs(None, 1.0, -1, 0, p) == -1 and "step >= 0" in err()
    assert L.gs_mcmc_step_inputs(None, 1.0, 1, 0, None) == -1 and "rec_dev" in err()
    assert L.gs_mcmc_step_inputs(None, 1.0, 1, 0, p + 8) == -1 and "16-byte aligned" in err()

    def noise(n=4, rec=p, ls=p, q=p, lo=p, means=p):
        return L.gs_mcmc_noise_step(None, n, rec, ls, q, lo, means)
    for kw in (dict(n=-1), dict(n=big)):
        assert noise(**kw) == -1 and "0 <= n < 2^31" in err(), kw
    for kw in (dict(rec=None), dict(ls=None), dict(q=None), dict(lo=None), dict(means=None)):
        assert noise(**kw) == -1 and "null pointer" in err(), kw
    for kw in (dict(rec=p + 8), dict(ls=p + 4), dict(q=p + 8), dict(lo=p + 4), dict(means=p + 4)):
        assert noise(**kw) == -1 and "16-byte aligned" in err(), kw
    assert noise(n=0, means=None) == 0

    def reg(n=4, lo=p, ls=p, a=0.01, b=0.01, loss3=p, ws=p, vl=p, vs=p):
        return L.gs_mcmc_reg(None, n, lo, ls, a, b, loss3, ws, vl, vs)
    assert reg(n=-1) == -1 and "N >= 0" in err()
    for kw in (dict(lo=None), dict(ls=None), dict(ws=None)):
        assert reg(**kw) == -1 and "null pointer" in err(), kw
    for kw in (dict(a=float("nan")), dict(b=float("nan"))):
        assert reg(**kw) == -1 and "NaN" in err(), kw
    assert reg(ws=p + 4) == -1 and "16-byte aligned" in err()
    for kw in (dict(lo=p + 2), dict(vl=p + 1), dict(vs=p + 2), dict(loss3=p + 3)):
        assert reg(**kw) == -1 and "4-byte aligned" in err(), kw
    assert reg(n=0, loss3=None, vl=None, vs=None) == 0


# ---- the Python refusals, none of which needs a device ----

def test_the_python_layer_refuses_before_any_native_call(monkeypatch):
    from easy_gaussian_splatting_amd import _native as nat
    monkeypatch.setattr(nat, "lib", lambda: pytest.fail("a refusal reached the native library"))
    with pytest.raises(ValueError, match="noise: 'torch' or 'counter'"):
        M.MCMCStrategy(None, cap_max=10, noise="philox")
    with pytest.raises(NotImplementedError, match="HIP device"):
        M.counter_normals(4, 1, 0, "cpu")
    # a runner over a strategy that draws torch.randn: its replays could not reproduce the draws
    torch_noise = types.SimpleNamespace(noise="torch", model=None, seed=0, noise_lr=1.0)
    with pytest.raises(ValueError, match="noise='counter'"):
        TrainStepGraph(None, None, None, {}, torch.zeros(1), mcmc=torch_noise)
    counter = types.SimpleNamespace(noise="counter", model=object(), seed=0, noise_lr=1.0)
    with pytest.raises(ValueError, match="another model"):
        TrainStepGraph(None, None, None, {}, torch.zeros(1), mcmc=counter)
    with pytest.raises(ValueError, match="broadcast draws"):
        ViewParallelGraphStep(None, None, None, {}, torch.zeros(1), vp=None, mcmc=counter)


def test_after_step_refuses_a_runner_built_for_another_strategy():
    s = M.MCMCStrategy.__new__(M.MCMCStrategy)
    s.noise, s.refine_start, s.refine_stop, s.refine_every = "counter", 0, 10, 5
    with pytest.raises(ValueError, match="mcmc=<this strategy>"):
        s.after_step(1, runner=types.SimpleNamespace(mcmc=None))


def test_budget_reference_against_finite_differences():
    g = np.random.default_rng(0)
    l, ls = g.uniform(-4, 4, 7), g.uniform(-3, 1, (7, 3))
    a, b = 0.3, 0.7
    v, gl, gs = R.budget_reg(l, ls, a, b)
    h = 1e-6
    for i in range(7):
        lp = l.copy(); lp[i] += h
        fd = (R.budget_reg(lp, ls, a, b)[0] - v) / h
        assert abs(fd - gl[i]) < 1e-6 * max(abs(gl[i]), 1e-3) + 1e-8   # (the float32 upstream factor: 6e-8 relative)
        sp = ls.copy(); sp[i, 1] += h
        fd = (R.budget_reg(l, sp, a, b)[0] - v) / h
        assert abs(fd - gs[i, 1]) < 2e-6 * abs(gs[i, 1]) + 1e-8
