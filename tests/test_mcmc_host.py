"""Training to a Gaussian budget (easy_gaussian_splatting_amd/mcmc.py, csrc/gs_mcmc.hip), host side: the reference of
tests/mcmc_ref.py against closed forms, the declarations and refusals of the new entry points, the workspace size, and the
strategy's refusals on CPU tensors.  Nothing here launches a kernel."""
import ctypes as ct
import math
import os

import numpy as np
import pytest
import torch

import mcmc_ref as R
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gs_mcmc_weights", "gs_mcmc_cdf_workspace_longs", "gs_mcmc_cdf", "gs_mcmc_sample", "gs_mcmc_relocation_values",
           "gs_mcmc_apply", "gs_mcmc_noise")


# ---- the reference ----

@pytest.mark.parametrize("values", [R.relocation_values, R.relocation_values_plain])
def test_one_copy_changes_nothing_and_two_copies_have_a_closed_form(values):
    s = np.array([0.3, 0.02, 1.7])
    for o in (0.005, 0.1, 0.5, 0.9, 1 - 2.0 ** -24):
        on, sn = values(o, s, 1)
        assert abs(on - o) <= 2e-16 and np.abs(sn - s).max() <= 1e-15 * s.max()
        on, sn = values(o, s, 2)
        assert abs(on - (1 - math.sqrt(1 - o))) <= 4e-16
        D = 2 * on - on * on / math.sqrt(2)
        assert np.abs(sn - s * o / D).max() <= 1e-14 * s.max()
    # a ratio outside [1, 51] is clamped
    assert values(0.3, s, 0)[0] == values(0.3, s, 1)[0] and values(0.3, s, 1000)[0] == values(0.3, s, 51)[0]


def test_scales_shrink_with_the_number_of_copies_and_the_last_ratio_stays_finite():
    for o in (0.01, 0.1, 0.5, 0.9, 0.999):
        shrink = [R.relocation_values(o, [1.0, 1.0, 1.0], r)[1][0] for r in range(1, 52)]
        assert shrink[0] == pytest.approx(1.0, abs=1e-15) and all(a > b for a, b in zip(shrink, shrink[1:])), o
        assert shrink[-1] > 0.05
    on, sn = R.relocation_values(1 - 2.0 ** -24, [1.0, 2.0, 3.0], 51)
    assert 0.27 < on < 0.29 and np.isfinite(sn).all() and (sn > 0).all() and sn[0] < 1.0
    # the two spellings of o' are one number where the power does not cancel; for a tiny o only log1p / expm1 keeps it
    for o in (0.1, 0.7):
        a, b = R.relocation_values(o, [1.0] * 3, 7), R.relocation_values_plain(o, [1.0] * 3, 7)
        assert abs(a[0] - b[0]) <= 1e-15 and np.abs(a[1] - b[1]).max() <= 1e-13
    assert R.relocation_values(1e-13, [1.0] * 3, 4)[0] == pytest.approx(2.5e-14, rel=1e-12)


def test_a_float32_restatement_of_the_values_is_not_good_enough():
    """Why the kernel works in fp64: the same sum in float32 is off by far more than the 2 ulp the GPU tests allow."""
    f = np.float32
    o, r = f(0.1), 51
    on = f(1) - f(f(1) - o) ** f(1.0 / r)
    D = f(0)
    for i in range(1, r + 1):
        for k in range(i):
            D = f(D + f(math.comb(i - 1, k)) * f((-1.0) ** k) * f(on ** f(k + 1)) / f(math.sqrt(k + 1)))
    ref = R.relocation_values(float(o), [1.0] * 3, r)[1][0]
    assert abs(float(o / D) - ref) / ref > 1e-6


def test_weights_cdf_and_draws_of_the_reference():
    logits = np.array([-30.0, 0.0, 30.0, -5.3, 2.0], dtype=np.float32)
    w, dead, o = R.weights(logits, 0.005)
    assert dead.tolist() == [True, False, False, True, False] and w.tolist() == [0, 2 ** 23, 2 ** 24 - 1, 0, int(math.floor(o[4] * 2 ** 24))]
    wg, dg, _ = R.weights(logits, 0.005, grow=True)
    assert not dg.any() and wg[0] == 1 and wg[3] == int(math.floor(o[3] * 2 ** 24))
    c = R.cdf([3, 0, 0, 5, 2 ** 32])
    assert c == [3, 3, 3, 8, 8 + 2 ** 32]
    assert [R.upper_bound(c, t) for t in (0, 2, 3, 7, 8, 7 + 2 ** 32)] == [0, 0, 3, 3, 4, 4]
    assert R.mulhi64(-1, 10) == 9 and R.mulhi64(0, 10) == 0 and R.mulhi64(2 ** 63, 10) == 5 and R.mulhi64(-2 ** 63, 10) == 5
    src, counts = R.draws([0, 7, 0], [0, -1, 12345], 3)
    assert src == [1, 1, 1] and counts.tolist() == [0, 3, 0]
    assert R.draws([0, 0], [5, 6], 2)[0] == []


def test_ulp_distance():
    a = np.array([1.0, -1.0, 0.0, 1e-45], dtype=np.float32)
    assert R.ulp_distance(a, a).tolist() == [0, 0, 0, 0]
    assert R.ulp_distance(a, np.nextafter(a, np.float32(2))).tolist() == [1, 1, 1, 1]
    assert R.ulp_distance(np.float32([1e-45]), np.float32([-1e-45])).tolist() == [2]


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    from easy_gaussian_splatting_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        nat.build()
    return nat, nat.lib()


def test_the_entry_points_are_declared_bound_and_exported(lib):
    nat, L = lib
    P, I, Q, D = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_double
    assert nat.SIGNATURES["gs_mcmc_weights"] == (ct.c_int, [P, Q, P, D, I, P, P])
    assert nat.SIGNATURES["gs_mcmc_cdf_workspace_longs"] == (ct.c_size_t, [Q])
    assert nat.SIGNATURES["gs_mcmc_cdf"] == (ct.c_int, [P, Q, P, P, P])
    assert nat.SIGNATURES["gs_mcmc_sample"] == (ct.c_int, [P, Q, Q, P, P, P, P, Q, P, P, P, P])
    assert nat.SIGNATURES["gs_mcmc_relocation_values"] == (ct.c_int, [P, Q, P, P, P, P, P])
    assert nat.SIGNATURES["gs_mcmc_apply"] == (ct.c_int, [P, Q, Q, I, D, P, P, P, P, Q, P, P, P, P])
    assert nat.SIGNATURES["gs_mcmc_noise"] == (ct.c_int, [P, Q, D, P, P, P, P, P])
    for name in ENTRIES:
        assert getattr(L, name).argtypes == nat.SIGNATURES[name][1], name
    assert L.gs_version() >= 350
    import easy_gaussian_splatting_amd as pkg
    for name in ("MCMCStrategy", "opacity_weights", "weight_cdf", "sample_by_weight", "relocation_values"):
        assert getattr(pkg, name) is getattr(M, name) and name in pkg.__all__
    mk = open(os.path.join(nat.CSRC_DIR, "Makefile")).read()
    assert "gs_mcmc.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]


def test_workspace_size_of_the_cdf(lib):
    _, L = lib
    ws = L.gs_mcmc_cdf_workspace_longs
    block = 2048   # weights per block: 256 threads of eight
    assert [ws(n) for n in (-1, 0, 1, block, block + 1, 1_000_000)] == [1, 1, 2, 2, 3, (1_000_000 + block - 1) // block + 1]


def test_every_entry_refuses_bad_arguments_before_a_launch(lib):
    _, L = lib
    raw = (ct.c_float * 16)()
    p = (ct.addressof(raw) + 15) & ~15   # never dereferenced: every call below is refused first, or has nothing to do
    err = lambda: L.gs_last_error().decode()
    offs = (ct.c_int64 * 6)(0, 12, 24, 40, 52, 52)
    big = 2 ** 31

    def weights(n=4, logit=p, mo=0.005, grow=0, w=p, dead=p):
        return L.gs_mcmc_weights(None, n, logit, mo, grow, w, dead)
    for kw in (dict(n=-1), dict(n=big)):
        assert weights(**kw) == -1 and "0 <= n < 2^31" in err(), kw
    for kw in (dict(mo=-0.1), dict(mo=1.0), dict(mo=float("nan"))):
        assert weights(**kw) == -1 and "min_opacity" in err(), kw
    assert weights(grow=2) == -1 and "grow is 0 or 1" in err()
    for kw in (dict(logit=None), dict(w=None), dict(dead=None)):
        assert weights(**kw) == -1 and "null pointer" in err(), kw
    assert weights(n=0, logit=None, w=None, dead=None) == 0

    def cdf(n=4, w=p, out=p, ws=p):
        return L.gs_mcmc_cdf(None, n, w, out, ws)
    for kw in (dict(n=-1), dict(n=big)):
        assert cdf(**kw) == -1 and "0 <= n < 2^31" in err(), kw
    for kw in (dict(w=None), dict(out=None), dict(ws=None)):
        assert cdf(**kw) == -1 and "null pointer" in err(), kw
    assert cdf(n=0, w=None, out=None, ws=None) == 0

    def sample(n=4, slots=4, cdf_=p, bits=p, dead=p, incl=p, nd=0, src=p, dst=p, counts=p, out=p):
        return L.gs_mcmc_sample(None, n, slots, cdf_, bits, dead, incl, nd, src, dst, counts, out)
    for kw in (dict(n=-1), dict(slots=-1), dict(n=big - 2, slots=big - 2)):
        assert sample(**kw) == -1 and "n + n_slots < 2^31" in err(), kw
    for kw in (dict(dead=None), dict(incl=None)):
        assert sample(**kw) == -1 and "go together" in err(), kw
    assert sample(slots=3) == -1 and "n_slots == n" in err()                                   # relocate: a word per Gaussian
    for kw in (dict(nd=-1), dict(nd=5)):
        assert sample(dead=None, incl=None, **kw) == -1 and "n_draws_host <= n_slots" in err(), kw
    assert sample(out=None) == -1 and "null n_draws_dev" in err()
    for kw in (dict(cdf_=None), dict(counts=None), dict(bits=None), dict(src=None), dict(dst=None)):
        assert sample(**kw) == -1 and "null pointer" in err(), kw

    def values(n=4, o=p, s=p, r=p, no=p, ns=p):
        return L.gs_mcmc_relocation_values(None, n, o, s, r, no, ns)
    assert values(n=-1) == -1 and "0 <= n < 2^31" in err()
    for kw in (dict(o=None), dict(s=None), dict(r=None), dict(no=None), dict(ns=None)):
        assert values(**kw) == -1 and "null pointer" in err(), kw
    assert values(n=0, o=None) == 0

    def apply(n=4, rows=4, K=16, mo=0.005, src=p, dst=p, counts=p, nd=p, max_draws=4, pp=p, m=p, v=p, offs_=offs):
        return L.gs_mcmc_apply(None, n, rows, K, mo, src, dst, counts, nd, max_draws, pp, m, v, offs_)
    for kw in (dict(n=-1), dict(n=5, rows=4), dict(rows=big)):
        assert apply(**kw) == -1 and "n <= n_rows < 2^31" in err(), kw
    for kw in (dict(K=0), dict(K=26)):
        assert apply(**kw) == -1 and "1 <= K <= 25" in err(), kw
    for kw in (dict(mo=-1.0), dict(mo=1.5)):
        assert apply(**kw) == -1 and "min_opacity" in err(), kw
    for kw in (dict(max_draws=-1), dict(max_draws=5)):
        assert apply(**kw) == -1 and "max_draws" in err(), kw
    for kw in (dict(src=None), dict(dst=None), dict(counts=None), dict(nd=None), dict(pp=None), dict(m=None), dict(v=None), dict(offs_=None)):
        assert apply(**kw) == -1 and "null pointer" in err(), kw
    assert apply(offs_=(ct.c_int64 * 6)(0, 12, -4, 40, 52, 52)) == -1 and "negative offset" in err()
    assert apply(n=0, rows=0, max_draws=0, counts=None, pp=None) == 0

    def noise(n=4, strength=1.0, ls=p, q=p, lo=p, z=p, means=p):
        return L.gs_mcmc_noise(None, n, strength, ls, q, lo, z, means)
    for kw in (dict(n=-1), dict(n=big)):
        assert noise(**kw) == -1 and "0 <= n < 2^31" in err(), kw
    assert noise(strength=float("nan")) == -1 and "NaN" in err()
    for kw in (dict(ls=None), dict(q=None), dict(lo=None), dict(z=None), dict(means=None)):
        assert noise(**kw) == -1 and "null pointer" in err(), kw
    for kw in (dict(ls=p + 4), dict(q=p + 8), dict(lo=p + 4), dict(z=p + 12), dict(means=p + 4)):
        assert noise(**kw) == -1 and "16-byte aligned" in err(), kw
    assert noise(n=0, means=None) == 0


# ---- the Python refusals, on CPU tensors ----

def cpu_model(n=12, K=4):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    return GaussianModel(means=r(n, 3), log_scales=r(n, 3), quats=r(n, 4), sh_0=r(n, 1, 3), sh_rest=r(n, K - 1, 3),
                         logit_opacities=r(n), sh_degree=1)


def test_the_strategy_refuses_what_it_cannot_do_before_any_native_call(monkeypatch):
    from easy_gaussian_splatting_amd import _native as nat
    monkeypatch.setattr(nat, "lib", lambda: pytest.fail("a refusal reached the native library"))
    lrs = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)
    torch_adam = cpu_model()
    build_optimizers(torch_adam, *lrs)
    with pytest.raises(NotImplementedError, match="FusedAdam"):
        M.MCMCStrategy(torch_adam, cap_max=100)
    with pytest.raises(NotImplementedError, match="FusedAdam"):
        M.MCMCStrategy(cpu_model(), cap_max=100)                     # no optimizer at all
    on_cpu = cpu_model()
    build_optimizers(on_cpu, *lrs, fused="hip")
    with pytest.raises(NotImplementedError, match="HIP device"):
        M.MCMCStrategy(on_cpu, cap_max=100)
    with pytest.raises(ValueError, match="cap_max = 11 is below the model's 12"):
        M.MCMCStrategy(on_cpu, cap_max=11)
    monkeypatch.setattr(M, "is_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match="broadcast draws"):
        M.MCMCStrategy(on_cpu, cap_max=100)
    monkeypatch.undo()
    monkeypatch.setattr(nat, "lib", lambda: pytest.fail("a refusal reached the native library"))
    # the seams have no CPU path either
    l = torch.zeros(4)
    with pytest.raises(NotImplementedError, match="HIP device"):
        M.opacity_weights(l, 0.005)
    with pytest.raises(NotImplementedError, match="HIP device"):
        M.weight_cdf(torch.ones(4, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="HIP device"):
        M.sample_by_weight(torch.ones(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), n_draws=4)
    with pytest.raises(NotImplementedError, match="HIP device"):
        M.relocation_values(torch.rand(4), torch.rand(4, 3), torch.ones(4, dtype=torch.int32))
