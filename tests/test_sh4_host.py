"""Degree-4 spherical harmonics of gs_math.h compiled for the host (tests/hostmath/sh4math.cpp), against the fp64 restatements
of tests/sh4_ref.py, and the front end's argument checks at degree 4 and 5 (no GPU needed)."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

import sh4_ref

HM = os.path.join(os.path.dirname(__file__), "hostmath")


@pytest.fixture(scope="module")
def sh4():
    so = os.path.join(HM, "libsh4math.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HM, "sh4math.cpp")], check=True)
    return ct.CDLL(so)


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ct.c_void_p)


def _dirs(n, seed):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_degree4_basis_equals_both_restatements(sh4):
    u = _dirs(20000, 1)
    Y = np.zeros((len(u), 25), np.float32)
    sh4.sh4_basis(4, len(u), _p(u), _p(Y))
    u64 = torch.from_numpy(u.astype(np.float64))
    closed = sh4_ref.sh_basis(u64, 4).numpy()
    # the two fp64 forms are the same functions ON the sphere (they differ off it: directions renormalised in fp64)
    un = u64 / u64.norm(dim=-1, keepdim=True)
    assert np.abs(sh4_ref.sh_basis(un, 4).numpy() - sh4_ref.sh_basis_sloan(un).numpy()).max() < 1e-13
    # fp32 evaluation: a few ulp of the largest term (|Y_k| <= ~2.6 on the sphere)
    assert np.abs(Y - closed).max() < 4e-6, np.abs(Y - closed).max()
    # degree 3 and below untouched by the degree-4 band: the first 16 functions are those of a degree-3 call, bit for bit
    Y3 = np.full((len(u), 25), 7.0, np.float32)
    sh4.sh4_basis(3, len(u), _p(u), _p(Y3))
    assert np.array_equal(Y3[:, :16], Y[:, :16]) and np.all(Y3[:, 16:] == 7.0)


def test_degree4_band_is_orthonormal_on_the_sphere():
    # Gauss-Legendre in cos(theta) x uniform in phi: exact for polynomials of degree 8 on the sphere
    xg, wg = np.polynomial.legendre.leggauss(12)
    phi = (np.arange(24) + 0.5) * (2 * np.pi / 24)
    z = np.repeat(xg, len(phi)); w = np.repeat(wg, len(phi)) * (2 * np.pi / len(phi))
    s = np.sqrt(1 - z * z)
    u = np.stack([s * np.cos(np.tile(phi, len(xg))), s * np.sin(np.tile(phi, len(xg))), z], -1)
    Y = sh4_ref.sh_basis(torch.from_numpy(u), 4).numpy()
    gram = (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(25)).max() < 1e-12, np.abs(gram - np.eye(25)).max()


def _free_grad64(u, d, degree):
    """sum_k d[k] dY_k/du with u free: fp64 autograd of the restated polynomials."""
    ut = torch.from_numpy(u.astype(np.float64)).requires_grad_(True)
    ka = (degree + 1) ** 2
    (sh4_ref.sh_basis(ut, degree) * torch.from_numpy(d[:, :ka].astype(np.float64))).sum().backward()
    return ut.grad.numpy()


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_dir_grad_against_autograd(sh4, degree):
    n = 4000
    u = _dirs(n, 2 + degree)
    d = np.random.default_rng(9).standard_normal((n, 25)).astype(np.float32)
    g = np.zeros((n, 3), np.float32)
    sh4.sh4_dir_grad(degree, n, _p(d), _p(u), _p(g))
    ref = _free_grad64(u, d, degree)
    scale = np.abs(ref).max()
    assert np.abs(g - ref).max() < 2e-6 * scale, np.abs(g - ref).max() / scale


def test_sh_dir_jacobian_degree4_against_autograd(sh4):
    n, K = 2000, 25
    u = _dirs(n, 5)
    sh = np.random.default_rng(6).standard_normal((n, K, 3)).astype(np.float32)
    G = np.zeros((n, 12), np.float32)
    sh4.sh4_dir_jacobian(4, K, n, _p(sh), _p(u), _p(G))
    for c in range(3):
        ref = _free_grad64(u, np.ascontiguousarray(sh[:, :, c]), 4)
        got = G.reshape(n, 3, 4)[:, :, c]
        assert np.abs(got - ref).max() < 2e-6 * np.abs(ref).max(), c
    assert np.all(G.reshape(n, 3, 4)[:, :, 3] == 0)


@pytest.mark.parametrize("degree,K", [(4, 25), (3, 25), (2, 25), (0, 25)])
def test_sh_to_rgb_and_vjps_against_autograd(sh4, degree, K):
    n = 3000
    rng = np.random.default_rng(10 + degree)
    means = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    cam = np.array([0.3, -0.2, -5.0], np.float32)
    dvec = (means - cam).astype(np.float32)
    dn = np.linalg.norm(dvec, axis=1).astype(np.float32)
    u = (dvec / dn[:, None]).astype(np.float32)
    sh = (rng.standard_normal((n, K, 3)) * 0.4).astype(np.float32)
    rgb = np.zeros((n, 3), np.float32)
    sh4.sh4_to_rgb(degree, K, n, _p(sh), _p(u), _p(rgb))
    # fp64 autograd through the normalisation: the direction term of v_mean with the clamp mask
    m64 = torch.from_numpy(means.astype(np.float64)).requires_grad_(True)
    s64 = torch.from_numpy(sh.astype(np.float64)).requires_grad_(True)
    ref_rgb = sh4_ref.sh_colors(s64, m64, torch.from_numpy(cam.astype(np.float64))[None], degree)[0]
    assert np.abs(rgb - ref_rgb.detach().numpy()).max() < 2e-5
    v_rgb = rng.standard_normal((n, 3)).astype(np.float32)
    v_sh_ref, v_m_ref = torch.autograd.grad(ref_rgb, (s64, m64), torch.from_numpy(v_rgb.astype(np.float64)), allow_unused=True)
    v_m_ref = torch.zeros_like(m64) if v_m_ref is None else v_m_ref   # (degree 0: the colour does not depend on the direction)
    # (a colour within fp32 rounding of the clamp may take the other side: leave those Gaussians out)
    keep = np.all(np.abs(ref_rgb.detach().numpy()) > 1e-5, axis=1)
    G = np.zeros((n, 12), np.float32)
    if degree >= 1:
        sh4.sh4_dir_jacobian(degree, K, n, _p(sh), _p(u), _p(G))
    for use_jac in (0, 1):
        v_sh = np.full((n, K, 3), 9.0, np.float32)
        v_m = np.zeros((n, 3), np.float32)
        sh4.sh4_vjp(degree, K, n, _p(sh), _p(G), _p(rgb), _p(v_rgb), _p(u), _p(dn), _p(v_sh), _p(v_m), use_jac)
        ka = (degree + 1) ** 2
        assert np.all(v_sh[:, ka:] == 0)
        rs = v_sh_ref.numpy()[keep]
        assert np.abs(v_sh[keep] - rs).max() < 1e-5 * np.abs(rs).max(), use_jac
        rm = v_m_ref.numpy()[keep]
        if degree == 0:
            assert np.all(v_m == 0)
        else:
            assert np.abs(v_m[keep] - rm).max() < 2e-5 * np.abs(rm).max(), (use_jac, np.abs(v_m[keep] - rm).max() / np.abs(rm).max())


def _frontend_args(K):
    N = 4
    return dict(means=torch.zeros(N, 3), quats=torch.ones(N, 4), scales=torch.ones(N, 3), opacities=torch.ones(N),
                colors=torch.zeros(N, K, 3), viewmats=torch.eye(4)[None], Ks=torch.eye(3)[None], width=32, height=32)


def test_frontend_takes_degree4_with_25_coefficients():
    from easy_gaussian_splatting_amd.rendering import rasterization
    a = _frontend_args(25)
    # past the argument checks: CPU tensors then meet the product path's refusal to fall back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(**a, sh_degree=4, packed=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(**a, sh_degree=2, packed=False)   # K = 25 storage at a lower active degree (the degree schedule)
    sh0, shr = torch.zeros(4, 1, 3), torch.zeros(4, 24, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(**{**a, "colors": (sh0, shr)}, sh_degree=4, packed=False)


def test_frontend_still_refuses_degree5_and_short_storage():
    from easy_gaussian_splatting_amd.rendering import rasterization
    with pytest.raises(NotImplementedError):
        rasterization(**_frontend_args(36), sh_degree=5, packed=False)
    with pytest.raises(NotImplementedError):
        rasterization(**_frontend_args(26), sh_degree=4, packed=False)   # more coefficients than degree 4 has
    with pytest.raises(AssertionError):
        rasterization(**_frontend_args(16), sh_degree=4, packed=False)
