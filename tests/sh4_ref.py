"""Degree-4 spherical harmonics restated in torch (fp64-capable, differentiable) for the SH4 tests.

The oracle (oracle/torch_oracle.py, oracle/c) stops at degree 3, so tests/test_sh4_host.py and tests/test_gpu_sh4.py restate
the basis here: `sh_basis` in the closed form of gsplat's sign convention (the polynomials exactly as gs_math.h writes them,
so that free-variable derivatives agree too), and `sh_basis_sloan` in the recurrence form gsplat evaluates
(`_eval_sh_bases_fast`: fC / fS / fTmpA..D), an independent second statement of the same functions on the unit sphere."""
import torch

C0 = 0.2820947917738781
C1 = 0.4886025119029199
C2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
C3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277)
C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
      -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761)


def sh_basis(dirs: torch.Tensor, degree: int) -> torch.Tensor:
    """[..., 3] direction (unit, or free for derivative checks) -> [..., (degree+1)^2]."""
    x, y, z = dirs.unbind(-1)
    Y = [torch.full_like(x, C0)]
    if degree >= 1:
        Y += [-C1 * y, C1 * z, -C1 * x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        Y += [C2[0] * x * y, -C2[0] * y * z, C2[1] * (2 * zz - xx - yy), -C2[0] * x * z, C2[2] * (xx - yy)]
    if degree >= 3:
        Y += [-C3[0] * y * (3 * xx - yy), C3[1] * x * y * z, -C3[2] * y * (4 * zz - xx - yy),
              C3[3] * z * (2 * zz - 3 * xx - 3 * yy), -C3[2] * x * (4 * zz - xx - yy), C3[4] * z * (xx - yy),
              -C3[0] * x * (xx - 3 * yy)]
    if degree >= 4:
        Y += [C4[0] * x * y * (xx - yy), C4[1] * y * z * (3 * xx - yy), C4[2] * x * y * (7 * zz - 1),
              C4[3] * y * z * (7 * zz - 3), C4[4] * (zz * (35 * zz - 30) + 3), C4[5] * x * z * (7 * zz - 3),
              C4[6] * (xx - yy) * (7 * zz - 1), C4[7] * x * z * (xx - 3 * yy), C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(Y, -1)


def sh_basis_sloan(dirs: torch.Tensor) -> torch.Tensor:
    """The 25 degree-0..4 functions in gsplat's recurrence form (unit directions only)."""
    x, y, z = dirs.unbind(-1)
    z2 = z * z
    out = [None] * 25
    out[0] = torch.full_like(x, 0.2820947917738781)
    out[1], out[2], out[3] = -0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x
    fC1, fS1 = x * x - y * y, 2 * x * y
    pSH6 = 0.9461746957575601 * z2 - 0.3153915652525201
    tB = -1.092548430592079 * z
    tA = 0.5462742152960395
    out[6], out[7], out[5], out[8], out[4] = pSH6, tB * x, tB * y, tA * fC1, tA * fS1
    tC = -2.285228997322329 * z2 + 0.4570457994644658
    tB = 1.445305721320277 * z
    tA = -0.5900435899266435
    fC2, fS2 = x * fC1 - y * fS1, x * fS1 + y * fC1
    pSH12 = z * (1.865881662950577 * z2 - 1.119528997770346)
    out[12], out[13], out[11], out[14], out[10], out[15], out[9] = pSH12, tC * x, tC * y, tB * fC1, tB * fS1, tA * fC2, tA * fS2
    tD = z * (-4.683325804901025 * z2 + 2.007139630671868)
    tC = 3.31161143515146 * z2 - 0.47308734787878
    tB = -1.770130769779931 * z
    tA = 0.6258357354491763
    fC3, fS3 = x * fC2 - y * fS2, x * fS2 + y * fC2
    out[20] = 1.984313483298443 * z * pSH12 - 1.006230589874905 * pSH6
    out[21], out[19], out[22], out[18] = tD * x, tD * y, tC * fC1, tC * fS1
    out[23], out[17], out[24], out[16] = tB * fC2, tB * fS2, tA * fC3, tA * fS3
    return torch.stack(out, -1)


def sh_colors(shs: torch.Tensor, means: torch.Tensor, campos: torch.Tensor, degree: int) -> torch.Tensor:
    """gsplat's `spherical_harmonics` + the +0.5 / clamp of `rasterization`: shs [N,K,3], means [N,3], campos [C,3] -> [C,N,3]."""
    d = means[None] - campos[:, None]
    u = d / d.norm(dim=-1, keepdim=True)
    ka = (degree + 1) ** 2
    Y = sh_basis(u, degree)
    return torch.clamp_min((Y[..., None] * shs[None, :, :ka]).sum(-2) + 0.5, 0.0)
