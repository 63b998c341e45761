"""`compress.quantize` / `dequantize` and the compact file on a CPU model (the codebook-is-the-points path: no kernel).  No GPU.

The bound: in the quantised domain T(v) -- T = sign(v) log1p(|v|) for the means, the identity otherwise --
    |T(v) - T(dequant(quant(v)))| <= 0.5 step (1 + 2^-10),  step = (T(hi) - T(lo)) / (2^b - 1),
half a step for the rounding to the nearest level and 2^-10 of it for the arithmetic.  `dequantize` returns float64 and is held to
that at every width.  A LOADED model stores float32: the rounding of the value costs up to 2^-24 |v| more, which lies inside the
2^-11 step of slack only while |v| <= 2^13 step (identity) resp. |v| / (1 + |v|) <= 2^13 step (log domain).  The file test therefore
uses a model in which that holds by construction and checks that it does: 8-bit channels of zero-centred values (|v| <= range, step
= range / 255) and means spanning +-100 units (T's range 9.2, step 1.4e-4: 2^13 step = 1.15 >= 1).  For a scene of smaller extent
the float32 store can add up to 2^-24 to half a 16-bit step of the means; DESIGN.md says so."""
import json
import os

import numpy as np
import pytest
import torch

import compress_ref as CR
from easy_gaussian_splatting_amd import compress as C
from easy_gaussian_splatting_amd.model import GaussianModel

SLACK = 1.0 + 2.0 ** -10


@pytest.mark.parametrize("bits", (1, 4, 8, 12, 16))
@pytest.mark.parametrize("log", (False, True))
def test_quantiser_stays_within_half_a_step(bits, log):
    g = torch.Generator().manual_seed(bits + 100 * log)
    v = torch.randn(4000, 5, generator=g) * torch.tensor([1.0, 1e-3, 50.0, 1.0, 7.0]) + torch.tensor([0.0, 5.0, -20.0, 1e4, 0.0])
    v[:, 4] = 7.0                                                   # a constant channel
    T = (C.log_domain, C.log_domain_inverse) if log else (None, None)
    q, lo, hi = C.quantize(v, bits, T[0])
    assert lo.dtype == hi.dtype == torch.float32 and torch.equal(lo, v.min(0).values) and torch.equal(hi, v.max(0).values)
    assert q.dtype == (torch.uint8 if bits <= 8 else torch.int32) and int(q.min()) == 0 and int(q.max()) == 2 ** bits - 1
    back = C.dequantize(q, lo, hi, bits, *T)
    assert back.dtype == torch.float64
    err, step = CR.domain_error(v.numpy(), back.numpy(), lo.numpy(), hi.numpy(), bits, log)
    print(f"[compress] bits = {bits}, log = {log}: worst error / step per channel = {(err.max(0) / np.maximum(step, 1e-300)).round(6).tolist()}")
    assert (err <= 0.5 * step[None, :] * SLACK).all()
    assert (q[:, 4] == 0).all() and torch.equal(back[:, 4], v[:, 4].double())      # hi == lo: q = 0, and the value back exactly
    # the formula itself, in numpy float64
    assert np.array_equal(q.numpy().astype(np.int64), CR.quant_formula(v.numpy(), lo.numpy(), hi.numpy(), bits, log))


def test_non_finite_values_and_bad_widths_are_refused():
    v = torch.zeros(4, 2)
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = v.clone()
        w[1, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            C.quantize(w, 8)
    for bits in (0, 17, 8.0, True):
        with pytest.raises(ValueError):
            C.quantize(v, bits)


def _model(n, degree, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    means = 30.0 * r(n, 3)
    if n >= 2:
        means[0], means[1] = torch.tensor([-100.0, -100.0, -100.0]), torch.tensor([100.0, 100.0, 100.0])   # the extent of the header
    means.clamp_(-100.0, 100.0)
    return GaussianModel(means=means, log_scales=r(n, 3), quats=r(n, 4), sh_0=r(n, 1, 3), sh_rest=0.1 * r(n, (degree + 1) ** 2 - 1, 3),
                         logit_opacities=2 * r(n), sh_degree=degree, white_background=True, min_opacity=0.01, max_scale_ratio=7.0)


@pytest.mark.parametrize("degree,n", [(3, 700), (0, 700), (1, 1)])
def test_file_round_trip_on_the_cpu(tmp_path, degree, n):
    m = _model(n, degree, seed=degree)
    m.active_sh_degree = min(1, degree)
    path = tmp_path / "model.compact"
    meta = C.save_compact(m, path, sh_clusters=65536)
    assert os.path.exists(path) and not os.path.exists(str(path) + ".npz")
    d = 3 * ((degree + 1) ** 2 - 1)
    k = n if degree else 0
    size = os.path.getsize(path)
    print(f"[compress] degree {degree}, N = {n}: {size} bytes = {size / n:.1f} per Gaussian (the raw codes: {19 * n + k * d})")
    assert size <= 19 * n + k * d + 8192
    back = C.load_compact(path, device="cpu")
    assert isinstance(back, GaussianModel) and back.nbr_gaussians == n
    assert (back.MAX_SH_DEGREE, back.active_sh_degree, back.BACKGROUND.tolist()) == (degree, min(1, degree), [1.0, 1.0, 1.0])
    assert (back.MIN_OPACITY, back.MAX_SCALE_RATIO, back.optimizer) == (0.01, 7.0, None) and meta["n"] == n
    assert back.sh_rest.shape == (n, (degree + 1) ** 2 - 1, 3) and back.sh_0.shape == (n, 1, 3) and back.logit_opacities.shape == (n,)
    with np.load(path, allow_pickle=False) as z:
        files = {name: z[name] for name in z.files}
    assert str(files["format"]) == C.FORMAT and json.loads(str(files["meta"])) == meta
    assert files["means"].dtype == np.uint16 and files["quats"].dtype == np.uint8
    assert ("sh_labels" in files) == ("sh_codebook" in files) == (degree > 0)
    # undo the Morton order WITHOUT the code under test: a loaded mean is within half a 16-bit step of its own original, the
    # originals are far further apart
    perm = CR.match_rows(m.means.detach().numpy(), back.means.detach().numpy())
    ranges, row = files["ranges"], 0
    for name, log in (("means", True), ("log_scales", False), ("quats", False), ("logit_opacities", False), ("sh_0", False)):
        want = CR.canonical(m, name)
        got = getattr(back, name).detach().numpy().reshape(n, -1).astype(np.float64)
        lo, hi = ranges[row:row + want.shape[1], 0], ranges[row:row + want.shape[1], 1]
        row += want.shape[1]
        assert np.array_equal(lo, want.min(0).astype(np.float32)) and np.array_equal(hi, want.max(0).astype(np.float32)), name
        err, step = CR.domain_error(want[perm], got, lo, hi, meta["bits"][name], log)
        assert CR.float32_store_fits(want, step, log), name         # the premise of the header
        assert (err <= 0.5 * step[None, :] * SLACK).all(), (name, float((err / np.maximum(step, 1e-300)).max()))
    if degree:
        lo, hi = ranges[row, 0], ranges[row, 1]
        assert files["sh_labels"].dtype == np.uint16 and files["sh_codebook"].shape == (n, d) and len(ranges) == row + 1
        want = m.sh_rest.detach().numpy().reshape(n, -1).astype(np.float64)[perm]
        got = back.sh_rest.detach().numpy().reshape(n, -1).astype(np.float64)
        step = (float(hi) - float(lo)) / 255.0
        assert float(lo) == want.min() and float(hi) == want.max()  # ONE global range
        assert (np.abs(want - got) <= 0.5 * step * SLACK).all()      # the codebook's own half step: the rows ARE the codebook
        assert sorted(files["sh_labels"].tolist()) == list(range(n))
    # neighbours sit together: the file's order is the Morton order of the means
    assert np.array_equal(perm, C.morton_order(m.means.detach()).numpy())


def test_morton_order_on_the_host():
    p = torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    assert C.morton_order(p).tolist() == [1, 5, 2, 3, 4, 0]           # x is the lowest bit, z the highest; equal codes keep their order
    assert C.morton_order(p[:1]).tolist() == [0] and C.morton_order(p[:0]).tolist() == []
    flat = torch.rand(100, 3, generator=torch.Generator().manual_seed(1))
    flat[:, 1] = 0.25                                                # an axis of zero extent contributes 0
    o = C.morton_order(flat)
    assert sorted(o.tolist()) == list(range(100))


def test_what_cannot_be_exported_is_refused(tmp_path):
    m = _model(50, 1)
    with torch.no_grad():
        m.log_scales[7, 1] = float("nan")
    with pytest.raises(ValueError, match="log_scales"):
        C.save_compact(m, tmp_path / "nan.compact")
    assert not os.path.exists(tmp_path / "nan.compact")
    m = _model(50, 1)
    with pytest.raises(ValueError, match="no array named"):
        C.save_compact(m, tmp_path / "x.compact", bits={"colors": 8})
    with pytest.raises(ValueError):
        C.save_compact(m, tmp_path / "x.compact", bits={"means": 24})
    with pytest.raises(NotImplementedError):                         # more Gaussians than clusters needs the device
        C.save_compact(m, tmp_path / "x.compact", sh_clusters=8)
    np.savez_compressed(tmp_path / "other.npz", format=np.array("something else"))
    with pytest.raises(ValueError, match="format"):
        C.load_compact(tmp_path / "other.npz", device="cpu")


def test_bits_override(tmp_path):
    m = _model(300, 2, seed=4)
    C.save_compact(m, tmp_path / "wide.compact", bits={"log_scales": 12, "sh_rest": 16, "sh_0": 4})
    with np.load(tmp_path / "wide.compact", allow_pickle=False) as z:
        assert z["log_scales"].dtype == np.uint16 and int(z["log_scales"].max()) == 4095
        assert z["sh_codebook"].dtype == np.uint16 and int(z["sh_0"].max()) == 15
    back = C.load_compact(tmp_path / "wide.compact", device="cpu")
    perm = CR.match_rows(m.means.detach().numpy(), back.means.detach().numpy())
    err = np.abs(m.log_scales.detach().numpy()[perm] - back.log_scales.detach().numpy())
    rng = (m.log_scales.detach().max(0).values - m.log_scales.detach().min(0).values).numpy()
    assert (err <= 0.5 * rng / 4095 * SLACK + 2.0 ** -24 * np.abs(m.log_scales.detach().numpy()[perm])).all()
