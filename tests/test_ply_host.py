"""`checkpoint.save_ply` / `load_ply`: the INRIA point_cloud.ply -- binary_little_endian, all properties float, in the order
x y z nx ny nz f_dc_0..2 f_rest_0..3(K-1)-1 opacity scale_0..2 rot_0..3, f_rest channel-major.  No GPU."""
import numpy as np
import pytest
import torch

from easy_gaussian_splatting_amd.checkpoint import load_ply, save_ply
from easy_gaussian_splatting_amd.model import GaussianModel

PARAMS = ("means", "log_scales", "quats", "sh_0", "sh_rest", "logit_opacities")


def _model(n, degree, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return GaussianModel(means=3 * r(n, 3), log_scales=r(n, 3) - 3, quats=r(n, 4), sh_0=r(n, 1, 3), sh_rest=0.1 * r(n, (degree + 1) ** 2 - 1, 3),
                         logit_opacities=2 * r(n), sh_degree=degree)


def _expected_header(n, degree):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2")]
    lines += [f"property float f_rest_{i}" for i in range(3 * ((degree + 1) ** 2 - 1))]
    lines += ["property float opacity"] + [f"property float scale_{i}" for i in range(3)] + [f"property float rot_{i}" for i in range(4)]
    return lines + ["end_header"]


@pytest.mark.parametrize("degree", (0, 3))
def test_header_is_the_inria_layout_line_for_line(tmp_path, degree):
    n = 7
    save_ply(_model(n, degree), tmp_path / "point_cloud.ply")
    raw = (tmp_path / "point_cloud.ply").read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert raw[:end].decode("ascii").split("\n")[:-1] == _expected_header(n, degree)
    assert len(raw) - end == n * 4 * (17 + 3 * ((degree + 1) ** 2 - 1))     # nothing but N rows of little-endian floats


@pytest.mark.parametrize("degree", (0, 1, 2, 3, 4))
def test_save_then_load_is_bit_for_bit(tmp_path, degree):
    m = _model(33, degree, seed=degree)
    save_ply(m, tmp_path / "a.ply")
    back = load_ply(tmp_path / "a.ply", device="cpu")
    assert back.MAX_SH_DEGREE == degree and back.active_sh_degree == degree
    for name in PARAMS:
        a, b = getattr(m, name).detach(), getattr(back, name).detach()
        assert a.shape == b.shape and b.dtype == torch.float32 and b.is_contiguous(), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert load_ply(tmp_path / "a.ply", sh_degree=degree, device="cpu", white_background=True).BACKGROUND.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        load_ply(tmp_path / "a.ply", sh_degree=(degree + 1) % 5, device="cpu")


def test_a_body_written_by_hand_loads_to_the_expected_tensors(tmp_path):
    """Written with numpy alone in the INRIA order; every value names its own (vertex, property), so a swapped column shows.
    f_rest is channel-major: f_rest[c * 15 + j] is coefficient j + 1 of colour channel c."""
    n, degree = 5, 3
    cols = 17 + 45
    body = (np.arange(n, dtype=np.float32)[:, None] * 1000 + np.arange(cols, dtype=np.float32)[None, :]).astype("<f4")
    with open(tmp_path / "hand.ply", "wb") as f:
        f.write(("\n".join(_expected_header(n, degree)) + "\n").encode("ascii"))
        f.write(body.tobytes())
    m = load_ply(tmp_path / "hand.ply", device="cpu")
    v = lambda i, c: float(i * 1000 + c)   # noqa: E731
    for i in range(n):
        assert m.means[i].tolist() == [v(i, 0), v(i, 1), v(i, 2)]                      # (3..5: the normals, dropped)
        assert m.sh_0[i, 0].tolist() == [v(i, 6), v(i, 7), v(i, 8)]
        for j in range(15):
            assert m.sh_rest[i, j].tolist() == [v(i, 9 + j), v(i, 9 + 15 + j), v(i, 9 + 30 + j)]
        assert m.logit_opacities.tolist()[i] == v(i, 54)                             # the logit, as stored
        assert m.log_scales[i].tolist() == [v(i, 55), v(i, 56), v(i, 57)]              # the logs, as stored
        assert m.quats[i].tolist() == [v(i, 58), v(i, 59), v(i, 60), v(i, 61)]         # wxyz, not normalised
    # and the writer puts them back where they came from, the normals as zeros
    save_ply(m, tmp_path / "again.ply")
    raw = (tmp_path / "again.ply").read_bytes()
    again = np.frombuffer(raw[raw.index(b"end_header\n") + 11:], dtype="<f4").reshape(n, cols)
    want = body.copy()
    want[:, 3:6] = 0.0
    assert np.array_equal(again, want)


def test_what_is_not_the_inria_layout_is_refused(tmp_path):
    header = _expected_header(2, 0)
    body = np.zeros((2, 17), "<f4").tobytes()

    def write(lines, payload=body):
        with open(tmp_path / "bad.ply", "wb") as f:
            f.write(("\n".join(lines) + "\n").encode("ascii"))
            f.write(payload)
        return tmp_path / "bad.ply"
    load_ply(write(header), device="cpu")                                             # the good one loads
    ascii_lines = [ln.replace("binary_little_endian", "ascii") for ln in header]
    with pytest.raises(ValueError, match="binary_little_endian"):
        load_ply(write(ascii_lines, ("0 " * 17 + "\n").encode() * 2), device="cpu")
    with pytest.raises(ValueError, match="binary_little_endian"):
        load_ply(write([ln.replace("binary_little_endian", "binary_big_endian") for ln in header]), device="cpu")
    rest10 = header[:12] + [f"property float f_rest_{i}" for i in range(10)] + header[12:]
    with pytest.raises(ValueError, match="f_rest"):
        load_ply(write(rest10, np.zeros((2, 27), "<f4").tobytes()), device="cpu")
    with pytest.raises(ValueError, match="property set"):
        load_ply(write(header[:-2] + ["property float extra", "end_header"]), device="cpu")       # rot_3 replaced
    with pytest.raises(ValueError, match="float"):
        load_ply(write([ln.replace("property float opacity", "property uchar opacity") for ln in header]), device="cpu")
    with pytest.raises(ValueError, match="bytes"):
        load_ply(write(header, body[:-4]), device="cpu")
    with pytest.raises(ValueError, match="not a PLY"):
        load_ply(write(["plx"] + header[1:]), device="cpu")
