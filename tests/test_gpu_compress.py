"""`compress.save_compact` / `load_compact` on the device: a 3000-Gaussian SH-3 model, 256 clusters -- the k-means kernels, the
device's Morton codes and the loaded model's render.  The bounds are those of tests/test_compress_host.py (its header says why the
model's means span +-100 units: two far-away Gaussians give the file that extent, so that the float32 store of a dequantised mean
lies inside the bound's slack).  No PSNR threshold: that figure is tools/compress_time.py's."""
import numpy as np
import pytest
import torch

import compress_ref as CR
from easy_gaussian_splatting_amd import compress as C
from easy_gaussian_splatting_amd import kmeans as KM
from easy_gaussian_splatting_amd.model import GaussianModel
from easy_gaussian_splatting_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
SLACK = 1.0 + 2.0 ** -10
N, K, W, H = 3000, 256, 64, 64


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dev = torch.device("cuda:0")
    sc = make_scene(N, W, H, sh_degree=3, seed=3, scale_range=(0.03, 0.15), dist=4.0)
    T = torch.from_numpy
    op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
    means = T(sc["means"]).clone()
    means[0], means[1] = torch.tensor([-100.0, -100.0, -100.0]), torch.tensor([100.0, 100.0, 100.0])
    shs = T(sc["shs"])
    m = GaussianModel(means=means, log_scales=torch.log(T(sc["scales"])), quats=T(sc["quats"]), sh_0=shs[:, :1].contiguous(),
                      sh_rest=shs[:, 1:].contiguous(), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)), sh_degree=3,
                      white_background=True).to(dev)
    path = tmp_path_factory.mktemp("compact") / "model.compact"
    meta = C.save_compact(m, path, sh_clusters=K, sh_iters=3, generator=torch.Generator().manual_seed(17))
    back = C.load_compact(path, device=dev)
    with np.load(path, allow_pickle=False) as z:
        files = {name: z[name] for name in z.files}
    perm = CR.match_rows(m.means.detach().cpu().numpy(), back.means.detach().cpu().numpy())
    data = {"w2c": T(sc["viewmats"][0]).to(dev), "K": T(sc["Ks"][0]).to(dev), "width": W, "height": H}
    return m, back, files, meta, perm, data


def test_every_array_stays_within_half_a_step(exported):
    m, back, files, meta, perm, _ = exported
    assert back.nbr_gaussians == N and back.means.is_cuda and meta["sh_clusters"] == K
    ranges, row = files["ranges"], 0
    for name, log in (("means", True), ("log_scales", False), ("quats", False), ("logit_opacities", False), ("sh_0", False)):
        want = CR.canonical(m, name)
        got = getattr(back, name).detach().cpu().numpy().reshape(N, -1).astype(np.float64)
        lo, hi = ranges[row:row + want.shape[1], 0], ranges[row:row + want.shape[1], 1]
        row += want.shape[1]
        assert np.array_equal(lo, want.min(0).astype(np.float32)) and np.array_equal(hi, want.max(0).astype(np.float32)), name
        err, step = CR.domain_error(want[perm], got, lo, hi, meta["bits"][name], log)
        print(f"[compress] {name}: worst error / step = {float((err / step[None, :]).max()):.6f}")
        assert CR.float32_store_fits(want, step, log), name
        assert (err <= 0.5 * step[None, :] * SLACK).all(), name
    # the file's order is the Morton order of the means, from the device's own codes
    assert np.array_equal(perm, C.morton_order(m.means.detach()).cpu().numpy())
    assert np.array_equal(perm, C.morton_order(m.means.detach().cpu()).numpy())      # and the host restatement agrees


def test_sh_rest_is_the_codebook_of_a_fresh_kmeans(exported):
    m, back, files, meta, perm, _ = exported
    labels, book = files["sh_labels"], files["sh_codebook"]
    assert labels.dtype == np.uint16 and labels.shape == (N,) and book.dtype == np.uint8 and book.shape == (K, 45)
    lo, hi = float(files["ranges"][-1, 0]), float(files["ranges"][-1, 1])
    deq = (lo + book.astype(np.float64) * ((hi - lo) / 255.0)).astype(np.float32)          # the dequantised codebook
    got = back.sh_rest.detach().cpu().numpy()
    assert got.shape == (N, 15, 3)
    assert np.array_equal(got.reshape(N, 45).view(np.int32), deq[labels.astype(np.int64)].view(np.int32))
    flat = m.sh_rest.detach().reshape(N, -1).contiguous()
    cent, fresh, inertia = KM.kmeans(flat, K, iters=3, generator=torch.Generator().manual_seed(17))
    assert np.array_equal(labels.astype(np.int32), fresh.cpu().numpy()[perm])
    cent = cent.cpu().numpy().astype(np.float64)
    assert lo == cent.min() and hi == cent.max()                                             # ONE global range
    assert (np.abs(cent - deq) <= 0.5 * (hi - lo) / 255.0 * SLACK).all()                     # the codebook's own half step
    vals = [float(t) for t in inertia]
    assert all(b <= a * (1 + 1e-6) for a, b in zip(vals, vals[1:])), vals


def test_the_loaded_model_renders(exported):
    m, back, _, _, _, data = exported
    with torch.no_grad():
        img = back(data)["render_img"]
        ref = m(data)["render_img"]
    assert img.shape == (H, W, 3) and bool(torch.isfinite(img).all())
    assert float(ref.std()) > 0.01                                                          # the view shows the scene
    print(f"[compress] render: mean |compact - original| = {float((img - ref).abs().mean()):.4f}")
