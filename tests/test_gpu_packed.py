"""`rasterization(packed=True)` and `sparse_grad=True` on the GPU (gs_packed.hip: gs_pack_flags, gs_pack_gather,
gs_pack_take, gs_pack_remap).  The reference of every assertion is this package's own `packed=False` call on the same inputs in the same
process -- the dense pipeline runs unchanged under the keyword, so everything is `torch.equal`: images, alphas, every input gradient,
and the packed meta against tests/packed_ref.py applied to the dense meta.

Scenes, the smallest at which the compaction can still go wrong:
  A  C = 3, N = 1000 (no multiple of a block), 64 x 48.  By construction: [256, 512) is behind camera 0 and off camera 2's image (a
     culled run that starts and ends on the edges of the gather kernel's 256-thread blocks, seen by camera 1 alone); every third Gaussian
     of [600, 850) is behind camera 1 and off camera 2; [850, 1000) is seen by nobody.
  B  C = 2, N = 8 390 000: C*N = 16 780 000 exceeds the 1024 x 16384 = 16 777 216 elements one pass of gs_scan_rows_i32's second level
     (scan_blocksums_kernel: 1024 block sums per pass, one block sum per 16384-element chunk) covers, so the carry between passes is used.
  C  C = 1, N = 1.   D  N = 0.   E  everything behind the cameras.
Every camera of A and B sees between 20 % and 80 % of the cloud (asserted)."""
import math

import pytest
import torch

import packed_ref as PR

pytestmark = pytest.mark.gpu
SCAN_CHUNK, SCAN_PASS = 16384, 1024   # gs_refine.hip: kScanChunk, kScanThreads (block sums per pass of the second level)
DIST = 4.0


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rot_y(deg, tx=0.0):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [[c, 0.0, s, tx], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, DIST], [0.0, 0.0, 0.0, 1.0]]


def _scene(name):
    """-> dict(means, quats, scales, opacities [tensors on the device], viewmats, Ks, W, H, N, C)."""
    d = dev()
    g = torch.Generator(device=d).manual_seed({"A": 1, "B": 2, "C": 3, "D": 4, "E": 5}[name])
    U = lambda *s: torch.rand(*s, generator=g, device=d)
    W, H = 64, 48
    if name == "A":
        N, cams = 1000, [_rot_y(0), _rot_y(180), _rot_y(90)]
        means = (U(N, 3) * 2 - 1) * 0.4
        n = torch.arange(N, device=d)
        means[(n >= 256) & (n < 512), 2] -= 2 * DIST
        means[(n >= 600) & (n < 850) & (n % 3 == 0), 2] += 2 * DIST
        means[n >= 850, 1] += 100.0
    elif name == "B":
        # two cameras side by side looking the same way: each sees a band of x, the bands overlap in the middle
        N, cams, W, H = 8_390_000, [_rot_y(0, 1.5), _rot_y(0, -1.5)], 512, 384
        means = (U(N, 3) * 2 - 1) * torch.tensor([4.6, 1.5, 0.3], device=d)
    elif name == "C":
        N, cams, means = 1, [_rot_y(0)], torch.tensor([[0.05, -0.02, 0.1]], device=d)
    elif name == "D":
        N, cams, means = 0, [_rot_y(0), _rot_y(180)], torch.zeros((0, 3), device=d)
    else:
        N, cams = 300, [_rot_y(0), _rot_y(0, 0.5)]
        means = (U(N, 3) * 2 - 1) * 0.4
        means[:, 2] -= 3 * DIST
    f = W / (2.0 * math.tan(math.radians(30.0)))
    K = torch.tensor([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], device=d)
    tiny = name == "B"   # (sub-pixel splats: short lists at 8 M Gaussians)
    return dict(means=means.contiguous(), quats=torch.randn(N, 4, generator=g, device=d),
                scales=torch.exp(U(N, 3) * math.log(3.0)) * (0.002 if tiny else 0.02), opacities=0.3 + 0.6 * U(N),
                viewmats=torch.tensor(cams, device=d), Ks=K[None].repeat(len(cams), 1, 1).contiguous(), W=W, H=H, N=N, C=len(cams), gen=g)


def _colors(sc, kind):
    """-> (colors argument as a list of tensors, sh_degree, channels)."""
    N, g, d = sc["N"], sc["gen"], dev()
    R = lambda *s: torch.randn(*s, generator=g, device=d)
    if kind == "sh0":
        return [R(N, 1, 3)], 0, 3
    if kind == "sh3pair":
        return [R(N, 1, 3), R(N, 15, 3) * 0.1], 3, 3
    D = {"feat3": 3, "feat4": 4, "feat8": 8}[kind]
    return [torch.rand(N, D, generator=g, device=d)], None, D


class Render:
    """One call, dense or packed, on clones of the scene's tensors; `.grads()` runs the backward of a fixed random functional of the
    image and the alphas and returns {name: gradient}."""
    NAMES = ("means", "quats", "scales", "opacities")

    def __init__(self, sc, cols, sh_degree, grad=True, cam_grads=False, raw=False, **kw):
        from easy_gaussian_splatting_amd.rendering import rasterization
        t = {k: sc[k].clone() for k in self.NAMES}
        if raw:
            t["scales"], t["opacities"] = t["scales"].log(), torch.logit(t["opacities"])
        self.ins = {k: t[k].requires_grad_(grad) for k in self.NAMES}
        cs = [c.clone().requires_grad_(grad) for c in cols]
        self.ins.update({f"colors{i}": c for i, c in enumerate(cs)})
        vm = sc["viewmats"].clone().requires_grad_(True) if cam_grads else sc["viewmats"]
        if cam_grads:
            self.ins["viewmats"] = vm
        with torch.set_grad_enabled(grad):
            self.img, self.alpha, self.meta = rasterization(
                *(self.ins[k] for k in self.NAMES), tuple(cs) if len(cs) == 2 else cs[0], vm, sc["Ks"], sc["W"], sc["H"],
                sh_degree=sh_degree, _camera_grads=cam_grads, **kw)

    def loss(self):
        g = torch.Generator(device=dev()).manual_seed(77)
        vc = torch.randn(self.img.shape, generator=g, device=dev())
        va = torch.randn(self.alpha.shape, generator=g, device=dev())
        return (self.img * vc).sum() + (self.alpha * va).sum()

    def grads(self):
        gs = torch.autograd.grad(self.loss(), list(self.ins.values()))
        return dict(zip(self.ins, gs))


def _same(got, ref, what):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got, ref), what


PER_PAIR = ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss")
LISTS = ("tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets")


def _check_meta(mp, md, C, N):
    """Packed meta `mp` against tests/packed_ref.py applied to the dense meta `md`; returns (camera_ids, gaussian_ids)."""
    dense = {k: (md[k].detach() if torch.is_tensor(md[k]) else md[k]) for k in PER_PAIR + LISTS}
    ref = PR.pack_meta(dense)
    nnz = int((dense["radii"] > 0).sum())
    for k in ("camera_ids", "gaussian_ids") + PER_PAIR + LISTS:
        _same(mp[k].detach(), ref[k], k)
    assert mp["camera_ids"].dtype == mp["gaussian_ids"].dtype == torch.int64 and mp["camera_ids"].shape == (nnz,)
    assert mp["radii"].dtype == mp["tiles_per_gauss"].dtype == mp["flatten_ids"].dtype == torch.int32
    assert mp["means2d"].shape == (nnz, 2) and mp["conics"].shape == (nnz, 3) and mp["depths"].shape == (nnz,) and mp["opacities"].shape == (nnz,)
    for k in ("width", "height", "tile_size", "n_cameras", "tile_width", "tile_height"):
        assert mp[k] == md[k]
    # flatten_ids indexes the packed rows
    fid, dfid = mp["flatten_ids"].long(), dense["flatten_ids"].long()
    if N:
        assert torch.equal(mp["gaussian_ids"][fid], dfid % N) and torch.equal(mp["camera_ids"][fid], dfid // N)
    return mp["camera_ids"], mp["gaussian_ids"]


def _visible_share(radii):
    return (radii > 0).float().mean(dim=1).tolist()


@pytest.mark.parametrize("culling", ["gsplat", "tight", "gsplat_eager"])
def test_scene_a_image_and_meta(culling):
    sc = _scene("A")
    cols, deg, _ = _colors(sc, "sh0")
    rd = Render(sc, cols, deg, grad=False, packed=False, _tile_culling=culling)
    rp = Render(sc, cols, deg, grad=False, packed=True, _tile_culling=culling)
    _same(rp.img, rd.img, "render_colors")
    _same(rp.alpha, rd.alpha, "render_alphas")
    radii = rd.meta["radii"]
    share = _visible_share(radii)
    print("scene A visible share per camera:", share)
    assert all(0.2 <= s <= 0.8 for s in share), share
    # the construction: a culled run of camera 0 on block edges, Gaussians one camera sees and another does not, some nobody sees
    v = radii > 0
    assert not v[0, 256:512].any() and v[0, 255] and v[0, 512] and v[1, 256:512].all() and not v[2, 256:512].any()
    assert v[0, 600] and not v[1, 600] and v[1, 601] and not v[:, 850:].any()
    _check_meta(rp.meta, rd.meta, sc["C"], sc["N"])


def test_scene_b_crosses_the_second_scan_level():
    sc = _scene("B")
    C, N = sc["C"], sc["N"]
    assert C == 2 and C * N > SCAN_PASS * SCAN_CHUNK, (C * N, SCAN_PASS * SCAN_CHUNK)
    cols, deg, _ = _colors(sc, "sh0")
    rd = Render(sc, cols, deg, packed=False, _tile_culling="tight")
    rp = Render(sc, cols, deg, packed=True, sparse_grad=True, _tile_culling="tight")
    _same(rp.img.detach(), rd.img.detach(), "render_colors")
    share = _visible_share(rd.meta["radii"])
    print("scene B visible share per camera:", share, "nnz / (C N):", sum(share) / C)
    assert all(0.2 <= s <= 0.8 for s in share), share
    _check_meta(rp.meta, rd.meta, C, N)
    gd, gp = rd.grads(), rp.grads()
    union = PR.union_ids(rd.meta["radii"])
    assert 0 < union.numel() < N
    for k in ("means", "quats", "scales"):
        assert gp[k].is_sparse and torch.equal(gp[k]._indices(), union[None])
        _same(gp[k].to_dense(), gd[k], k)
    _same(gp["opacities"], gd["opacities"], "opacities")


def test_scene_c_one_pair():
    sc = _scene("C")
    cols, deg, _ = _colors(sc, "sh0")
    rd, rp = Render(sc, cols, deg, packed=False, absgrad=True), Render(sc, cols, deg, packed=True, absgrad=True)
    assert int(rd.meta["radii"][0, 0]) > 0
    _same(rp.img.detach(), rd.img.detach(), "render_colors")
    _check_meta(rp.meta, rd.meta, 1, 1)
    gd, gp = rd.grads(), rp.grads()
    for k in gd:
        _same(gp[k], gd[k], k)
    _same(rp.meta["means2d"].absgrad, rd.meta["means2d"].absgrad.reshape(1, 2), "absgrad")


@pytest.mark.parametrize("kind", ["sh3pair", "feat4"])
def test_backward_with_absgrad(kind):
    sc = _scene("A")
    cols, deg, D = _colors(sc, kind)
    bg = torch.rand(sc["C"], D, generator=sc["gen"], device=dev())
    rd = Render(sc, cols, deg, packed=False, absgrad=True, backgrounds=bg)
    rp = Render(sc, cols, deg, packed=True, absgrad=True, backgrounds=bg)
    _same(rp.img.detach(), rd.img.detach(), "render_colors")
    _same(rp.alpha.detach(), rd.alpha.detach(), "render_alphas")
    cam, gid = _check_meta(rp.meta, rd.meta, sc["C"], sc["N"])
    assert rp.meta["means2d"].requires_grad and rp.meta["means2d"].is_leaf
    gd, gp = rd.grads(), rp.grads()
    assert set(gp) == set(gd) and len(gd) == (6 if kind == "sh3pair" else 5)
    for k in gd:
        assert not gp[k].is_sparse
        _same(gp[k], gd[k], k)
    md, mp = rd.meta["means2d"], rp.meta["means2d"]
    assert float(md.absgrad.abs().max()) > 0 and float(md.grad.abs().max()) > 0
    _same(mp.absgrad, md.absgrad[cam, gid], "means2d.absgrad")
    _same(mp.grad, md.grad[cam, gid], "means2d.grad")


def test_sparse_grad_and_sparse_adam():
    sc = _scene("A")
    cols, deg, _ = _colors(sc, "sh0")
    N = sc["N"]
    rd = Render(sc, cols, deg, packed=False)
    rp = Render(sc, cols, deg, packed=True, sparse_grad=True)
    gd, gp = rd.grads(), rp.grads()
    union = PR.union_ids(rd.meta["radii"])
    unseen = torch.ones(N, dtype=torch.bool, device=dev())
    unseen[union] = False
    assert 0 < union.numel() < N and int(unseen.sum()) >= 150
    for k, w in (("means", 3), ("quats", 4), ("scales", 3)):
        g = gp[k]
        assert g.is_sparse and g.is_coalesced() and g.shape == (N, w)
        idx = g._indices()
        assert idx.dtype == torch.int64 and idx.shape == (1, union.numel()) and torch.equal(idx[0], union)
        assert bool((idx[0, 1:] > idx[0, :-1]).all())
        _same(g._values(), gd[k][union], k + " values")
        _same(g.to_dense(), gd[k], k)
        assert float(gd[k][unseen].abs().max()) == 0.0, k   # the dense gradient of a Gaussian no camera saw is zero
    for k in ("opacities", "colors0"):
        assert not gp[k].is_sparse
        _same(gp[k], gd[k], k)
    # one torch.optim.SparseAdam step through .backward(): unseen rows keep their bits, seen rows with a gradient move
    r = Render(sc, cols, deg, packed=True, sparse_grad=True)
    params = [r.ins[k] for k in ("means", "quats", "scales")]
    before = [p.detach().clone() for p in params]
    r.loss().backward()
    assert all(p.grad.is_sparse for p in params) and not r.ins["opacities"].grad.is_sparse
    torch.optim.SparseAdam(params, lr=1e-2).step()
    for p, b, k in zip(params, before, ("means", "quats", "scales")):
        moved = (p.detach() != b).any(dim=1)
        assert not moved[unseen].any(), k
        # (a seen Gaussian whose gradient row is zero -- listed, never taken by a pixel -- has nothing to move by; one whose gradient
        #  is far above Adam's eps = 1e-8 moves by about lr)
        has_grad, clear_grad = (gd[k] != 0).any(dim=1), (gd[k].abs() > 1e-6).any(dim=1)
        assert not moved[~has_grad].any() and moved[clear_grad].all() and int(clear_grad.sum()) > union.numel() // 2, k


def _ride(kind="sh0", absgrad=True, packed_kw=None, **kw):
    """Scene A under the keywords `kw`, dense and packed (the packed call also under `packed_kw`): image, alphas, meta, every gradient."""
    sc = _scene("A")
    cols, deg, _ = _colors(sc, kind)
    rd = Render(sc, cols, deg, packed=False, absgrad=absgrad, **kw)
    rp = Render(sc, cols, deg, packed=True, absgrad=absgrad, **kw, **(packed_kw or {}))
    _same(rp.img.detach(), rd.img.detach(), "render_colors")
    _same(rp.alpha.detach(), rd.alpha.detach(), "render_alphas")
    cam, gid = _check_meta(rp.meta, rd.meta, sc["C"], sc["N"])
    gd, gp = rd.grads(), rp.grads()
    for k in gd:
        _same(gp[k].to_dense() if gp[k].is_sparse else gp[k], gd[k], k)
    if absgrad:
        _same(rp.meta["means2d"].absgrad, rd.meta["means2d"].absgrad[cam, gid], "means2d.absgrad")
    _same(rp.meta["means2d"].grad, rd.meta["means2d"].grad[cam, gid], "means2d.grad")
    return sc, rd, rp, gd, gp


def test_rides_along_expected_depth():
    sc, rd, rp, _, _ = _ride(render_mode="RGB+ED")
    assert rp.img.shape[-1] == 4


def test_rides_along_fisheye():
    _ride(camera_model="fisheye")


def test_rides_along_antialiased():
    sc, rd, rp, _, _ = _ride(rasterize_mode="antialiased")
    # meta["opacities"] carries rho: below the input opacity for every visible pair
    op = sc["opacities"][rp.meta["gaussian_ids"]]
    assert bool((rp.meta["opacities"] < op).all()) and bool((rp.meta["opacities"] > 0).any())


def test_rides_along_activations_with_sparse_grad():
    sc, rd, rp, gd, gp = _ride(_activations="exp_sigmoid", raw=True, packed_kw=dict(sparse_grad=True))
    assert gp["scales"].is_sparse and gp["means"].is_sparse and not gp["opacities"].is_sparse
    _same(rp.meta["opacities"], torch.logit(sc["opacities"])[rp.meta["gaussian_ids"]], "logits")


def test_rides_along_eight_feature_channels():
    sc, rd, rp, _, _ = _ride(kind="feat8", absgrad=False)
    assert rp.img.shape[-1] == 8


def test_rides_along_camera_grads():
    sc, rd, rp, gd, gp = _ride(kind="sh3pair", cam_grads=True)
    assert float(gd["viewmats"].abs().max()) > 0 and not gp["viewmats"].is_sparse


@pytest.mark.parametrize("name", ["D", "E"])
def test_empty_scenes(name):
    sc = _scene(name)
    C, N, W, H = sc["C"], sc["N"], sc["W"], sc["H"]
    cols, deg, _ = _colors(sc, "sh0")
    bg = torch.tensor([[0.25, 0.5, 0.75]], device=dev()).repeat(C, 1)
    rp = Render(sc, cols, deg, packed=True, sparse_grad=True, absgrad=True, backgrounds=bg)
    m = rp.meta
    assert torch.equal(rp.img.detach(), bg[:, None, None, :].expand(C, H, W, 3)) and float(rp.alpha.detach().abs().max()) == 0.0
    want = {"camera_ids": (torch.int64, (0,)), "gaussian_ids": (torch.int64, (0,)), "radii": (torch.int32, (0,)), "means2d": (torch.float32, (0, 2)),
            "depths": (torch.float32, (0,)), "conics": (torch.float32, (0, 3)), "opacities": (torch.float32, (0,)),
            "tiles_per_gauss": (torch.int32, (0,)), "flatten_ids": (torch.int32, (0,)), "isect_ids": (torch.int64, (0,))}
    for k, (dt, shp) in want.items():
        assert m[k].dtype == dt and tuple(m[k].shape) == shp, (k, m[k].dtype, tuple(m[k].shape))
    assert tuple(m["isect_offsets"].shape) == (C, math.ceil(H / 16), math.ceil(W / 16)) and int(m["isect_offsets"].abs().max()) == 0
    g = rp.grads()
    for k, w in (("means", 3), ("quats", 4), ("scales", 3)):
        assert g[k].is_sparse and g[k].shape == (N, w) and g[k]._indices().shape == (1, 0) and g[k]._values().shape == (0, w)
        assert g[k].to_dense().shape == (N, w) and float(g[k].to_dense().abs().sum()) == 0.0
    assert g["opacities"].shape == (N,) and not g["opacities"].is_sparse
    assert m["means2d"].grad.shape == (0, 2) and m["means2d"].absgrad.shape == (0, 2)


def test_default_call_is_packed():
    from easy_gaussian_splatting_amd.rendering import rasterization
    sc = _scene("A")
    cols, deg, _ = _colors(sc, "sh0")
    with torch.no_grad():
        img, alpha, meta = rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], cols[0], sc["viewmats"], sc["Ks"], sc["W"], sc["H"],
                                         sh_degree=deg)
        img_d, _, meta_d = rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], cols[0], sc["viewmats"], sc["Ks"], sc["W"],
                                         sc["H"], sh_degree=deg, packed=False)
    nnz = int((meta_d["radii"] > 0).sum())
    assert meta["camera_ids"].shape == (nnz,) and meta["radii"].shape == (nnz,) and meta["means2d"].shape == (nnz, 2)
    _same(img, img_d, "render_colors")


def test_fused_adam_refuses_sparse_grads():
    from easy_gaussian_splatting_amd.optim import FusedAdam
    sc = _scene("A")
    cols, deg, _ = _colors(sc, "sh0")
    r = Render(sc, cols, deg, packed=True, sparse_grad=True)
    means = r.ins["means"]
    opt = FusedAdam([{"params": [means], "lr": 1e-2, "name": "means"}])
    before = means.detach().clone()
    r.loss().backward()
    assert means.grad.is_sparse
    with pytest.raises(TypeError, match=r"step\(visible=.*torch\.optim\.SparseAdam"):
        opt.step()
    assert torch.equal(means.detach(), before)


def test_nothing_without_the_keyword(monkeypatch):
    from easy_gaussian_splatting_amd import rendering as R
    sc = _scene("A")
    cols, deg, _ = _colors(sc, "sh0")
    Render(sc, cols, deg, packed=False, absgrad=True).grads()   # (capacities of this call shape learnt: no repeated attempt below)
    names = []
    real = R._stage
    monkeypatch.setattr(R, "_stage", lambda name, device, thunk: (names.append(name), real(name, device, thunk))[1])
    rd = Render(sc, cols, deg, packed=False, absgrad=True)
    rd.grads()
    dense_names = list(names)
    assert dense_names and not [n for n in dense_names if "pack" in n], dense_names
    assert rd.meta["camera_ids"] is None and rd.meta["gaussian_ids"] is None and rd.meta["radii"].shape == (sc["C"], sc["N"])
    del names[:]
    rp = Render(sc, cols, deg, packed=True, absgrad=True)
    rp.grads()
    # the packed call: the dense call's stages in the dense call's order, and the packing stages among them
    assert [n for n in names if "pack" not in n] == dense_names
    assert names.count("gs_pack_flags") == 1 and names.count("gs_pack_gather") == 1 and "gs_pack_take" in names
