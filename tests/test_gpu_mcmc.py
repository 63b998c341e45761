"""Training to a Gaussian budget on the device (easy_gaussian_splatting_amd/mcmc.py, csrc/gs_mcmc.hip) against the independent
reference of tests/mcmc_ref.py, seam by seam: weights, CDF (bit-exact), draws (exact), relocate and grow through the strategy
(values within 2 float32 ulp, everything else bit for bit), noise, and a short run that reaches its cap."""
import math

import numpy as np
import pytest
import torch

import adam_ref
import mcmc_ref as R
from easy_gaussian_splatting_amd import mcmc as M
from easy_gaussian_splatting_amd.loss import LossComputer
from easy_gaussian_splatting_amd.model import GaussianModel, build_optimizers
from easy_gaussian_splatting_amd.optim import FusedAdam
from scenes import make_scene

pytestmark = pytest.mark.gpu

MIN_OPACITY = 0.005
LRS = (1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2)


def dev():
    return torch.device("cuda:0")


def host(t):
    return t.detach().cpu().numpy()


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def as_int64(b):
    """a Python integer in [0, 2^64) as the int64 with the same bits"""
    return b - 2 ** 64 if b >= 2 ** 63 else b


# ---- (a) weights ----

def test_weights_and_dead_flags():
    l0 = np.float32(math.log(MIN_OPACITY / (1 - MIN_OPACITY)))
    rng = np.random.default_rng(1)
    fixed = np.array([30, -30, 0, l0, np.nextafter(l0, np.float32(-np.inf)), np.nextafter(l0, np.float32(np.inf)), 88, -88, 17, -17],
                     dtype=np.float32)
    logits = np.concatenate([fixed, (rng.standard_normal(4000) * 4).astype(np.float32)])
    w, dead = M.opacity_weights(torch.from_numpy(logits).to(dev()), MIN_OPACITY)
    w_ref, dead_ref, o = R.weights(logits, MIN_OPACITY)
    clear = np.abs(o - MIN_OPACITY) > 1e-12
    assert (~clear).sum() <= 2
    assert np.array_equal(host(dead)[clear].astype(bool), dead_ref[clear])
    diff = np.abs(host(w).astype(np.int64) - w_ref)
    print(f"[mcmc] weights: {int((~clear).sum())} at the threshold, max |w - ref| = {int(diff.max())}, {int(dead_ref.sum())} dead")
    assert diff.max() <= 1
    assert host(w).max() == 2 ** 24 and (host(w)[~host(dead).astype(bool)] >= 1).all() and (host(w)[host(dead).astype(bool)] == 0).all()
    # grow: nothing is dead, every weight at least 1
    wg, dg = M.opacity_weights(torch.from_numpy(logits).to(dev()), MIN_OPACITY, grow=True)
    wg_ref, _, _ = R.weights(logits, MIN_OPACITY, grow=True)
    assert not host(dg).any() and host(wg).min() == 1 and np.abs(host(wg).astype(np.int64) - wg_ref).max() <= 1
    e = M.opacity_weights(torch.empty(0, device=dev()), MIN_OPACITY)
    assert e[0].shape == (0,) and e[1].shape == (0,)


# ---- (b) the CDF ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3 * 256 + 17, 2047, 2048, 2049, 200_003, 600_001])
def test_cdf_is_bit_exact(n):
    """block = 2048 weights; 200 003 needs the second level, 600 001 takes its loop round twice (more than 256 block sums)"""
    rng = np.random.default_rng(n)
    w = rng.integers(0, 2 ** 24, n, endpoint=True)
    w[rng.random(n) < 0.2] = 0
    w[rng.random(n) < 0.1] = 2 ** 24
    got = host(M.weight_cdf(torch.from_numpy(w.astype(np.int32)).to(dev())))
    assert got.dtype == np.int64 and got.tolist() == R.cdf(w)
    if n >= 1000:
        assert got[-1] > 2 ** 32


def test_cdf_of_zeros_and_of_nothing():
    assert not host(M.weight_cdf(torch.zeros(5000, dtype=torch.int32, device=dev()))).any()
    assert M.weight_cdf(torch.zeros(0, dtype=torch.int32, device=dev())).shape == (0,)


# ---- (c) draws ----

def bits_for(t, total):
    """a word b with mulhi64(b, total) == t"""
    b = -((-t * 2 ** 64) // total)
    assert 0 <= b < 2 ** 64 and R.mulhi64(b, total) == t
    return b


def test_draws_are_the_references_given_the_devices_weights():
    n, edge = 2048 + 300, 2048   # the scan's block edge
    rng = np.random.default_rng(7)
    logits = (rng.standard_normal(n) * 3).astype(np.float32)
    logits[edge - 8:edge + 12] = -30.0                     # a run of zero weights across the block edge
    logits[edge - 9], logits[edge + 12], logits[0], logits[n - 1] = 1.0, 0.5, 2.0, -1.0
    w, dead = M.opacity_weights(torch.from_numpy(logits).to(dev()), MIN_OPACITY)
    w_host = host(w).astype(np.int64)
    n_dead = int(host(dead).sum())
    assert (w_host[edge - 8:edge + 12] == 0).all() and 40 <= n_dead <= 400
    c = R.cdf(w_host)
    total = c[-1]
    words = [0, 2 ** 64 - 1, 2 ** 63, 1]
    for i in (0, 255, 256, edge - 9, edge - 1, edge, edge + 11, edge + 12, n - 2, n - 1):
        for t in (c[i], c[i] - 1):
            if 0 <= t < total:
                words.append(bits_for(t, total))
    assert len(words) <= n_dead
    bits = rng.integers(-2 ** 63, 2 ** 63, n, dtype=np.int64)
    bits[:len(words)] = [as_int64(b) for b in words]
    tb = torch.from_numpy(bits).to(dev())
    # relocate: as many draws as dead Gaussians, counted on the device
    src, counts, nd = M.sample_by_weight(w, tb, dead=dead)
    src_ref, counts_ref = R.draws(w_host, bits, n_dead)
    assert int(nd) == n_dead and host(src)[:n_dead].tolist() == src_ref and (host(src)[n_dead:] == -1).all()
    assert np.array_equal(host(counts), counts_ref) and (w_host[src_ref] > 0).all()
    assert src_ref[0] == 0 and src_ref[1] == int(np.nonzero(w_host)[0][-1])
    assert edge + 12 in src_ref and edge - 9 in src_ref       # behind and in front of the run of zeros
    dst = M._sample(w, tb, None, dead)["dst"]
    assert host(dst)[:n_dead].tolist() == np.nonzero(w_host == 0)[0].tolist() and (host(dst)[n_dead:] == -1).all()
    # grow: the host-known number of draws
    for k in (0, 1, len(words), 257):
        src, counts, nd = M.sample_by_weight(w, tb[:k], n_draws=k)
        src_ref, counts_ref = R.draws(w_host, bits, k)
        assert int(nd) == k and host(src).tolist() == src_ref and np.array_equal(host(counts), counts_ref)
    assert host(M._sample(w, tb, 5, None)["dst"]).tolist() == [n, n + 1, n + 2, n + 3, n + 4]


def test_draws_when_all_or_none_or_all_but_one_are_dead():
    d = dev()
    bits = M.random_bits(101, d, torch.Generator(device=d).manual_seed(3))
    for logits, want_draws in ((torch.full((101,), -30.0), 0), (torch.full((101,), 1.5), 0)):
        w, dead = M.opacity_weights(logits.to(d), MIN_OPACITY)
        src, counts, nd = M.sample_by_weight(w, bits, dead=dead)
        assert int(nd) == want_draws and (host(src) == -1).all() and not host(counts).any()
    # every weight zero: no draws in grow mode either
    src, counts, nd = M.sample_by_weight(torch.zeros(101, dtype=torch.int32, device=d), bits, n_draws=7)
    assert int(nd) == 0 and (host(src) == -1).all() and not host(counts).any()
    logits = torch.full((101,), -30.0)
    logits[37] = 0.3
    w, dead = M.opacity_weights(logits.to(d), MIN_OPACITY)
    src, counts, nd = M.sample_by_weight(w, bits, dead=dead)
    want = np.zeros(101, dtype=np.int32)
    want[37] = 100
    assert int(nd) == 100 and (host(src)[:100] == 37).all() and host(src)[100] == -1 and np.array_equal(host(counts), want)


def test_relocation_values_seam():
    rng = np.random.default_rng(11)
    n = 300
    o = rng.uniform(0.006, 0.999, n).astype(np.float32)
    s = rng.uniform(0.01, 2.0, (n, 3)).astype(np.float32)
    ratio = rng.integers(1, 60, n).astype(np.int32)
    ratio[:4] = [1, 2, 51, 1000]
    no, ns = M.relocation_values(*(torch.from_numpy(x).to(dev()) for x in (o, s, ratio)))
    ref = [R.relocation_values(float(o[i]), s[i], int(ratio[i])) for i in range(n)]
    ref_o, ref_s = np.float32([r[0] for r in ref]), np.stack([r[1] for r in ref]).astype(np.float32)
    du, ds = R.ulp_distance(host(no), ref_o).max(), R.ulp_distance(host(ns), ref_s).max()
    print(f"[mcmc] relocation_values: {du} ulp on o', {ds} ulp on s'")
    assert du <= 2 and ds <= 2
    one = ratio == 1
    assert np.array_equal(host(no)[one], o[one]) and np.array_equal(host(ns)[one], s[one])


# ---- (d) relocate and grow through the strategy ----

def make_model(n, K, seed, logits=None, scale_range=(0.01, 0.5)):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    scales = torch.exp(torch.rand(n, 3, generator=g) * math.log(scale_range[1] / scale_range[0]) + math.log(scale_range[0]))
    if logits is None:
        logits = r(n) * 2.5 - 2.0                                           # about one in eleven is dead
        near = (torch.sigmoid(logits) - MIN_OPACITY).abs() < 1e-4          # off the threshold: both sides agree on who is dead
        logits = torch.where(near, logits + 0.5, logits)
    sh_degree = {1: 0, 4: 1, 9: 2, 16: 3}[K]
    m = GaussianModel(means=r(n, 3), log_scales=torch.log(scales), quats=r(n, 4) * 2, sh_0=r(n, 1, 3), sh_rest=r(n, K - 1, 3) * 0.1,
                      logit_opacities=logits, sh_degree=sh_degree).to(dev())
    opt = build_optimizers(m, *LRS, fused="hip")
    gd = torch.Generator(device=dev()).manual_seed(seed + 100)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, device=dev(), generator=gd) + 3.0)         # non-zero everywhere, pads included
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, device=dev(), generator=gd) + 0.5)
    return m, opt


def snapshot(opt):
    return host(opt.flat_param).copy(), host(opt.exp_avg).copy(), host(opt.exp_avg_sq).copy()


def check_against_apply(opt, ref, n_rows, K, offs, label):
    """Device buffers against R.apply's: logit_opacities / log_scales of the rewritten rows within 2 float32 ulp, every other
    element of the three flat buffers bit for bit (pads included)."""
    p_ref, m_ref, v_ref, touched = ref
    p, m, v = snapshot(opt)
    assert p.shape == p_ref.shape
    loose = np.zeros(p.shape, dtype=bool)
    rows = np.array(sorted(touched), dtype=np.int64)
    for t in (1, 5):
        wd = R.WIDTHS(K)[t]
        idx = (offs[t] + rows[:, None] * wd + np.arange(wd)[None, :]).reshape(-1)
        loose[idx] = True
    assert np.array_equal(bits_of(p)[~loose], bits_of(p_ref)[~loose]), label
    ulps = R.ulp_distance(p[loose], p_ref[loose])
    print(f"[mcmc] {label}: {len(rows)} rows rewritten, values at most {int(ulps.max()) if ulps.size else 0} ulp from the reference")
    assert ulps.size == 0 or ulps.max() <= 2, label
    assert np.array_equal(bits_of(m), bits_of(m_ref)) and np.array_equal(bits_of(v), bits_of(v_ref)), label
    return p, m, v


@pytest.mark.parametrize("K", [1, 16])
def test_relocate_through_the_strategy(K):
    n = 1003
    model, opt = make_model(n, K, 20 + K)
    st = M.MCMCStrategy(model, cap_max=n, generator=torch.Generator(device=dev()).manual_seed(5))
    before = snapshot(opt)
    offs = list(opt._offs)
    logits = host(model.logit_opacities).copy()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")     # a host synchronisation inside relocate() raises
    try:
        info = st.relocate()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    nd = int(info["n_dead"])
    src, dst, counts = host(info["src"]), host(info["dst"]), host(info["counts"])
    w_ref, dead_ref, o = R.weights(logits, MIN_OPACITY)
    assert np.abs(o - MIN_OPACITY).min() > 1e-6 and 20 <= dead_ref.sum() == nd
    assert dst[:nd].tolist() == np.nonzero(dead_ref)[0].tolist() and (src[nd:] == -1).all() and (dst[nd:] == -1).all()
    assert not dead_ref[src[:nd]].any() and np.array_equal(counts, np.bincount(src[:nd], minlength=n))
    assert model.nbr_gaussians == n and opt.flat_param.data_ptr() == model.means.data_ptr()
    ref = R.apply(*before, n, n, K, offs, src[:nd], dst[:nd], counts, MIN_OPACITY)
    p, m, v = check_against_apply(opt, ref, n, K, offs, f"relocate K={K}")
    # the destinations are their sources' rows, bit for bit, in all six tensors; sources and destinations start Adam afresh
    P, M_, V_ = (R.split_flat(x, n, K, offs) for x in (p, m, v))
    M0 = R.split_flat(before[1], n, K, offs)
    for t in range(6):
        assert np.array_equal(bits_of(P[t][dst[:nd]]), bits_of(P[t][src[:nd]])), t
        rows = np.union1d(src[:nd], dst[:nd])
        assert not M_[t][rows].any() and not V_[t][rows].any() and (M0[t][rows] != 0).all()
    assert (P[5][src[:nd], 0] < logits[src[:nd]]).all()      # shared out: every source got more transparent


def test_relocate_onto_one_survivor_clamps_the_ratio_at_51():
    n, K, alive = 1000, 4, 123
    logits = torch.full((n,), -9.0)
    logits[alive] = 2.0
    model, opt = make_model(n, K, 31, logits=logits)
    st = M.MCMCStrategy(model, cap_max=n, generator=torch.Generator(device=dev()).manual_seed(6))
    before = snapshot(opt)
    offs = list(opt._offs)
    info = st.relocate()
    counts = host(info["counts"])
    assert int(info["n_dead"]) == n - 1 and counts[alive] == n - 1 and counts.sum() == n - 1
    ref = R.apply(*before, n, n, K, offs, host(info["src"])[:n - 1], host(info["dst"])[:n - 1], counts, MIN_OPACITY)
    p, _, _ = check_against_apply(opt, ref, n, K, offs, "one survivor")
    P, P0 = R.split_flat(p, n, K, offs), R.split_flat(before[0], n, K, offs)
    o = float(R.sigmoid(P0[5][alive, 0]))
    s = np.exp(P0[1][alive].astype(np.float64))
    on51, s51 = R.relocation_values(o, s, 51)
    on50, s50 = R.relocation_values_plain(o, s, 50)
    want = np.float32(np.log(s51))
    assert R.ulp_distance(P[1][alive], want).max() <= 2 and R.ulp_distance(np.float32(np.log(s50)), want).min() > 2
    assert R.ulp_distance(P[5][alive], np.float32([math.log(on51 / (1 - on51))])).max() <= 2
    for t in range(6):     # all thousand rows are the survivor's now
        assert (bits_of(P[t]) == bits_of(P[t][alive])).all()


def test_relocate_with_nobody_dead_changes_nothing():
    model, opt = make_model(300, 4, 41, logits=torch.linspace(-3.0, 4.0, 300))
    before = snapshot(opt)
    info = M.MCMCStrategy(model, cap_max=300).relocate()
    assert int(info["n_dead"]) == 0
    for a, b in zip(snapshot(opt), before):
        assert np.array_equal(bits_of(a), bits_of(b))


@pytest.mark.parametrize("K", [1, 16])
def test_grow_to_the_cap(K):
    n, cap = 1000, 1030
    model, opt = make_model(n, K, 50 + K)
    st = M.MCMCStrategy(model, cap_max=cap, generator=torch.Generator(device=dev()).manual_seed(9))
    before = snapshot(opt)
    old_offs = list(opt._offs)
    n_new = cap - n
    # what grow() will draw: the same words from a generator in the same state, the device's own grow-mode weights
    bits = host(M.random_bits(n_new, dev(), torch.Generator(device=dev()).manual_seed(9)))
    w, _ = M.opacity_weights(model.logit_opacities, MIN_OPACITY, grow=True)
    src_ref, counts_ref = R.draws(host(w).astype(np.int64), bits, n_new)
    step_before = opt._step
    assert st.grow() == n_new and model.nbr_gaussians == cap
    widths = R.WIDTHS(K)
    offs, _, total = FusedAdam.flat_layout([cap * wd for wd in widths])
    assert list(opt._offs) == offs and opt.flat_param.numel() == total and opt._step == step_before
    # the old buffers in the new layout: old rows and their moments kept, new rows and pads zero
    grown = [np.zeros(total, dtype=np.float32) for _ in range(3)]
    for big, old in zip(grown, before):
        for oo, no, wd in zip(old_offs, offs, widths):
            big[no:no + n * wd] = old[oo:oo + n * wd]
    ref = R.apply(*grown, n, cap, K, offs, src_ref, list(range(n, cap)), counts_ref, MIN_OPACITY)
    p, m, v = check_against_apply(opt, ref, cap, K, offs, f"grow K={K}")
    P = R.split_flat(p, cap, K, offs)
    for t in range(6):
        assert np.array_equal(bits_of(P[t][n:]), bits_of(P[t][src_ref])), t      # new rows equal their sources
    for name, wd, o_ in zip(model.param_names, widths, offs):
        prm = getattr(model, name)
        assert prm.shape[0] == cap and prm.numel() == cap * wd and (wd == 0 or prm.data_ptr() == opt.flat_param.data_ptr() + 4 * o_)
    for buf in (model.grad_norm_accum, model.collecting_counts, model.max_radii):
        assert buf.shape == (cap,) and not host(buf).any()
    assert st.grow() == 0 and model.nbr_gaussians == cap
    # the optimizer steps on the adopted buffers: a source, a new row and an untouched row against the fp64 Adam
    g = torch.Generator().manual_seed(1)
    grads = {}
    for name in model.param_names:
        grads[name] = torch.randn(getattr(model, name).shape, generator=g)
        getattr(model, name).grad = grads[name].to(dev())
    opt.step()
    untouched = next(i for i in range(n) if counts_ref[i] == 0)
    rows = [src_ref[0], n, cap - 1, untouched]
    p2, m2, v2 = snapshot(opt)
    b1, b2 = opt.defaults["betas"]
    for t, name in enumerate(model.param_names):
        wd = widths[t]
        if wd == 0:
            continue
        sl = lambda x: R.split_flat(x, cap, K, offs)[t][rows].astype(np.float64)
        gr = host(grads[name]).reshape(cap, wd)[rows]
        ref_step = adam_ref.adam_ref(sl(p), gr, sl(m), sl(v), LRS[t], opt._step, b1, b2, opt.defaults["eps"])
        ratios = adam_ref.error_ratios((sl(p2), sl(m2), sl(v2)), sl(p), ref_step)
        assert max(ratios["p"], ratios["m"], ratios["v"]) <= 1.0, (name, ratios)


# ---- (e) noise ----

@pytest.mark.parametrize("n", [1, 255, 257, 100_003])
def test_noise_on_the_means(n):
    gate_opacities = torch.tensor([0.001, 0.004, 0.005, 0.006, 0.5, 0.999])
    logits = torch.logit(gate_opacities[torch.arange(n) % 6])
    model, opt = make_model(n, 1, 60, logits=logits, scale_range=(0.05, 1.0))
    st = M.MCMCStrategy(model, cap_max=n, noise_lr=2.0, generator=torch.Generator(device=dev()).manual_seed(n))
    z = host(torch.randn((n, 3), device=dev(), generator=torch.Generator(device=dev()).manual_seed(n)))
    before = snapshot(opt)
    offs = list(opt._offs)
    P0 = R.split_flat(before[0], n, 1, offs)
    st.inject_noise(0.5)      # strength = noise_lr * means_lr = 1
    want = R.noise(P0[0], P0[1], P0[2], P0[5][:, 0], z, 1.0).astype(np.float32)
    p, m, v = snapshot(opt)
    got = R.split_flat(p, n, 1, offs)[0]
    ulps = R.ulp_distance(got, want)
    moved = np.abs(got - P0[0]).max(axis=1)
    print(f"[mcmc] noise n={n}: at most {int(ulps.max())} ulp from the reference, largest move {moved.max():.3g}")
    assert ulps.max() <= 2
    rest = np.ones(p.shape, dtype=bool)
    rest[offs[0]:offs[0] + 3 * n] = False
    assert np.array_equal(bits_of(p)[rest], bits_of(before[0])[rest])
    assert np.array_equal(bits_of(m), bits_of(before[1])) and np.array_equal(bits_of(v), bits_of(before[2]))
    # the gate: transparent Gaussians move, opaque ones stay where they are
    if n >= 255:
        k = np.arange(n) % 6
        assert moved[k == 0].max() > 1e-3 and moved[k == 4].max() == 0 and moved[k == 5].max() == 0


# ---- a short run ----

def test_a_short_run_reaches_its_cap_and_stays_there():
    d = dev()
    W, H, n0 = 64, 64, 2000
    sc = make_scene(n0, W, H, sh_degree=3, n_views=2, seed=12, scale_range=(0.03, 0.15), dist=4.0)
    T = lambda a: torch.from_numpy(a)

    def build(noise, seed):
        g = torch.Generator().manual_seed(seed)
        op = np.clip(sc["opacities"], 1e-3, 1 - 1e-3)
        shs = T(sc["shs"])
        return GaussianModel(means=T(sc["means"]) + noise * 0.03 * torch.randn(sc["means"].shape, generator=g),
                             log_scales=torch.log(T(sc["scales"])) + noise * 0.2 * torch.randn(sc["scales"].shape, generator=g),
                             quats=T(sc["quats"]), sh_0=(shs[:, :1] + noise * 0.5 * torch.randn(shs[:, :1].shape, generator=g)).contiguous(),
                             sh_rest=shs[:, 1:].contiguous() * (1 - noise), logit_opacities=T(np.log(op / (1 - op)).astype(np.float32)),
                             sh_degree=3, white_background=True).to(d)

    datas = [{"w2c": T(sc["viewmats"][v]).to(d), "K": T(sc["Ks"][v]).to(d), "width": W, "height": H} for v in range(2)]
    target_model = build(0.0, 0)
    with torch.no_grad():
        targets = [target_model(x)["render_img"] for x in datas]
    model = build(1.0, 1)
    opt = build_optimizers(model, 1.6e-4, 5e-3, 1e-3, 2.5e-2, 1.25e-3, 5e-2, fused="hip")
    cap = int(1.2 * n0)
    st = M.MCMCStrategy(model, cap_max=cap, refine_start=0, refine_stop=300, refine_every=50,
                        generator=torch.Generator(device=d).manual_seed(2))
    lc = LossComputer(0.2)
    losses, sizes = [], []
    for step in range(1, 301):
        v = step % 2
        out = model(datas[v])
        loss = lc.get_loss_dict(out["render_img"], targets[v])["total"]
        (loss + st.regularization()).backward()
        opt.step()
        opt.zero_grad()
        st.after_step(step)
        losses.append(loss.detach())
        sizes.append(model.nbr_gaussians)
    losses = torch.stack(losses).cpu().numpy()
    print(f"[mcmc] short run: N {n0} -> {sizes[-1]} (cap {cap}), loss {losses[:6].mean():.4f} -> {losses[-6:].mean():.4f}")
    assert max(sizes) <= cap and sizes[-1] == cap and sizes == sorted(sizes) and sizes[48] == n0 and sizes[49] == int(1.05 * n0)
    for name in model.param_names:
        assert torch.isfinite(getattr(model, name)).all(), name
    assert np.isfinite(losses).all() and losses[-6:].mean() < losses[:6].mean()
    assert model.means.shape[0] == model.grad_norm_accum.shape[0] == cap
