#!/usr/bin/env python3
"""What `rasterization(packed=True)` and `sparse_grad=True` add to a call, at the bench scene (1 M Gaussians, 1920x1080, SH degree 3,
tight lists), with 1 camera and with 4: `tools/packed_time.py [steps] [rounds] [--n N] [--out FILE]`.

Per camera count, in ONE process, the three calls alternate -- `packed=False`, `packed=True`, `packed=True, sparse_grad=True` --
`rounds` times (default 3); each turn times `steps` forwards under no_grad and `steps` forward + backward pairs, wall clock between
synchronisations.  Reported per call: the minimum over its turns; for the unchanged `packed=False` call all `rounds` runs (the
yardstick for "nothing without the keyword": a difference inside their spread is no difference); and nnz / (C N) as the packed call saw it.

Next to it, on the dense meta and gradients of one call, the packing steps alone against the same gathers written with torch indexing
-- what the kernels of gs_packed.hip must beat: ids (`torch.nonzero(radii > 0)` vs gs_pack_flags + scan + the host read), the five
per-pair arrays (`dense[camera_ids, gaussian_ids]` x 5 vs one gs_pack_gather), a [C,N,2] gradient at the pairs (vs gs_pack_take) and a
[N,3] gradient at the seen Gaussians (`v[ids]` vs gs_pack_take), each over `reps` repetitions between synchronisations.
Prints one JSON line; `--out FILE` also writes it to FILE."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from easy_gaussian_splatting_amd import rendering as R
from easy_gaussian_splatting_amd.synthetic import config_bench_1m

args = sys.argv[1:]
opts = {"--out": None, "--n": "1000000"}
for flag in list(opts):
    if flag in args:
        i = args.index(flag)
        opts[flag] = args[i + 1]
        del args[i:i + 2]
steps = int(args[0]) if len(args) > 0 else 30
rounds = int(args[1]) if len(args) > 1 else 3
n_gauss, reps = int(opts["--n"]), 20
if not torch.cuda.is_available():
    sys.exit("tools/packed_time.py measures on the GPU: no HIP device found")
dev = torch.device("cuda:0")
CALLS = {"dense": dict(packed=False), "packed": dict(packed=True), "packed_sparse": dict(packed=True, sparse_grad=True)}


def wall_ms(fn, n):
    fn()   # (once untimed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def measure(C: int):
    sc = config_bench_1m(seed=42, n=n_gauss, n_views=C)
    T = lambda k: torch.from_numpy(sc[k]).to(dev)
    W, H, N = sc["width"], sc["height"], n_gauss
    base = [T("means"), T("quats"), T("scales"), T("opacities"), T("shs")]
    vm, Ks, bg = T("viewmats"), T("Ks"), T("backgrounds")
    vc = torch.randn((C, H, W, 3), generator=torch.Generator().manual_seed(0)).to(dev)
    kw = dict(sh_degree=3, backgrounds=bg, absgrad=True, _tile_culling="tight")
    seen = {}

    def forward(name):
        with torch.no_grad():
            _, _, meta = R.rasterization(*base, vm, Ks, W, H, **kw, **CALLS[name])
        if name == "packed":
            seen["nnz"] = int(meta["camera_ids"].numel())

    def forward_backward(name):
        ins = [t.detach().requires_grad_(True) for t in base]
        img, _, _ = R.rasterization(*ins, vm, Ks, W, H, **kw, **CALLS[name])
        torch.autograd.grad((img * vc).sum(), ins)

    runs = {name: {"fwd_ms": [], "fwd_bwd_ms": []} for name in CALLS}
    for _ in range(rounds):
        for name in CALLS:
            runs[name]["fwd_ms"].append(round(wall_ms(lambda: forward(name), steps), 4))
            runs[name]["fwd_bwd_ms"].append(round(wall_ms(lambda: forward_backward(name), steps), 4))
    out = {"cameras": C, "nnz_over_CN": round(seen["nnz"] / (C * N), 4),
           "calls": {name: {k: min(v) for k, v in r.items()} for name, r in runs.items()},
           "dense_runs": runs["dense"],
           "dense_spread": {k: round(max(v) - min(v), 4) for k, v in runs["dense"].items()}}

    # the packing steps alone, and the same gathers with torch indexing, on one dense call's meta and gradients
    with torch.no_grad():
        _, _, md = R.rasterization(*base, vm, Ks, W, H, **kw, packed=False)
    radii, per_pair = md["radii"], [md[k].contiguous() for k in ("radii", "means2d", "depths", "conics")] + [md["opacities"].contiguous()]
    v_pairs, v_rows = torch.randn((C, N, 2), device=dev), torch.randn((N, 3), device=dev)
    idx = torch.nonzero(radii > 0)
    cam, gid = idx[:, 0].contiguous(), idx[:, 1].contiguous()
    ids = torch.nonzero((radii > 0).any(dim=0))[:, 0].contiguous()
    pk = R._Pack(radii, C, N, True)
    assert pk.nnz == cam.numel() and pk.nu == ids.numel()
    op = base[3]

    def kernel_gather():
        meta = R._LazyMeta({**{k: dict.__getitem__(md, k) for k in dict.keys(md)}})
        R._pack_meta(meta, C, N, op, False)

    steps_ms = {
        "ids_torch_nonzero": wall_ms(lambda: torch.nonzero(radii > 0), reps),
        "ids_kernels_flags_scan_read": wall_ms(lambda: R._Pack(radii, C, N, False), reps),
        "five_arrays_torch_index": wall_ms(lambda: [a[cam, gid] for a in per_pair], reps),
        "ids_and_five_arrays_kernels": wall_ms(kernel_gather, reps),
        "pair_rows_torch_index": wall_ms(lambda: v_pairs[cam, gid], reps),
        "pair_rows_gs_pack_take": wall_ms(lambda: pk.take_pairs(v_pairs, 2), reps),
        "seen_ids_torch_nonzero": wall_ms(lambda: torch.nonzero((radii > 0).any(dim=0)), reps),
        "seen_rows_torch_index": wall_ms(lambda: v_rows[ids], reps),
        "seen_rows_gs_pack_take": wall_ms(lambda: pk.take_seen(v_rows, 3), reps),
    }
    out["packing_steps_ms"] = {k: round(v, 4) for k, v in steps_ms.items()}
    return out


res = {"workload": f"{n_gauss} Gaussians, 1920x1080, SH degree 3, tight lists, eager rasterization()", "steps": steps, "rounds": rounds,
       "reps": reps, "by_cameras": [measure(C) for C in (1, 4)]}
print(json.dumps(res))
if opts["--out"]:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as f:
        json.dump(res, f, indent=1)
