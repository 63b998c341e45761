"""References for the mesh tests (tests/test_tsdf_host.py, tests/test_gpu_mesh.py), none of them the code under test:

  * `integrate64`: the TSDF integration of one view in float64 numpy, with the set of *razor* voxels -- those whose branch a float32
    rounding may turn -- decided by the float64 run alone;
  * `extract64`: marching tetrahedra over the Kuhn split as plain loops in float64; the orientation of every triangle is decided
    geometrically (its normal against the direction from the inside corners to the outside ones), not from a table;
  * `host_lib`: tests/hostmath/tsdf.cpp -- csrc/gs_tsdf.h, the device's own text -- built with the host compiler;
  * mesh checks (edge counts, Euler characteristic) and the data of the cases both files share.
"""
import ctypes as ct
import itertools
import os
import subprocess
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24   # the unit roundoff of float32


# ---- the host build ----

def host_lib(directory):
    so = os.path.join(str(directory), "libtsdf_host.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostmath", "tsdf.cpp")], check=True)
    L = ct.CDLL(so)
    P, F, I = ct.c_void_p, ct.c_float, ct.c_int
    L.ts_grid_ok.argtypes, L.ts_grid_ok.restype = [P, F], I
    L.ts_integrate.argtypes, L.ts_integrate.restype = [P, P, F, F, F, F, F, P, P, I, I, P, I, I, I, P, P, P, P], None
    L.ts_extract.argtypes, L.ts_extract.restype = [P, P, F, F, P, P, P, P, P, P, P, P, P], None
    return L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def host_integrate(L, dims, origin, h, trunc, view, tsdf, weight, color, *, depth_channel, color_channel, depth_max, min_alpha,
                   max_weight):
    """One view into (copies of) tsdf [n], weight [n], color [n, 3] or None -> the new arrays.  view: dict(viewmat, K, image, alphas)."""
    d, o = np.asarray(dims, np.int32), _f32(origin)
    tsdf, weight = _f32(tsdf).copy(), _f32(weight).copy()
    color = None if color is None else _f32(color).copy()
    vm, K, img = _f32(view["viewmat"]), _f32(view["K"]), _f32(view["image"])
    al = None if view.get("alphas") is None else _f32(view["alphas"])
    H, W, S = img.shape
    L.ts_integrate(d.ctypes.data, o.ctypes.data, h, trunc, depth_max, min_alpha, max_weight, vm.ctypes.data, K.ctypes.data, W, H,
                   img.ctypes.data, S, depth_channel % S, color_channel, None if al is None else al.ctypes.data, tsdf.ctypes.data,
                   weight.ctypes.data, None if color is None else color.ctypes.data)
    return tsdf, weight, color


def host_extract(L, dims, origin, h, min_weight, tsdf, weight, color):
    """-> dict(vertices f32 [V,3], colors f32 [V,3] or None, faces i32 [F,3], owner i64 [V], kind i32 [V]) of the host build"""
    d, o = np.asarray(dims, np.int32), _f32(origin)
    tsdf, weight = _f32(tsdf).ravel(), _f32(weight).ravel()
    color = None if color is None else _f32(color).reshape(-1, 3)
    cp = None if color is None else color.ctypes.data
    totals = np.zeros(2, np.int64)
    L.ts_extract(d.ctypes.data, o.ctypes.data, h, min_weight, tsdf.ctypes.data, weight.ctypes.data, cp, totals.ctypes.data, None, None,
                 None, None, None)
    nv, nf = int(totals[0]), int(totals[1])
    v, c, f = np.full((nv + 1, 3), -7.0, np.float32), np.full((nv + 1, 3), -7.0, np.float32), np.full((nf + 1, 3), -7, np.int32)
    owner, kind = np.zeros(nv + 1, np.int64), np.zeros(nv + 1, np.int32)   # (a canary row behind each)
    L.ts_extract(d.ctypes.data, o.ctypes.data, h, min_weight, tsdf.ctypes.data, weight.ctypes.data, cp, totals.ctypes.data, v.ctypes.data,
                 c.ctypes.data, f.ctypes.data, owner.ctypes.data, kind.ctypes.data)
    assert (v[-1] == -7).all() and (c[-1] == -7).all() and (f[-1] == -7).all()
    return dict(vertices=v[:-1], colors=None if color is None else c[:-1], faces=f[:-1], owner=owner[:-1], kind=kind[:-1])


# ---- the integration in float64 ----

def grid_points64(dims, origin, h):
    """[n, 3] float64 sample positions in linear-index order (x fastest), from the float32 origin and voxel size"""
    nx, ny, nz = dims
    o = np.asarray(_f32(origin), np.float64)
    h = float(np.float32(h))
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + ix.ravel() * h, o[1] + iy.ravel() * h, o[2] + iz.ravel() * h], 1)


def integrate64(pts, view, trunc, tsdf, weight, color, *, depth_channel, color_channel, depth_max, min_alpha, max_weight):
    """One view into the float64 arrays tsdf [n], weight [n], color [n,3] or None, IN PLACE.  -> (razor bool [n], the largest
    camera-space coordinate magnitude).  A voxel is razor when u or v lies within 1e-3 px of an integer (the image border is one),
    |sdf + trunc| < 1e-4 trunc, |z| < 1e-5, or d is within 1e-5 of depth_max."""
    vm, K = np.asarray(_f32(view["viewmat"]), np.float64), np.asarray(_f32(view["K"]), np.float64)
    img = np.asarray(_f32(view["image"]), np.float64)
    al = None if view.get("alphas") is None else np.asarray(_f32(view["alphas"]), np.float64)
    H, W, _ = img.shape
    trunc, min_alpha = float(np.float32(trunc)), float(np.float32(min_alpha))
    pc = pts @ vm[:3, :3].T + vm[:3, 3]
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    razor = np.abs(z) < 1e-5
    live = z > 0
    zs = np.where(live, z, 1.0)
    u, v = K[0, 0] * (x / zs) + K[0, 2], K[1, 1] * (y / zs) + K[1, 2]
    razor |= live & ((np.abs(u - np.rint(u)) < 1e-3) | (np.abs(v - np.rint(v)) < 1e-3))
    pu, pv = np.floor(u), np.floor(v)
    live &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    pi, pj = np.where(live, pu, 0).astype(np.int64), np.where(live, pv, 0).astype(np.int64)
    d = img[pj, pi, depth_channel]
    with np.errstate(invalid="ignore"):
        razor |= live & np.isfinite(d) & (np.abs(d - depth_max) < 1e-5)
        live &= np.isfinite(d) & (d > 0) & (d <= depth_max)
        if al is not None:
            live &= al[pj, pi] >= min_alpha
        sdf = np.where(live, d - z, 0.0)
    razor |= live & (np.abs(sdf + trunc) < 1e-4 * trunc)
    live &= ~(sdf < -trunc)
    s = np.minimum(1.0, sdf / trunc)
    w = weight.copy()
    w1 = w + 1.0
    tsdf[live] = ((tsdf * w + s) / w1)[live]
    if color is not None:
        c = img[pj, pi][:, color_channel:color_channel + 3]
        color[live] = ((color * w[:, None] + c) / w1[:, None])[live]
    weight[live] = np.minimum(w1, max_weight)[live]
    return razor, float(np.abs(pc).max())


# ---- marching tetrahedra in float64, plain loops ----

# the six tetrahedra of the Kuhn split: the axis orders xyz, xzy, yxz, yzx, zxy, zyx, each the chain 0 -> +a -> +a+b -> 7
TETS = []
for perm in itertools.permutations(range(3)):
    m, chain = 0, [0]
    for axis in perm:
        m |= 1 << axis
        chain.append(m)
    TETS.append(tuple(chain))
assert TETS == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def _unit(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64)


def extract64(dims, origin, h, min_weight, tsdf, weight, color=None):
    """-> dict(keys: the sorted list of (owner, kind); vertices f64 [V,3]; colors f64 [V,3] or None; faces: list of index triples in
    the order (cell, tetrahedron, triangle), oriented so that (v1 - v0) x (v2 - v0) points from inside to outside)."""
    nx, ny, nz = dims
    f = np.asarray(_f32(tsdf), np.float64).reshape(nz, ny, nx)
    wt = np.asarray(_f32(weight), np.float64).reshape(nz, ny, nx)
    col = None if color is None else np.asarray(_f32(color), np.float64).reshape(nz, ny, nx, 3)
    o64, h64 = np.asarray(_f32(origin), np.float64), float(np.float32(h))
    lin = lambda x, y, z: x + nx * (y + ny * z)
    keys, tris = set(), []   # tris: ((owner, kind) x 3)
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                at = lambda c: (x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1))
                val = lambda c: f[at(c)[2], at(c)[1], at(c)[0]]
                if not all(wt[at(c)[2], at(c)[1], at(c)[0]] >= min_weight for c in range(8)):
                    continue
                for tet in TETS:
                    ins = [c for c in tet if val(c) < 0]
                    out = [c for c in tet if not val(c) < 0]
                    if not ins or not out:
                        continue

                    def edge(p, q):   # the vertex on the edge between corners p and q: its key and its cell-local position
                        lo, hi = (p, q) if p < q else (q, p)
                        assert lo & hi == lo
                        t = val(lo) / (val(lo) - val(hi))
                        return (lin(*at(lo)), hi ^ lo), _unit(lo) + t * (_unit(hi) - _unit(lo))

                    if len(ins) == 1:
                        cand = [[edge(ins[0], c) for c in out]]
                    elif len(out) == 1:
                        cand = [[edge(c, out[0]) for c in ins]]
                    else:
                        (a, b), (c, d) = ins, out
                        ac, ad, bd, bc = edge(a, c), edge(a, d), edge(b, d), edge(b, c)
                        cand = [[ac, ad, bd], [ac, bd, bc]]
                    towards = np.mean([_unit(c) for c in out], 0) - np.mean([_unit(c) for c in ins], 0)
                    for t3 in cand:
                        (k0, p0), (k1, p1), (k2, p2) = t3
                        if np.dot(np.cross(p1 - p0, p2 - p0), towards) < 0:
                            k1, k2 = k2, k1
                        keys.update((k0, k1, k2))
                        tris.append((k0, k1, k2))
    keys = sorted(keys)
    index = {k: i for i, k in enumerate(keys)}
    verts, cols = np.zeros((len(keys), 3)), (None if col is None else np.zeros((len(keys), 3)))
    for i, (o, kind) in enumerate(keys):
        x, y, z = o % nx, (o // nx) % ny, o // (nx * ny)
        x1, y1, z1 = x + (kind & 1), y + ((kind >> 1) & 1), z + ((kind >> 2) & 1)
        f0, f1 = f[z, y, x], f[z1, y1, x1]
        t = f0 / (f0 - f1)
        verts[i] = o64 + (np.array([x, y, z]) + t * _unit(kind)) * h64
        if col is not None:
            cols[i] = col[z, y, x] + t * (col[z1, y1, x1] - col[z, y, x])
    return dict(keys=keys, vertices=verts, colors=cols, faces=[tuple(index[k] for k in t) for t in tris])


# ---- mesh checks ----

def rotate_min_first(faces):
    """every triple rotated (orientation kept) so that its smallest index comes first"""
    out = []
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        m = min(a, b, c)
        out.append((a, b, c) if a == m else ((b, c, a) if b == m else (c, a, b)))
    return out


def directed_edges(faces):
    cnt = Counter()
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        cnt.update([(a, b), (b, c), (c, a)])
    return cnt


def undirected_edges(faces):
    cnt = Counter()
    for (a, b), k in directed_edges(faces).items():
        cnt[(min(a, b), max(a, b))] += k
    return cnt


def euler(n_vertices, faces):
    return n_vertices - len(undirected_edges(faces)) + len(np.asarray(faces).reshape(-1, 3))


def assert_closed_oriented(faces):
    """every undirected edge lies in exactly two faces, once in each direction"""
    d = directed_edges(faces)
    assert all(k == 1 for k in d.values()), "a directed edge appears twice"
    assert all((b, a) in d for (a, b) in d), "an edge without its opposite: the surface is open"


# ---- data ----

GRID_A = dict(dims=(24, 20, 17), origin=(-0.6, -0.5, -0.42), h=0.05, trunc=0.2)
PARAMS_A = dict(depth_channel=3, color_channel=0, depth_max=2.0, min_alpha=0.5, max_weight=3.0)
W_A, H_A = 37, 29


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world -> camera [4,4] float32, +z forward, +x right, +y down (the rasterizer's convention)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, -R @ eye
    return m.astype(np.float32)


def views_a(seed):
    """Four views of GRID_A, 37 x 29 x [r g b depth] with an alpha image: three cameras around the volume and one INSIDE it (some
    voxels have z <= 0).  The depth has holes of 0, negatives, NaN and inf, and values beyond depth_max; alpha straddles min_alpha."""
    rng = np.random.default_rng(seed)
    K = np.array([[30.0, 0, 18.5], [0, 31.0, 14.5], [0, 0, 1]], np.float32)
    eyes = [(1.5, 0.3, 0.4), (-0.4, -1.5, 0.5), (0.3, 0.9, -1.2), (0.11, 0.04, -0.07)]
    targets = [(0, 0, 0), (0.05, 0, -0.05), (-0.05, 0.02, 0), (-0.5, 0.3, 0.1)]
    views = []
    for eye, tgt in zip(eyes, targets):
        img = np.empty((H_A, W_A, 4), np.float32)
        img[..., :3] = rng.uniform(0, 1, (H_A, W_A, 3))
        near = 0.1 if eye == eyes[-1] else 0.8
        depth = rng.uniform(near, 2.2, (H_A, W_A)).astype(np.float32)
        hole = rng.integers(0, 25, (H_A, W_A))
        depth[hole == 0] = 0.0
        depth[hole == 1] = -1.0
        depth[hole == 2] = np.nan
        depth[hole == 3] = np.inf
        img[..., 3] = depth
        alphas = rng.choice(np.array([0.2, 0.49, 0.5, 0.51, 0.9, 1.0], np.float32), (H_A, W_A), p=[0.05, 0.05, 0.1, 0.1, 0.2, 0.5])
        views.append(dict(viewmat=look_at(eye, tgt), K=K, image=img, alphas=alphas.astype(np.float32)))
    return views


def blind_view_a(seed):
    """a view that sees nothing of GRID_A: the camera looks away from it"""
    v = views_a(seed)[0]
    return dict(v, viewmat=look_at((1.5, 0.3, 0.4), (3.0, 0.6, 0.8)))


def fresh(dims, color=True):
    n = int(np.prod(dims))
    return np.ones(n, np.float32), np.zeros(n, np.float32), (np.zeros((n, 3), np.float32) if color else None)


def smooth_case(seed, dims=(9, 8, 7), h=0.1, origin=(0.3, -0.2, 1.1), unobserved=0.15):
    """dims, origin, h, tsdf, weight, color: a sum of a few sines, a random share of the corners unobserved (weight 0)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([ix, iy, iz], -1).astype(np.float64)
    f = np.zeros((nz, ny, nx))
    for _ in range(4):
        k, ph, amp = rng.uniform(0.4, 1.3, 3), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1.0)
        f += amp * np.sin(p @ k + ph)
    weight = (rng.uniform(0, 1, f.shape) >= unobserved).astype(np.float32) * rng.integers(1, 4, f.shape).astype(np.float32)
    color = rng.uniform(0, 1, f.shape + (3,)).astype(np.float32)
    return dict(dims=dims, origin=origin, h=h, tsdf=(f / 3).astype(np.float32).ravel(), weight=weight.ravel(), color=color.reshape(-1, 3))


def field_case(fn, dims=(16, 16, 16), h=1.0 / 15.0, origin=(0.0, 0.0, 0.0), observed=None):
    """the float32 samples of fn(points float64 [n,3]) on a grid; weight 1 (or `observed(points)` as 0/1)"""
    pts = grid_points64(dims, origin, h)
    w = np.ones(len(pts), np.float32) if observed is None else observed(pts).astype(np.float32)
    return dict(dims=dims, origin=origin, h=h, tsdf=fn(pts).astype(np.float32), weight=w, color=None)


SPHERE_C, SPHERE_R = np.array([0.513, 0.487, 0.521]), 0.3


def sphere(c=SPHERE_C, r=SPHERE_R):
    return lambda p: np.linalg.norm(p - np.asarray(c), axis=1) - r
