"""Float64 reference of the blend-weight scores and the small scenes their tests share.

Definitions.  Camera c, Gaussian n, pixel p.  The blend TAKES the pair when the pixel is live, sigma >= 0,
alpha = min(0.999, opacity * exp(-sigma)) >= 1/255 and T' = T - alpha * T > 1e-4; a pair that would push T to 1e-4 or below is not
blended and finishes the pixel.  A taken pair has w = alpha * T.  Gaussians are met in depth order, and only inside the tile
rectangle gsplat lists them for ([mean2d - radius, mean2d + radius] in tiles of 16 pixels, clipped to the image)."""
import math

import numpy as np

ALPHA_MIN, ALPHA_MAX, T_MIN, TILE = 1.0 / 255.0, 0.999, 1e-4, 16


def pixel_weights(means2d, conics, opacities, depths, radii, width, height):
    """One camera: means2d [N,2], conics [N,3] (a, b, c of sigma = (a dx^2 + c dy^2) / 2 + b dx dy), opacities [N] (what the blend
    sees), depths [N], radii [N] (<= 0: culled).  Returns (w [H,W,N] float64, T_final [H,W] float64)."""
    means2d, conics, opacities, depths = (np.asarray(a, dtype=np.float64) for a in (means2d, conics, opacities, depths))
    radii = np.asarray(radii)
    N = means2d.shape[0]
    w = np.zeros((height, width, N), dtype=np.float64)
    T = np.ones((height, width), dtype=np.float64)
    live = np.ones((height, width), dtype=bool)
    px = np.arange(width, dtype=np.float64)[None, :] + 0.5
    py = np.arange(height, dtype=np.float64)[:, None] + 0.5
    tw, th = math.ceil(width / TILE), math.ceil(height / TILE)
    tile_x = (np.arange(width) // TILE)[None, :]
    tile_y = (np.arange(height) // TILE)[:, None]
    order = [n for n in np.argsort(depths, kind="stable") if radii[n] > 0]
    for n in order:
        r = float(radii[n])
        x0 = min(max(int(math.floor((means2d[n, 0] - r) / TILE)), 0), tw)
        x1 = min(max(int(math.ceil((means2d[n, 0] + r) / TILE)), 0), tw)
        y0 = min(max(int(math.floor((means2d[n, 1] - r) / TILE)), 0), th)
        y1 = min(max(int(math.ceil((means2d[n, 1] + r) / TILE)), 0), th)
        listed = (tile_x >= x0) & (tile_x < x1) & (tile_y >= y0) & (tile_y < y1)
        dx, dy = means2d[n, 0] - px, means2d[n, 1] - py
        sigma = 0.5 * (conics[n, 0] * dx * dx + conics[n, 2] * dy * dy) + conics[n, 1] * dx * dy
        alpha = np.minimum(ALPHA_MAX, opacities[n] * np.exp(-sigma))
        ok = live & listed & (sigma >= 0.0) & (alpha >= ALPHA_MIN)
        Tn = T - alpha * T
        stop = ok & (Tn <= T_MIN)
        take = ok & ~stop
        w[:, :, n] = np.where(take, alpha * T, 0.0)
        T = np.where(take, Tn, T)
        live &= ~stop
    return w, T


def scores_from_weights(w):
    """(weight_sum f64 [N], weight_max f64 [N], hits i64 [N]) of a [H,W,N] weight array."""
    return w.sum(axis=(0, 1)), w.max(axis=(0, 1), initial=0.0), (w > 0).sum(axis=(0, 1)).astype(np.int64)


# ---- the scenes of tests/test_gpu_blend_weights.py: 40 x 28 pixels (ragged tiles, ragged quadrants), two different cameras
W, H = 40, 28


def two_cameras(dist=6.0, angle_deg=25.0):
    """World -> camera: view 0 looks down +z from (0, 0, -dist); view 1 is turned about the y axis.  Ks: 60 degrees horizontal."""
    out = []
    for ang in (0.0, math.radians(angle_deg)):
        c, s = math.cos(ang), math.sin(ang)
        V = np.eye(4)
        V[:3, :3] = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        V[2, 3] = dist
        out.append(V)
    f = W / (2.0 * math.tan(math.radians(30.0)))
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]])
    return np.stack(out).astype(np.float32), np.tile(K[None], (2, 1, 1)).astype(np.float32)


def _scene(means, scales, quats, opac):
    viewmats, Ks = two_cameras()
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(means=f32(means), quats=f32(quats), scales=f32(scales), opacities=f32(opac), viewmats=viewmats, Ks=Ks, width=W, height=H)


def stack_scene(n, seed, opacity=(0.02, 0.2)):
    """Every Gaussian covers the whole image in both cameras (a footprint of 17+ pixels standard deviation around the image centre)."""
    rng = np.random.default_rng(seed)
    means = (rng.random((n, 3)) * 2 - 1) * np.array([0.2, 0.2, 0.4])
    scales = rng.uniform(3.0, 6.0, (n, 3))
    return _scene(means, scales, rng.standard_normal((n, 4)), rng.uniform(opacity[0], opacity[1], n))


def sparse_scene(seed, n=64):
    """Gaussians 1-3 pixels wide.  Returns (scene, dead): `dead` [n] marks those that can contribute to no camera -- behind both
    cameras, off screen, or with opacity 0.003 (projected, never taken: 0.003 < 1/255)."""
    rng = np.random.default_rng(seed)
    means = (rng.random((n, 3)) * 2 - 1) * np.array([2.6, 1.8, 0.5])
    scales = rng.uniform(0.03, 0.17, (n, 3))
    opac = rng.uniform(0.3, 0.9, n)
    kind = np.arange(n) % 8
    means[kind == 1] = np.array([0.0, 0.0, -8.0]) + rng.uniform(-0.3, 0.3, (int((kind == 1).sum()), 3))   # behind both cameras
    means[kind == 3, 0] = 60.0                                                                            # off screen
    opac[kind == 5] = 0.003
    return _scene(means, scales, rng.standard_normal((n, 4)), opac), (kind == 1) | (kind == 3) | (kind == 5)
