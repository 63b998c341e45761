"""General cameras for the tests: `make_scene`'s cloud seen through what a COLMAP capture holds and the orbit of
`synthetic.look_at_circle` does not -- rotations with roll (no symmetric R), translations with all three components, fx != fy, a
principal point off the image centre, one K per camera, and cameras that may stand inside the cloud (Gaussians behind the camera
and splats covering the whole image).  Plain module: no fixture, no product code.

`CONFIGS`: four named configurations, each a `centre_box` and the four projection keywords of `rasterization()`.  Measured with
the fp64 C oracle alone at n=3000, 160x112, C=2, seeds 1-3: razor-pixel fraction 0.0013-0.0026 per camera, 17-82 % visible, up to
30 % behind the near plane, 3-16 % beyond far=3.0, radii up to 8729 px, longest tile list 127-381 (tests/test_oracle.py pins
this for the seed the GPU tests use)."""
import numpy as np

from scenes import make_scene

CONFIGS = {
    "inside": dict(centre_box=1.5, near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3),
    "inside_slab": dict(centre_box=1.5, near_plane=0.2, far_plane=3.0, radius_clip=0.0, eps2d=0.3),
    "outside": dict(centre_box=3.5, near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3),
    "clip": dict(centre_box=3.0, near_plane=0.01, far_plane=1e10, radius_clip=3.0, eps2d=0.1),
}
PROJ_KEYS = ("near_plane", "far_plane", "radius_clip", "eps2d")
SEED = 2   # the seed of the GPU tests (tests/test_oracle.py checks what it promises, the razor fraction included)


def general_cameras(C, W, H, seed, centre_box):
    """(viewmats [C,4,4], Ks [C,3,3]) float32.  Per camera, in this order from default_rng(seed + 500): centre, target, up
    vector, then fx, cx, fy, cy."""
    rng = np.random.default_rng(seed + 500)
    f = W / (2.0 * np.tan(np.radians(30.0)))   # make_scene's focal length
    viewmats, Ks = [], []
    for _ in range(C):
        centre = rng.uniform(-1, 1, 3) * centre_box
        target = rng.uniform(-0.5, 0.5, 3)
        up = np.array([0.0, 1.0, 0.0]) + rng.normal(0, 0.4, 3)   # roll
        z = target - centre
        z /= np.linalg.norm(z)
        x = np.cross(up, z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        V = np.eye(4)
        V[:3, :3] = R
        V[:3, 3] = -R @ centre
        viewmats.append(V)
        fx, cx = f * rng.uniform(0.8, 1.2), W * rng.uniform(0.3, 0.7)   # (drawn in K's row-major order)
        fy, cy = f * rng.uniform(0.8, 1.3), H * rng.uniform(0.3, 0.7)
        Ks.append(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]))
    f32 = lambda a: np.ascontiguousarray(np.stack(a), dtype=np.float32)
    return f32(viewmats), f32(Ks)


def general_scene(n, W, H, C, seed, centre_box, sh_degree=3, **make_scene_kw):
    sc = make_scene(n, W, H, sh_degree=sh_degree, n_views=C, seed=seed, scale_range=(0.02, 0.2), dist=4.0, **make_scene_kw)
    sc["viewmats"], sc["Ks"] = general_cameras(C, W, H, seed, centre_box)
    return sc


def config_scene(name, n=3000, W=160, H=112, C=2, seed=SEED, sh_degree=3, **make_scene_kw):
    """(scene, the four projection keywords) of a named configuration."""
    cfg = CONFIGS[name]
    sc = general_scene(n, W, H, C, seed, cfg["centre_box"], sh_degree=sh_degree, **make_scene_kw)
    return sc, {k: cfg[k] for k in PROJ_KEYS}
