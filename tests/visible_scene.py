"""The scenes of tests/test_gpu_visible_step.py: visibility known by construction.

`make_scene` at 64 x 48, two views (view 0 is [I | (0, 0, 4)], view 1 looks back from the other side of the y axis), every mean pulled
into |x|, |y|, |z| <= 0.8 -- inside both frusta, so every Gaussian left alone is seen by both views.  The Gaussians of `culled_rows`
are moved behind camera 0 (z_w in [-7, -5]: z_c < 0 there, z_c in [9, 11] under view 1); every other one of them is also lifted to
y_w = 40, outside the frustum of view 1 -- culled under both views.

  "third": every third Gaussian culled -- 16-byte quads of the width-3 tensors straddle a seen and a culled row
  "block": [256, 512) culled -- a whole block of the fused kernel without a visible Gaussian
  "none":  nothing culled

tests/test_visible_adam_python_host.py holds these promises to the fp64 projection of the oracle, on the CPU."""
import numpy as np

from scenes import make_scene

W, H = 64, 48
CASES = ("third", "block", "none")
SIZES = (257, 2 * 256 + 3)


def culled_rows(case, N):
    i = np.arange(N)
    return {"third": i % 3 == 1, "block": (i >= 256) & (i < 512), "none": np.zeros(N, dtype=bool)}[case]


def scene(case, N, max_deg, seed=31):
    """(scene dict of `make_scene` with the means moved, the rows culled under view 0, those culled under both views)."""
    sc = make_scene(N, W, H, sh_degree=max_deg, n_views=2, seed=seed, scale_range=(0.05, 0.3), dist=4.0)
    rng = np.random.default_rng(seed + 1)
    means = sc["means"] * np.float32(0.4)
    behind = culled_rows(case, N)
    means[behind, 2] = -5.0 - rng.uniform(0.0, 2.0, int(behind.sum())).astype(np.float32)
    both = behind & (np.cumsum(behind) % 2 == 1)
    means[both, 1] = 40.0
    sc["means"] = means
    return sc, behind, both
