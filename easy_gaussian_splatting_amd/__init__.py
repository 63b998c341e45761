"""MI355X-native Gaussian-splat rasterizer: the hot path behind
`gsplat.rendering.rasterization()` as called by li199603/easy_gaussian_splatting
(`model/gaussian.py:353-367`), written as hand-made gfx950 HIP kernels behind a C ABI.

Public surface (mirrors the reference's names for this path):
  rendering.rasterization   -- gsplat-signature drop-in (forward + autograd backward)
  model.GaussianModel       -- the reference's `forward(data)` / `update_statistics` harness
  loss.LossComputer         -- L1 + (1 - SSIM) as the reference's train step uses
  distributed               -- one-view-per-GPU gradient all-reduce over RCCL
  evaluate.Evaluator        -- the reference's held-out evaluation (eval.py): PSNR / SSIM from one fused kernel per view
  viewer.FrameRenderer      -- the viewer's render_func (launch_viewer.py) and the camera-path video export, finished on the device
  mcmc.MCMCStrategy         -- training to a Gaussian budget: MCMC relocate / grow / noise on the flat Adam buffers
  exposure.ExposureTable    -- per-view exposure compensation: a learnable 3x4 colour affine per training image
  bilagrid.BilateralGrids   -- per-view appearance correction: a learnable bilateral grid of colour affines per training image
  depth_loss.depth_loss     -- depth supervision: the expected depth of the render against a target depth map, in depth or disparity
  mesh.extract_mesh         -- a triangle mesh of a trained model: TSDF fusion of rendered depth and marching tetrahedra on the device
  normals.normal_consistency_loss -- regularising geometry for meshing: blended Gaussian normals against the normals of the rendered depth
"""
from .bilagrid import BilagridAdamState, BilateralGrids  # noqa: F401
from .depth_loss import DepthSupervision  # noqa: F401  (depth_loss.depth_loss keeps its module path: the names collide)
from .evaluate import Evaluator, evaluate_output, image_metrics  # noqa: F401
from .mcmc import MCMCStrategy, counter_normals, opacity_weights, relocation_values, sample_by_weight, weight_cdf  # noqa: F401
from .mesh import TSDFVolume, extract_mesh, fuse_model, load_mesh_ply, save_mesh_ply  # noqa: F401
from .normals import depth_to_normal, gaussian_normals, normal_consistency_loss, render_normals  # noqa: F401
from .rendering import rasterization  # noqa: F401
from .viewer import FrameRenderer, camera_interpolation, export_video, finish_frame, viewer_render_func  # noqa: F401

__all__ = ["rasterization", "Evaluator", "image_metrics", "evaluate_output", "FrameRenderer", "finish_frame", "camera_interpolation",
           "export_video", "viewer_render_func", "MCMCStrategy", "opacity_weights", "weight_cdf", "sample_by_weight", "relocation_values", "counter_normals",
           "BilateralGrids", "BilagridAdamState", "DepthSupervision", "TSDFVolume", "fuse_model", "extract_mesh", "save_mesh_ply", "load_mesh_ply",
           "gaussian_normals", "render_normals", "normal_consistency_loss", "depth_to_normal"]
__version__ = "0.1.0"
