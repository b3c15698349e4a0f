"""drtk_amd -- MI355X-native differentiable rasterization hot path
(rasterize -> render -> interpolate -> edge_grad), drop-in for the `drtk.*` functions of
facebookresearch/DRTK on PyTorch-ROCm, plus the mesh geometry of `drtk.utils` (vertex normals,
face info, UV Jacobians, binormals), `grid_scatter`, the `msi` background, the `filter2d` resampling filters and layered rendering (`rasterize_layers`, `composite_layers`).  Kernels: hand-written HIP for gfx950 in
`drtk_amd/csrc`, C ABI in `include/drtk_amd.h`."""
from drtk_amd.composite import composite_layers  # noqa: F401
from drtk_amd.edge_grad_estimator import edge_grad_estimator  # noqa: F401
from drtk_amd.filter2d import (  # noqa: F401
    FilterOptions,
    FilterType,
    downsample,
    filter,
    low_pass_filter,
    make_resampling_kernel,
    resample_filter,
    upsample,
)
from drtk_amd.geometry import (  # noqa: F401
    cotangent_weights,
    face_attribute_to_vert,
    face_dpdt,
    face_info,
    mesh_laplacian,
    vert_binormals,
    vert_normals,
)
from drtk_amd.graph import capture_step  # noqa: F401
from drtk_amd.grid_scatter import grid_scatter  # noqa: F401
from drtk_amd.image_loss import photometric_loss, ssim  # noqa: F401
from drtk_amd.interpolate import (  # noqa: F401
    interpolate,
    interpolate_masked,
    interpolation_matrix,
    interpolation_normal_matrix,
)
from drtk_amd.kinematics import forward_kinematics  # noqa: F401
from drtk_amd.mipmap_grid_sample import mipmap_grid_sample  # noqa: F401
from drtk_amd.mipmap_pyramid import mipmap_pyramid  # noqa: F401
from drtk_amd.msi import msi  # noqa: F401
from drtk_amd.nearest import chamfer_distance, nearest_points  # noqa: F401
from drtk_amd.rasterize import (  # noqa: F401
    get_depth_order,
    rasterize,
    rasterize_layers,
    rasterize_layers_with_depth,
    rasterize_with_depth,
    set_depth_order,
)
from drtk_amd.render import render  # noqa: F401
from drtk_amd.screen_space_uv_derivative import screen_space_uv_derivative  # noqa: F401
from drtk_amd.shade import shade  # noqa: F401
from drtk_amd.skin import skin, sparse_skin_weights  # noqa: F401
from drtk_amd.transform import transform, transform_with_v_cam  # noqa: F401

__version__ = "0.1.0"

# The public surface.  Same names, arguments and defaults as `drtk.*` for everything on the hot path and its "next"
# rows; `interpolate_masked` (interpolate with the background written as 0), `capture_step` (a whole step as a
# HIP graph) and `set_depth_order` / `get_depth_order` (the rasterizer's depth order: the reference's source, or the
# reference as its setup.py builds it) and `rasterize_layers` / `rasterize_layers_with_depth` (the K nearest triangles per
# pixel) with `composite_layers` (their front-to-back compositing over a background, one kernel each way) are this package's
# additions, and so are `mipmap_pyramid` (the mip chain `mipmap_grid_sample` reads, one fused pass each way) and the image
# losses `ssim` / `photometric_loss` (L1 and D-SSIM under the foreground mask, one fused pass each way).  The mesh geometry of drtk.utils (face_info,
# vert_normals, face_attribute_to_vert, face_dpdt, vert_binormals) is exported here too, and so is `grid_scatter` (the
# splatting counterpart of grid_sample), `msi` (the multi-sphere-image background) and the eight names of `filter2d` (fused
# alias-free up/down-sampling and low-pass filtering); the `drtk` drop-in package does not lift these three yet --
# INTEGRATION.md.  `cotangent_weights` and `mesh_laplacian` (the mesh regulariser of a geometry fit: cotangent or uniform
# Laplacian through the cached vertex incidence, one launch each way) are this package's additions too, and stay out of the
# drop-in (the reference has no such names).  `shade` (the per-pixel Blinn-Phong shading of a render-and-compare step --
# Lambert, ambient, highlight, background select and gamma in one fused pass each way, the parameter gradients summed in a
# fixed order) is an addition of the same kind and stays out of the drop-in as well.  `skin` (linear blend skinning, the
# step from rig parameters to geometry: forward and the gradients to the rest pose, the weights and the joint transforms,
# no float atomics) with its companion `sparse_skin_weights` is one more, and stays out of the drop-in too.
# `forward_kinematics` (the step before it: axis-angle or matrix pose along a joint tree to the skinning matrices `skin`
# reads and the posed joints, one launch each way, the exponential map smooth at 0) is one more, and stays out of the
# drop-in as well.  `nearest_points` / `chamfer_distance` (closest-point queries between point sets by a brute-force tiled
# kernel, bit-defined, with the gradients to both sets in a fixed order: the data term of registration to a scan) are the
# latest, and stay out of the drop-in too.  `transform` / `transform_with_v_cam` serve the pinhole camera and, on the HIP device, the reference's
# distortion models (radial-tangential, fisheye, fisheye62 with its lookup table, per-view lists) in one fused kernel each
# way; the field-of-view estimators live in drtk_amd.transform (`estimate_rt_fov`, `estimate_fisheye_fov`,
# `estimate_fisheye62_fov`) and in the drop-in's drtk.utils.  Not provided: the pure-PyTorch `*_ref` models (out of scope).
__all__ = [
    "rasterize",
    "rasterize_with_depth",
    "rasterize_layers",
    "rasterize_layers_with_depth",
    "composite_layers",
    "render",
    "interpolate",
    "interpolate_masked",
    "edge_grad_estimator",
    "interpolation_matrix",
    "interpolation_normal_matrix",
    "mipmap_grid_sample",
    "mipmap_pyramid",
    "ssim",
    "photometric_loss",
    "shade",
    "grid_scatter",
    "msi",
    "FilterType",
    "FilterOptions",
    "resample_filter",
    "filter",
    "low_pass_filter",
    "downsample",
    "upsample",
    "make_resampling_kernel",
    "screen_space_uv_derivative",
    "transform",
    "transform_with_v_cam",
    "capture_step",
    "set_depth_order",
    "get_depth_order",
    "face_info",
    "vert_normals",
    "face_attribute_to_vert",
    "face_dpdt",
    "vert_binormals",
    "cotangent_weights",
    "mesh_laplacian",
    "skin",
    "sparse_skin_weights",
    "forward_kinematics",
    "nearest_points",
    "chamfer_distance",
]
