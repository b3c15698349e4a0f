"""drtk.utils of the drop-in: the loader, the projection with its field-of-view estimators and the mesh geometry (drtk/utils/__init__.py:8-22 of
the reference); project_points_grad is outside it."""
from drtk.utils.geometry import face_dpdt, face_info, vert_binormals, vert_normals  # noqa: F401
from drtk.utils.indexing import index  # noqa: F401
from drtk.utils.load_torch_ops import load_torch_ops  # noqa: F401
from drtk.utils.projection import (  # noqa: F401
    DISTORTION_MODES,
    estimate_fisheye62_fov,
    estimate_fisheye_fov,
    estimate_rt_fov,
    project_pinhole,
    project_points,
)

_OUT_OF_SCOPE = {"project_points_grad"}


def __getattr__(name):
    if name in _OUT_OF_SCOPE:
        raise AttributeError(f"drtk.utils.{name} is not provided by drtk_amd's drop-in (outside the rasterize -> render -> "
                             "interpolate -> edge_grad path; DESIGN.md, out of scope)")
    raise AttributeError(f"module 'drtk.utils' has no attribute '{name}'")
