"""drtk.utils.geometry of the drop-in (drtk/utils/geometry.py of the reference), served by drtk_amd.geometry: HIP
kernels for float32 / float64 tensors on the GPU, a PyTorch formulation otherwise."""
from drtk_amd.geometry import (  # noqa: F401
    face_attribute_to_vert,
    face_dpdt,
    face_info,
    index,
    vert_binormals,
    vert_normals,
)
