"""drtk.utils.projection of the drop-in: `project_points` (drtk/utils/projection.py:33-53, 486-646) -- what
`drtk.transform` is made of -- and the field-of-view estimators.  The distortion models (radial-tangential, fisheye,
fisheye62 + lookup table) run on the HIP device (drtk_amd/transform.py); on CPU tensors only the pinhole camera is
provided and a distortion mode raises NotImplementedError.  The per-model `project_*_distort*` functions are not provided."""
from typing import List, Optional, Tuple, Union

import torch as th

from drtk_amd.transform import (  # noqa: F401
    DISTORTION_MODES,
    estimate_fisheye62_fov,
    estimate_fisheye_fov,
    estimate_rt_fov,
    project_pinhole,
    transform_with_v_cam,
)


def project_points(
    v: th.Tensor,
    campos: th.Tensor,
    camrot: th.Tensor,
    focal: th.Tensor,
    princpt: th.Tensor,
    distortion_mode: Optional[Union[List[str], str]] = None,
    distortion_coeff: Optional[th.Tensor] = None,
    fov: Optional[th.Tensor] = None,
    lut_vector_field: Optional[th.Tensor] = None,
    lut_spacing: Optional[th.Tensor] = None,
) -> Tuple[th.Tensor, th.Tensor]:
    """`(v_pix, v_cam)`, both `[N,V,3]`; `v_cam = camrot @ (v - campos)`, `v_pix = (x_pix, y_pix, z_cam)`.
    `distortion_mode`, `distortion_coeff`, `fov`, `lut_vector_field`, `lut_spacing` as in the reference (HIP tensors)."""
    return transform_with_v_cam(v, campos, camrot, focal, princpt, None, None, distortion_mode, distortion_coeff, fov,
                                lut_vector_field, lut_spacing)
