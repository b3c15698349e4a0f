"""`msi` -- host-side mirror of drtk/msi.py:14-54."""
import torch as th
from drtk_amd.utils import load_torch_ops

# the operator library is one file; it is loaded through a name the loader serves (`msi_ext` is not one of them: the `drtk`
# drop-in package does not lift msi yet -- INTEGRATION.md)
load_torch_ops("drtk.rasterize_ext")


@th.compiler.disable
def msi(
    ray_o: th.Tensor,
    ray_d: th.Tensor,
    texture: th.Tensor,
    sub_step_count: int = 2,
    min_inv_r: float = 1.0,
    max_inv_r: float = 0.0,
    stop_thresh: float = 1e-7,
) -> th.Tensor:
    """Renders a multi-sphere image (MSI) in the style of "NeRF++: Analyzing and Improving Neural Radiance Fields": a stack
    of equirectangular RGB-sigma layers on concentric spheres, marched by one ray per pixel from the innermost sphere
    outwards -- the background to composite under a rendered mesh, `img = mask * mesh + (1 - mask) * msi(...)[:, :3]`.
    Sampling is bilinear within a layer and cubic between the layers.

    Args:
        ray_o: ray origins `[N, 3]`, float32.
        ray_d: ray directions `[N, 3]`, float32; they need not be normalised.
        texture: the MSI `[L, 4, H, W]`, L layers of r, g, b and sigma (the density: negative log of transmittance per unit
            of the march).  float32 (the tuned path) or float64; half precision under autocast is cast to float32.
        sub_step_count: spheres sampled per layer.
        min_inv_r: inverse radius of the innermost sphere (1: the unit sphere).
        max_inv_r: inverse radius towards which the outermost sphere goes (0: infinity).
        stop_thresh: a ray ends once its transmittance falls below this value.

    Returns:
        `[N, 4]` in the dtype of `texture`: r, g, b and the log of the remaining transmittance (-1000 for a ray that ended
        early).  HIP tensors only.

    Gradients: `texture` only -- the rays get none, and the gradient arriving for the fourth output column is ignored, both
    as in the reference.  The gradient of sigma is the reference's expression, which is NOT the derivative of the forward
    pass: with `T` the transmittance after a sample, `ref = sum_ch(max(rgb, 0) * g * exp(-sigma) * T - acc)` is what is
    scattered, while the derivative is `(ref + sum_ch(max(rgb, 0) * g * T * (1 - exp(-sigma)))) / (L * sub_step_count)`.
    It is kept for parity with what users of the reference trained against.  The texture gradient is summed with float
    atomics: equal up to rounding, not bitwise, from run to run.

    With a float64 texture the ray geometry runs in float64 too (the reference keeps it in float32).
    """
    return th.ops.msi_ext.msi(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh)
