"""`shade` -- Blinn-Phong deferred shading of an interpolated G-buffer in one kernel each way (no counterpart in `drtk`)."""
import math
from typing import Optional

import torch as th
from drtk_amd.utils import load_torch_ops

# the operator library is one file; it is loaded through a name the loader serves
load_torch_ops("drtk.rasterize_ext")


def _check_param(name: str, t: th.Tensor, count, N: int) -> None:
    ok = (t.ndim == 1 and t.shape[0] == count) or (t.ndim == 2 and t.shape[0] == N and t.shape[1] == count)
    if not ok:
        raise ValueError(f"shade(): expected {name} to be [{count}] or [N, {count}] = [{N}, {count}], but got {tuple(t.shape)}")


def _check_image(name: str, t: th.Tensor, shape) -> None:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"shade(): expected {name} to be [N, {shape[1]}, H, W] = {list(shape)}, but got {tuple(t.shape)}")


@th.compiler.disable
def shade(
    normal_img: th.Tensor,
    light_dir: th.Tensor,
    albedo: th.Tensor,
    ambient: th.Tensor,
    index_img: Optional[th.Tensor] = None,
    pos_img: Optional[th.Tensor] = None,
    specular: Optional[th.Tensor] = None,
    shininess: Optional[th.Tensor] = None,
    background: Optional[th.Tensor] = None,
    gamma: Optional[float] = None,
) -> th.Tensor:
    """Shades the pixels of an interpolated G-buffer -- Lambert plus ambient, an optional Blinn-Phong highlight, the
    background where nothing was rasterised, an optional gamma curve -- in one kernel (and one for the backward pass).

    The definition, per pixel, evaluated in the tensors' own dtype, with `unit(x) = x / max(||x||, 1e-12)` (the rule of
    `F.normalize`)::

        L = unit(light_dir)                         # camera space, as the normals are
        n = unit(normal_img[:, :, y, x])
        d = max(-(n . L), 0)
        col[c] = albedo[c] * (d + ambient[c])
        if specular is not None:                    # then pos_img and shininess are required
            w = unit(pos_img[:, :, y, x])           # camera at the origin: direction camera -> surface point
            h = unit(L - w)
            b = max(-(h . n), 1e-8)
            col[c] += (b ** shininess) * specular[c]
        out[c] = col[c] if index_img is None or index_img[n, y, x] != -1 else (background[c] if background is not None else 0)
        if gamma is not None:  out[c] = max(out[c], 0) ** (1 / gamma)     # background pixels included

    With `shininess = gloss * 40` and `gamma = 2.2` this is the shading of the reference's hand-fitting tutorial.  The
    choice between foreground and background is a select, not a blend.

    Args:
        normal_img: `[N, 3, H, W]`, float32 or float64 (half precision under autocast is cast to float32); normally a channel
            slice of one `interpolate` output, such as `attr[:, 0:3]`.
        light_dir: `[3]` or `[N, 3]`, the direction the light travels, in the space of the normals.
        albedo: `[C]`, `[N, C]`, or an image `[N, C, H, W]` (a sampled texture).
        ambient: `[C]` or `[N, C]`; `C` (1 to 4) is taken from it.
        index_img: `[N, H, W]` int32 as returned by :func:`rasterize`, optional.  Where it is `-1` none of `normal_img`,
            `pos_img` and an image `albedo` is read: NaN there reaches neither the output nor a gradient.  Not differentiable.
        pos_img: `[N, 3, H, W]`, camera-space positions (`attr[:, 3:6]`); read only with `specular`.
        specular: `[C]` or `[N, C]`, optional; needs `pos_img` and `shininess`.
        shininess: `[1]` or `[N, 1]`.
        background: `[N, C, H, W]`, optional; a view-shared background (`bg.expand(N, -1, -1, -1)`) is read in place.  It is
            not read at foreground pixels.
        gamma: a positive finite float, optional.

    Returns:
        `[N, C, H, W]`.  HIP tensors only.

    Images whose W stride is 1 are read in place, whatever their other strides (channel slices, view slices, crops);
    anything else is copied once.  Gradients flow to every floating-point tensor argument that requires one; a parameter
    shaped `[K]` receives the sum over the views.  They are the derivative of the definition, with these conventions at its
    non-smooth points: `d` passes a gradient only where `-(n . L) > 0`, `b` only where `-(h . n) > 1e-8`, the gamma step only
    where its argument is `> 0` -- elsewhere the gradient is exactly 0, never NaN or inf, which differs from PyTorch's
    `pow(clamp(x, 0), 1 / gamma)` on purpose -- and `unit(x)` of a vector whose norm is `<= 1e-12` is a constant (0 for the
    zero vector) with zero gradient.  The foreground images get 0 at background pixels, `background` gets 0 at foreground
    pixels.  Nothing but the inputs is kept for the backward pass, which recomputes the shading; the parameter gradients are
    summed in double in a fixed order, so results are bitwise reproducible from run to run.  Double backward is not
    supported.
    """
    if ambient.ndim not in (1, 2):
        raise ValueError(f"shade(): expected ambient to be [C] or [N, C], but got {tuple(ambient.shape)}")
    C = ambient.shape[-1]
    if not 1 <= C <= 4:
        raise ValueError(f"shade(): the number of channels must be in [1, 4], but ambient has shape {tuple(ambient.shape)}")
    if normal_img.ndim != 4 or normal_img.shape[1] != 3:
        raise ValueError(f"shade(): expected normal_img to be [N, 3, H, W], but got {tuple(normal_img.shape)}")
    N, _, H, W = normal_img.shape
    if specular is not None and (pos_img is None or shininess is None):
        raise ValueError("shade(): specular needs pos_img and shininess")
    _check_param("ambient", ambient, C, N)
    _check_param("light_dir", light_dir, 3, N)
    if albedo.ndim == 4:
        _check_image("albedo", albedo, (N, C, H, W))
    else:
        _check_param("albedo", albedo, C, N)
    if specular is not None:
        _check_param("specular", specular, C, N)
    if shininess is not None:
        _check_param("shininess", shininess, 1, N)
    if pos_img is not None:
        _check_image("pos_img", pos_img, (N, 3, H, W))
    if background is not None:
        _check_image("background", background, (N, C, H, W))
    if index_img is not None:
        if index_img.dtype != th.int32:
            raise ValueError(f"shade(): expected index_img to have int32 type, but index_img has {index_img.dtype}")
        if tuple(index_img.shape) != (N, H, W):
            raise ValueError(f"shade(): expected index_img to be [N, H, W] = {[N, H, W]}, but got {tuple(index_img.shape)}")
    if gamma is not None:
        gamma = float(gamma)
        if not (gamma > 0.0 and math.isfinite(gamma)):
            raise ValueError(f"shade(): gamma must be positive and finite, but got {gamma}")
    return th.ops.drtk_amd_ext.shade(
        normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma)
