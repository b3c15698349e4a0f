"""`ssim` and `photometric_loss` -- the image losses of a render-and-compare step, one fused kernel each way
(csrc/image_loss.hip; no counterpart in `drtk`)."""
from typing import Optional

import torch as th
from drtk_amd.utils import load_torch_ops

# the operator library is one file; it is loaded through a name the loader serves
load_torch_ops("drtk.mipmap_grid_sampler_ext")

MIN_WINDOW, MAX_WINDOW = 3, 15


def _valid(name: str, window_size, sigma, data_range, padding) -> bool:
    """The argument errors, before any launch; returns whether the padding is "valid"."""
    if not (isinstance(window_size, int) and not isinstance(window_size, bool)) or window_size % 2 != 1 or not MIN_WINDOW <= window_size <= MAX_WINDOW:
        raise ValueError(f"{name}(): window_size must be an odd integer in [{MIN_WINDOW}, {MAX_WINDOW}], but got {window_size!r}")
    if not float(sigma) > 0.0 or float(sigma) == float("inf"):
        raise ValueError(f"{name}(): sigma must be positive and finite, but got {sigma!r}")
    if not float(data_range) > 0.0 or float(data_range) == float("inf"):
        raise ValueError(f"{name}(): data_range must be positive and finite, but got {data_range!r}")
    if padding not in ("same", "valid"):
        raise ValueError(f"{name}(): padding must be 'same' or 'valid', but got {padding!r}")
    return padding == "valid"


def _fits(name: str, img, window_size: int, valid: bool) -> None:
    if valid and isinstance(img, th.Tensor) and img.ndim == 4 and min(img.shape[2:]) < window_size:
        raise ValueError(
            f"{name}(): padding='valid' needs H, W >= window_size ({window_size}), but got H: {img.shape[2]}, W: {img.shape[3]}")


@th.compiler.disable
def ssim(img: th.Tensor, target: th.Tensor, weight: Optional[th.Tensor] = None, window_size: int = 11, sigma: float = 1.5,
         data_range: float = 1.0, padding: str = "same", reduction: str = "mean") -> th.Tensor:
    """The structural similarity of two images under a per-pixel weight, evaluated in the tensors' dtype::

        g[i] = exp(-(i - r)^2 / (2 sigma^2)), r = window_size // 2, normalised to sum 1;  G*z: the separable blur with g
        C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2
        mu_x = G*x, mu_y = G*y, s_x = G*(x x) - mu_x^2, s_y = G*(y y) - mu_y^2, s_xy = G*(x y) - mu_x mu_y
        S = (2 mu_x mu_y + C1) (2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1) (s_x + s_y + C2))
        ssim = sum(w S) / (C sum(w))

    Args:
        img, target: `[N, C, H, W]`, float32 or float64, same dtype and shape (half precision under autocast is cast to
            float32).  HIP tensors only.  Tensors whose W stride is 1 are read in place, whatever their other strides
            (`rgba[:, :3]`, view slices); anything else is copied once.
        weight: `None`, `[N, 1, H, W]` or `[N, H, W]`, bool or the images' dtype: the foreground mask, e.g.
            `index_img != -1`.  Assumed non-negative; never validated (nothing is read back).  It gets no gradient.  A
            weight that sums to 0 makes the mean 0 and its gradient 0, not NaN.
        window_size: odd, 3 ... 15.  sigma: positive.  data_range: the value range of the images.
        padding: `"same"` blurs over zeros outside the image, so the map covers the whole image (the convention of the
            fused SSIM kernels used with splatting); `"valid"` uses only windows inside the image, so the map is the
            interior `[H - 2r, W - 2r]` and the weight is cropped to it (pytorch-msssim, skimage).  `"valid"` needs
            `H, W >= window_size`.
        reduction: `"mean"` (a 0-dim tensor) or `"none"` (the map `S`, `[N, C, H', W']`; `weight` must be `None`).

    `img` gets a gradient.  `target` requiring one is an error: the loss is symmetric, so call again with the arguments
    exchanged.  Results are bitwise reproducible and the calls are graph-capturable.  Double backward is not supported.
    Anything wrong with `window_size`, `sigma`, `data_range`, `padding` or `reduction` is a `ValueError` before any launch.
    """
    valid = _valid("ssim", window_size, sigma, data_range, padding)
    if reduction not in ("mean", "none"):
        raise ValueError(f"ssim(): reduction must be 'mean' or 'none', but got {reduction!r}")
    if reduction == "none" and weight is not None:
        raise ValueError("ssim(): reduction='none' returns the map itself and takes no weight")
    _fits("ssim", img, window_size, valid)
    if reduction == "none":
        return th.ops.drtk_amd_ext.ssim_map(img, target, window_size, float(sigma), float(data_range), valid)
    return th.ops.drtk_amd_ext.ssim(img, target, weight, window_size, float(sigma), float(data_range), valid)


@th.compiler.disable
def photometric_loss(img: th.Tensor, target: th.Tensor, weight: Optional[th.Tensor] = None, l1_weight: float = 0.8,
                     ssim_weight: float = 0.2, window_size: int = 11, sigma: float = 1.5, data_range: float = 1.0,
                     padding: str = "same") -> th.Tensor:
    """`l1_weight * l1 + ssim_weight * (1 - ssim)`: the weighted mix of L1 and D-SSIM over the foreground, one fused kernel
    for the forward pass (plus a one-workgroup reduction) and one for the backward pass.

    `ssim` is :func:`ssim` with `reduction="mean"` and the same arguments; `l1 = sum(w |img - target|) / (C sum(w))` over
    the whole image in both padding modes.  A weight that sums to 0 makes both means 0 -- the loss is then the constant
    `ssim_weight` -- and the gradient 0.  The gradient of the L1 term is `l1_weight * w * sign(img - target) / (C sum(w))`
    with `sign(0) = 0`.  Arguments, gradients, errors and limits as for :func:`ssim`.

    Example, a render against a photograph under the rasterizer's mask::

        loss = drtk_amd.photometric_loss(render[:, :3], photo, weight=(index_img != -1))
    """
    valid = _valid("photometric_loss", window_size, sigma, data_range, padding)
    _fits("photometric_loss", img, window_size, valid)
    return th.ops.drtk_amd_ext.photometric_loss(
        img, target, weight, float(l1_weight), float(ssim_weight), window_size, float(sigma), float(data_range), valid)
