"""`composite_layers` -- front-to-back compositing of the layers of `rasterize_layers` (no counterpart in `drtk`)."""
from typing import Optional, Tuple

import torch as th
from drtk_amd.utils import load_torch_ops

# the operator library is one file; it is loaded through a name the loader serves
load_torch_ops("drtk.rasterize_ext")


@th.compiler.disable
def composite_layers(
    color: th.Tensor,
    alpha: Optional[th.Tensor] = None,
    index_img: Optional[th.Tensor] = None,
    background: Optional[th.Tensor] = None,
) -> Tuple[th.Tensor, th.Tensor]:
    """Composites K layers front to back into one image, in one kernel (and one for the backward pass).

    The definition, evaluated in the tensors' own dtype -- the forward result is this loop's, bit for bit::

        img, T = zeros(N, C, H, W), ones(N, 1, H, W)
        for k in range(K):                      # layer 0 is nearest
            a = alpha[:, k:k+1]
            img = img + (T * a) * color[:, k]
            T = T * (1 - a)
        if background is not None:
            img = img + T * background

    Args:
        color: `[N, K, C, H, W]`, float32 or float64 (half precision under autocast is cast to float32).  With
            `alpha=None` it is rgba, `[N, K, C + 1, H, W]` with alpha as the last channel -- what
            `interpolate(...).unflatten(0, (N, K))` gives when alpha is the last attribute.
        alpha: `[N, K, H, W]` or `[N, K, 1, H, W]`, or `None` (rgba).
        index_img: `[N, K, H, W]` int32 as returned by :func:`rasterize_layers`, optional.  A layer whose index is `-1`
            is skipped -- also between two present layers --, and neither its colour nor its alpha is read: NaN there does
            not propagate.  Not differentiable.
        background: `[N, C, H, W]`, optional; a view-shared background (`bg.expand(N, -1, -1, -1)`) is read in place.

    Returns:
        `(img [N, C, H, W], transmittance [N, 1, H, W])`.  HIP tensors only.

    Tensors whose `H x W` planes are contiguous (split tensors, rgba, channel slices of rgba) are read in place, anything
    else is copied once.  Gradients flow to `color`, `alpha` and `background` (zeros at skipped layers); the backward
    pass is division-free, so `alpha == 1` is exact, and the alpha gradient of an opaque layer sees the layers behind it.
    Results are bitwise reproducible from run to run.  Double backward is not supported.
    """
    return th.ops.drtk_amd_ext.composite_layers(color, alpha, index_img, background)
