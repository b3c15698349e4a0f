"""`mipmap_pyramid` -- the mip chain `mipmap_grid_sample` reads, from one texture (no counterpart in `drtk`)."""
from typing import List, Optional

import torch as th
from drtk_amd.utils import load_torch_ops

# the operator library is one file; it is loaded through a name the loader serves
load_torch_ops("drtk.mipmap_grid_sampler_ext")

MAX_LEVELS = 11  # what mipmap_grid_sample takes


def max_levels(height: int, width: int) -> int:
    """`min(11, 1 + floor(log2(min(height, width))))`: halve until the smaller side is 1, at most the sampler's 11."""
    return min(MAX_LEVELS, int(min(height, width)).bit_length())


@th.compiler.disable
def mipmap_pyramid(input: th.Tensor, levels: Optional[int] = None) -> List[th.Tensor]:
    """The mip pyramid of a texture, finest level first, ready for :func:`mipmap_grid_sample` -- one fused kernel for up
    to seven levels (a second, tiny launch beyond), and one kernel for the whole backward pass.

    The definition, evaluated in the tensor's own dtype, every level from the previous level as stored -- the result is
    the chain of `avg_pool2d(x, 2)` calls, bit for bit::

        def next_level(x):                       # floor sizes: a trailing odd row / column is dropped
            h, w = x.shape[-2] // 2, x.shape[-1] // 2
            a, b = x[..., 0:2*h:2, 0:2*w:2], x[..., 0:2*h:2, 1:2*w:2]
            c, d = x[..., 1:2*h:2, 0:2*w:2], x[..., 1:2*h:2, 1:2*w:2]
            return (((a + b) + c) + d) * 0.25

    Args:
        input: `[N, C, H, W]`, float32 or float64 (half precision under autocast is cast to float32).  HIP tensors only.
        levels: how many levels to return, `input` included; `None` means all of them,
            `min(11, 1 + floor(log2(min(H, W))))`.  Anything outside `[1, that maximum]` raises `ValueError`.

    Returns:
        `levels` tensors `[N, C, H >> l, W >> l]`.  Element 0 shares `input`'s memory (it is not a copy); the others are
        views into one allocation, back to back at multiples of 16 bytes.  `levels=1` returns `[input]`.

    An input whose `H x W` planes are contiguous (any view and channel stride: channel slices) is read in place, anything
    else is copied once.  One texture shared by all views (`tex.expand(N, -1, -1, -1)`) is reduced once and the levels come
    back expanded the same way.  The gradient of every level flows to `input` through
    `G_l = g_l + 0.25 * up(G_{l+1})`, which is autograd of the `avg_pool2d` chain bit for bit; levels that received no
    gradient are not read.  Results are bitwise reproducible.  Double backward is not supported.
    """
    if isinstance(input, th.Tensor) and input.ndim == 4 and min(input.shape[2:]) >= 1:
        most = max_levels(input.shape[2], input.shape[3])
        if levels is None:
            levels = most
        elif not 1 <= int(levels) <= most:
            raise ValueError(
                f"mipmap_pyramid(): levels must be in [1, {most}] for a {input.shape[2]} x {input.shape[3]} texture, but got {levels}")
        if input.shape[0] > 1 and input.stride(0) == 0:  # one texture for all views: autograd's expand sums the gradients
            N = input.shape[0]
            return [t.expand(N, -1, -1, -1) for t in th.ops.drtk_amd_ext.mipmap_pyramid(input[:1], int(levels))]
    elif levels is None:
        levels = 1  # the operator says what is wrong with the input
    return th.ops.drtk_amd_ext.mipmap_pyramid(input, int(levels))
