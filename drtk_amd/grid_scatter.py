"""`grid_scatter` -- host-side mirror of drtk/grid_scatter.py:17-105."""
from typing import Optional

import torch as th
from drtk_amd.utils import load_torch_ops

load_torch_ops("drtk.grid_scatter_ext")


@th.compiler.disable
def grid_scatter(
    input: th.Tensor,
    grid: th.Tensor,
    output_height: int,
    output_width: int,
    mode: str = "bilinear",
    padding_mode: str = "border",
    align_corners: Optional[bool] = None,
) -> th.Tensor:
    """The splatting counterpart of `torch.nn.functional.grid_sample`: where `grid_sample` lets every output pixel READ
    from a location of the input, `grid_scatter` lets every input pixel ADD its value to the location `grid` names in an
    output of the given size -- e.g. camera-view values, visibility weights or gradients accumulated into a UV atlas,
    with the per-pixel UV image of `interpolate` as the grid.

    The forward pass is the adjoint of `grid_sample` with respect to its texture; the backward pass samples the
    incoming gradient back (`grad_input = grid_sample(grad_out, grid)`) and gives the gradient with respect to `grid`.

    Args:
        input: source values `[N, C, H, W]` (float32 / float64; half precision under autocast is cast to float32).
        grid: destinations `[N, H, W, 2]` in `grid_sample`'s normalised `[-1, 1]` convention.  A channel-first UV
            image `[N, 2, H, W]` seen through `permute(0, 2, 3, 1)` is read in place.
        output_height, output_width: size of the output.
        mode: `'bilinear'` | `'bicubic'`.
        padding_mode: `'zeros'` | `'border'` | `'reflection'`.
        align_corners: as in `grid_sample` (default False).

    Returns:
        `[N, C, output_height, output_width]`.  Contributions that meet in a texel are summed with float atomics: the
        result is equal up to rounding, not bitwise, from run to run.  HIP tensors only.
    """
    if mode != "bilinear" and mode != "bicubic":
        raise ValueError(
            "grid_scatter(): only 'bilinear' and 'bicubic' modes are supported " "but got: '{}'".format(mode)
        )
    if padding_mode != "zeros" and padding_mode != "border" and padding_mode != "reflection":
        raise ValueError(
            "grid_scatter(): expected padding_mode "
            "to be 'zeros', 'border', or 'reflection', "
            "but got: '{}'".format(padding_mode)
        )
    mode_enum = 0 if mode == "bilinear" else 2
    padding_mode_enum = {"zeros": 0, "border": 1, "reflection": 2}[padding_mode]
    if align_corners is None:
        align_corners = False
    return th.ops.grid_scatter_ext.grid_scatter_2d(
        input,
        grid,
        output_height,
        output_width,
        padding_mode_enum,
        mode_enum,
        align_corners,
    )
