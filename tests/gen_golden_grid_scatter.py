#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/grid_scatter_<case>.npz from the REFERENCE'S OWN pure-PyTorch
model of grid_scatter (drtk/grid_scatter.py: grid_scatter_ref, the autograd function around F.grid_sample), imported
from where it lies through oracle/gen_golden_refpy.import_reference() (build machine only), on the CPU.  A process of
its own: nothing of drtk_amd is imported.  Single torch thread => deterministic accumulation order.  No test imports
this file.

    python tests/gen_golden_grid_scatter.py      # rewrites tests/golden/grid_scatter_*.npz

Per case: the inputs (input, grid, grad_out, the mode / padding / align_corners / output size), the model's output and
its autograd gradients for grad_out.  The bicubic border / reflection cases keep the grid where the unnormalised
coordinate lies inside [0, size - 1]: outside, the model (grid_sample's rule) and the reference's kernel differ
(tests/grid_scatter_oracle.py), and the kernel's rule is what this package implements."""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

# name: (mode, padding, align_corners, dtype, grid kind, grid extent, (N, C, H, W), (oh, ow))
CASES = {
    "bilinear_border_f32": ("bilinear", "border", False, th.float32, "uniform", 1.2, (2, 3, 24, 40), (20, 28)),
    "bilinear_zeros_ac_f32": ("bilinear", "zeros", True, th.float32, "uniform", 1.2, (2, 4, 33, 21), (48, 17)),
    "bilinear_reflection_f64": ("bilinear", "reflection", False, th.float64, "uniform", 1.6, (1, 2, 24, 40), (20, 28)),
    "bicubic_zeros_f32": ("bicubic", "zeros", False, th.float32, "uniform", 1.2, (2, 3, 24, 40), (20, 28)),
    "bicubic_border_f32": ("bicubic", "border", False, th.float32, "warp", 0.9, (2, 1, 40, 24), (28, 20)),
    "bicubic_reflection_ac_f64": ("bicubic", "reflection", True, th.float64, "uniform", 0.95, (1, 3, 24, 40), (20, 28)),
    "bicubic_border_ac_f64": ("bicubic", "border", True, th.float64, "warp", 1.0, (1, 2, 64, 64), (48, 48)),
}


def main():
    th.set_num_threads(1)
    from gen_golden_refpy import import_reference

    drtk = import_reference()
    import grid_scatter_oracle as O  # seeded inputs only

    ref = sys.modules["drtk.grid_scatter"].grid_scatter_ref
    for seed, (name, (mode, padding, align, dtype, kind, extent, shape, (oh, ow))) in enumerate(CASES.items()):
        inp, grid, gout = O.make_case(100 + seed, *shape, oh, ow, dtype=dtype, kind=kind, extent=extent)
        if mode == "bicubic" and padding != "zeros":
            assert O.rules_coincide(grid, oh, ow, mode, padding, align), name
        x, g = inp.clone().requires_grad_(True), grid.clone().requires_grad_(True)
        out = ref(x, g, oh, ow, mode, padding, align)
        # autograd.grad, not backward(): the model's forward runs `grid_sample(ones, grid).backward(input)` under enable_grad
        # to form its output, which also ACCUMULATES into the .grad of a grid leaf -- a stray term (non-zero where taps fall
        # outside under zeros padding) that is no part of the gradient the model's backward returns
        gx, gg = th.autograd.grad(out, (x, g), gout)
        arrs = {
            "in_input": inp, "in_grid": grid, "in_grad_out": gout, "in_mode": np.int64(O.MODE_ENUM[mode]),
            "in_padding": np.int64(O.PADDING_ENUM[padding]), "in_align": np.int64(int(align)), "in_oh": np.int64(oh),
            "in_ow": np.int64(ow), "out_out": out.detach(), "out_grad_input": gx, "out_grad_grid": gg,
        }
        path = os.path.join(OUT, "grid_scatter_" + name + ".npz")
        np.savez_compressed(path, **{k: (v.detach().numpy() if isinstance(v, th.Tensor) else v) for k, v in arrs.items()})
        print(f"  {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
