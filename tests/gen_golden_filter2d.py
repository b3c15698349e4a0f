#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/filter2d_*.npz from the REFERENCE'S OWN pure-PyTorch model of
filter2d (drtk/filter2d_ref.py: pad, zero insertion, crop, two grouped conv2d; its numpy filter design), imported from
where it lies through oracle/gen_golden_refpy.import_reference() (build machine only), on the CPU.  A process of its own:
nothing of drtk_amd is imported.  Single torch thread => deterministic accumulation order.  No test imports this file.

    python tests/gen_golden_filter2d.py      # rewrites tests/golden/filter2d_*.npz

filter2d_weights.npz   make_resampling_kernel for n_taps 2 ... 6 x m in {1, 2, 4, 8} x freq_div in {1, 2} x
                       alias_guard_band in {0, 0.5, 1} x both filter types, at gain 1 and at gain m: `params` [R, 6] =
                       (n_taps, m, freq_div, gain, alias_guard_band, filter_type), the weights of row r in
                       `weights[offsets[r]:offsets[r + 1]]`.
filter2d_<case>.npz    per case of tests/filter2d_oracle.py CASES: the inputs, the model's float64 output for each padding
                       of the case, and for zeros padding the autograd gradient of the stored grad_out -- of the first P
                       of the case's N * C planes, as [1, P, H, W], P the most that keeps the file below 300 KiB.

The model CORRELATES with f (conv2d) where the operator -- the reference's CUDA kernel and its ATen CPU route, which flip f
first -- CONVOLVES: the two agree for the symmetric filters of make_resampling_kernel, and for the random filters of the
case table the model is handed f reversed, so that what is recorded is the operator on `in_f`.

The model imports torchvision for a Gaussian-blur helper nothing here calls; empty stand-in modules take its place.  Its
conv2d needs the filter in x's type: float64 inputs get f.double()."""
import os
import sys
import types

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")


def save(name, arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if isinstance(v, th.Tensor) else np.asarray(v)) for k, v in arrs.items()})
    size = os.path.getsize(path)
    print(f"  {path}: {size / 1024:.1f} KiB")
    assert size < 300 * 1024, path


def main():
    th.set_num_threads(1)
    from gen_golden_refpy import import_reference

    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    import_reference()
    sys.path.insert(0, "/root/reference")
    import drtk.filter2d_ref as ref  # noqa: E402

    sys.path.remove("/root/reference")
    import filter2d_oracle as O  # seeded inputs only

    params, weights, offsets = [], [], [0]
    for filter_type in (ref.FilterType.Kaiser, ref.FilterType.Lanczos):
        for n_taps in (2, 3, 4, 5, 6):
            for m in (1, 2, 4, 8):
                for freq_div in (1.0, 2.0):
                    for guard in (0.0, 0.5, 1.0):
                        for gain in sorted({1.0, float(m)}):
                            w = ref.make_resampling_kernel(ref.FilterOptions(n_taps, filter_type, guard), m, freq_div, gain)
                            assert w.dtype == th.float32 and w.shape == (n_taps * m,)
                            params.append((n_taps, m, freq_div, gain, guard, filter_type.value))
                            weights.append(w.numpy())
                            offsets.append(offsets[-1] + w.numel())
    save("filter2d_weights", {"params": np.asarray(params, dtype=np.float64), "weights": np.concatenate(weights),
                              "offsets": np.asarray(offsets, dtype=np.int64)})

    for name, (up, down, _, shape, paddings) in O.CASES.items():
        x, f, gout, up, down = O.make_case(name)
        # float64 results of random data do not compress: a file holds the first P planes of its case (the operator works
        # plane by plane), P the most that keeps it below 300 KiB
        n_in, n_out = x.shape[2] * x.shape[3], gout.shape[2] * gout.shape[3]
        per_plane = 4 * n_in + 4 * n_out + 8 * n_out * len(paddings) + (8 * n_in if "zeros" in paddings else 0)
        P = min(shape[0] * shape[1], (270 * 1024) // per_plane)
        x, gout = x.reshape(1, -1, *x.shape[2:])[:, :P], gout.reshape(1, -1, *gout.shape[2:])[:, :P]
        arrs = {"in_x": x, "in_f": f, "in_grad_out": gout, "in_up": np.int64(up), "in_down": np.int64(down)}
        for padding in paddings:
            xd = x.double().requires_grad_(True)
            out = ref.resample_filter(xd, f.double().flip(0), up, down, padding)
            arrs["out_" + padding] = out.detach()
            if padding == "zeros":
                assert out.shape == gout.shape, (name, out.shape, gout.shape)
                arrs["grad_zeros"] = th.autograd.grad(out, xd, gout.double())[0]
        save("filter2d_" + name, arrs)


if __name__ == "__main__":
    main()
