#!/usr/bin/env python3
"""Writes tests/golden/laplacian_tutorial.npz: what the reference's hand-fitting tutorial computes as its Laplacian
regulariser, on a small mesh, as data.

Run on a machine that has the reference checkout:

    python tests/gen_golden_laplacian.py [--reference /path/to/DRTK]

The tutorial's `laplacian(v, vi)` (docs/source/tutorials/DRTK_Tutorial_hand_fitting.ipynb, the cell under "Laplacian") is
read from the notebook and run here; nothing of its text is stored.  It returns a padded neighbour table and float32
weights; the fixture holds the mesh, a field x, the tutorial's application of the table to x --
(w[:, :, None] * x[idx]).sum(1) -- carried in float64, and acc = sum_j |W_ij| |x_j| per element, the magnitude the
float32 weight storage scales with.

Mesh: a jittered 6 x 6 grid (50 faces), plus a duplicate-corner face and a collinear face on three more vertices with
integer coordinates, so that c = 0 exactly in this package's formulation and the area is exactly 0 in the tutorial's
(Heron's formula on the sorted edge lengths): 39 vertices, 52 faces."""
import argparse
import json
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def tutorial_laplacian(reference):
    path = os.path.join(reference, "docs", "source", "tutorials", "DRTK_Tutorial_hand_fitting.ipynb")
    with open(path) as f:
        cells = json.load(f)["cells"]
    src = ["".join(c["source"]) for c in cells if c["cell_type"] == "code"]
    (cell,) = [s for s in src if s.lstrip().startswith("def laplacian(")]
    scope = {"np": np, "th": th}
    exec(compile(cell, path, "exec"), scope)
    return scope["laplacian"]


def main():
    import laplacian_oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    laplacian = tutorial_laplacian(a.reference)
    v, vi = O.grid_mesh(6, 6, seed=2024)
    V = v.shape[0]
    v = th.cat([v, th.tensor([[10.0, 0.0, 0.0], [12.0, 0.0, 0.0], [13.0, 0.0, 0.0]], dtype=th.float64)])
    vi = th.cat([vi, th.tensor([[7, 7, 8], [V, V + 1, V + 2]])])
    assert v.shape == (39, 3) and vi.shape == (52, 3)
    x = th.from_numpy(np.random.default_rng(7).uniform(-1, 1, (39, 3)))
    idx, w = laplacian(v.numpy(), vi.numpy())
    assert w.dtype == th.float32 and idx.shape == w.shape and idx.shape[0] == 39
    lx = (w.double()[:, :, None] * x[idx]).sum(1)
    acc = (w.double().abs()[:, :, None] * x[idx].abs()).sum(1)
    assert bool((acc[36:] == 0).all()) and bool((acc[:36] > 0).all())
    out = os.path.join(HERE, "golden", "laplacian_tutorial.npz")
    np.savez_compressed(out, v=v.numpy(), vi=vi.numpy(), x=x.numpy(), lx=lx.numpy(), acc=acc.numpy())
    print(f"wrote {out}: {os.path.getsize(out)} bytes, max valence {idx.shape[1]}")


if __name__ == "__main__":
    main()
