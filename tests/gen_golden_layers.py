#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/layers_<scene>.npz, the expected output of `rasterize_layers` at
K = 8 for the committed scenes, with tests/layers_oracle.py (the CPU oracle's rasterize on every triangle alone, keys
sorted per pixel).  Needs oracle/libdrtk_oracle.so (built on first use) and tests/golden/<scene>.npz only; nothing of
drtk_amd is imported.  No test imports this file; tests/test_rasterize_layers_host.py re-derives the fixtures.

    python tests/gen_golden_layers.py      # rewrites tests/golden/layers_*.npz

Per scene: `depth` [N,8,H,W] float32 and `index` [N,8,H,W] int32 (strict depth order)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layers_oracle as LO  # noqa: E402


def main():
    for name in LO.SCENES:
        v, vi, H, W = LO.scene_inputs(name)
        depth, index = LO.layers(v, vi, H, W, LO.MAX_LAYERS)
        LO.check_layer_properties(depth, index)
        path = os.path.join(LO.GOLDEN, "layers_" + name + ".npz")
        np.savez_compressed(path, depth=depth, index=index)
        per_pixel = (index >= 0).sum(1)
        print(f"{name}: {tuple(index.shape)}, most fragments on a pixel {int(per_pixel.max())}, "
              f"pixels with >= 2: {int((per_pixel >= 2).sum())}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
