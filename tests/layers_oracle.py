"""TEST INFRASTRUCTURE ONLY -- the oracle of `rasterize_layers`, built from the CPU oracle's `rasterize` with no new
rasterizer: every triangle is rasterized ALONE (`vi[..., f:f+1, :]`), which yields its coverage and float32 depth
under the reference's arithmetic; a pixel's fragments get the key `(depth bits << 32) | id` as an UNSIGNED 64-bit
number (rasterize_kernel.cu:153-160: the reference's atomicMin compares unsigned, so a depth with the sign bit set
sorts last); the keys are sorted per pixel and layer k is the k-th of them.  Imports nothing of drtk_amd."""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = ("spheres_f32", "spheres_f64", "ragged_f32", "edge_cases_f32", "two_triangles_f32", "tutorial3_f32")
MAX_LAYERS = 8
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _oracle():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import oracle

    return oracle


def scene_inputs(name):
    """(v [N,V,3], vi [F,3] or [N,F,3] as the scene's rasterize call takes it, H, W) of tests/golden/<name>.npz"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    vi = d["in_vi_raster"] if "in_vi_raster" in d.files else d["in_vi"]
    return th.from_numpy(d["in_v"]), th.from_numpy(vi), int(d["in_H"]), int(d["in_W"])


def pack_keys(depth, index):
    """[...] float32 depth, int32 index -> uint64 keys, EMPTY where index < 0.  All arithmetic in uint64."""
    depth = np.ascontiguousarray(np.asarray(depth, dtype=np.float32))
    index = np.asarray(index, dtype=np.int32)
    bits = depth.view(np.uint32).astype(np.uint64)
    keys = (bits << np.uint64(32)) | index.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return np.where(index < 0, EMPTY, keys)


def unpack_keys(keys):
    """uint64 keys -> (float32 depth, int32 index): 0.0 / -1 where EMPTY"""
    keys = np.asarray(keys, dtype=np.uint64)
    empty = keys == EMPTY
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return np.where(empty, np.float32(0), depth), np.where(empty, np.int32(-1), index)


def layers(v, vi, height, width, num_layers):
    """(depth [N,K,H,W] float32, index [N,K,H,W] int32) numpy arrays"""
    oracle = _oracle()
    N = v.shape[0]
    F = vi.shape[-2]
    frag = np.full((max(F, 1), N, height, width), EMPTY, dtype=np.uint64)
    for f in range(F):
        one = vi[..., f:f + 1, :].contiguous()
        depth, index = oracle.rasterize(v, one, height, width)
        index = index.numpy()
        assert ((index == 0) | (index == -1)).all()
        frag[f] = pack_keys(depth.numpy(), np.where(index == 0, np.int32(f), np.int32(-1)))
    frag.sort(axis=0)  # unsigned: EMPTY last
    out = np.full((num_layers, N, height, width), EMPTY, dtype=np.uint64)
    k = min(num_layers, frag.shape[0])
    out[:k] = frag[:k]
    depth, index = unpack_keys(out.transpose(1, 0, 2, 3))
    return np.ascontiguousarray(depth), np.ascontiguousarray(index)


def check_layer_properties(depth, index):
    """keys increase strictly with k, empties trail, empty layers hold (0.0, -1)"""
    keys = pack_keys(depth, index)
    a, b = keys[:, :-1], keys[:, 1:]
    assert ((a < b) | (b == EMPTY)).all(), "keys do not increase strictly"
    assert (~(a == EMPTY) | (b == EMPTY)).all(), "an empty layer is followed by a filled one"
    assert (np.asarray(depth)[np.asarray(index) < 0] == 0).all()
    assert (np.asarray(index) >= -1).all()
