"""CPU: `rasterize_layers` without a GPU -- the committed layer fixtures re-derive from the CPU oracle and agree with
the scenes' own fixtures, the feature is present at every layer of the interface (Python signatures, operator schema
and dispatch keys, header, exported symbols), and the C ABI validates its arguments before anything touches a device.
Then the random soups of tests/fuzz_layers.py: by the oracle alone they deliver what
tests/test_gpu_rasterize_layers_soup.py relies on."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch as th
from conftest import GOLDEN, ROOT

import fuzz_layers as FL
import layers_oracle as LO


@pytest.mark.parametrize("scene", LO.SCENES)
def test_layer_fixtures_rederive_and_extend_the_scene_fixtures(scene):
    z = np.load(os.path.join(GOLDEN, "layers_" + scene + ".npz"))
    depth, index = z["depth"], z["index"]
    v, vi, H, W = LO.scene_inputs(scene)
    assert index.shape == (v.shape[0], LO.MAX_LAYERS, H, W) and index.dtype == np.int32
    assert depth.shape == index.shape and depth.dtype == np.float32
    d2, i2 = LO.layers(v, vi, H, W, LO.MAX_LAYERS)
    assert np.array_equal(i2, index)
    assert np.array_equal(d2.view(np.uint32), depth.view(np.uint32))
    # layer 0 is the scene's own fixture (the reference's rasterize of the whole mesh), index and depth bits
    s = np.load(os.path.join(GOLDEN, scene + ".npz"))
    assert np.array_equal(index[:, 0], s["out_index_img"])
    assert np.array_equal(depth[:, 0].view(np.uint32), s["out_depth_img"].view(np.uint32))
    LO.check_layer_properties(depth, index)
    # a prefix of the layers is the layers of a smaller K
    d4, i4 = LO.layers(v, vi, H, W, 4)
    assert np.array_equal(i4, index[:, :4]) and np.array_equal(d4.view(np.uint32), depth[:, :4].view(np.uint32))


def test_the_fixtures_have_something_behind_the_first_surface():
    most = {s: int((np.load(os.path.join(GOLDEN, "layers_" + s + ".npz"))["index"] >= 0).sum(1).max()) for s in LO.SCENES}
    assert most["spheres_f32"] == 4 and most["spheres_f64"] == 4, most
    assert all(m >= 2 for m in most.values()), most


def test_keys_compare_as_unsigned_64_bit_numbers():
    # a depth with the sign bit set sorts LAST (the reference's atomicMin is unsigned): the helper must not shift in int64
    depth = np.array([-1.0, 1.0, 0.5], dtype=np.float32)
    index = np.array([0, 1, 2], dtype=np.int32)
    keys = LO.pack_keys(depth, index)
    assert keys.dtype == np.uint64
    assert list(np.argsort(keys)) == [2, 1, 0]
    d, i = LO.unpack_keys(keys)
    assert np.array_equal(d.view(np.uint32), depth.view(np.uint32)) and np.array_equal(i, index)
    assert LO.pack_keys(np.zeros(1, np.float32), np.array([-1], np.int32))[0] == LO.EMPTY
    # equal depth: the lower id first
    keys = LO.pack_keys(np.array([2.0, 2.0], np.float32), np.array([7, 3], np.int32))
    assert keys[1] < keys[0]


def test_python_signatures_and_exports():
    import drtk_amd

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    want = [("v", E), ("vi", E), ("height", E), ("width", E), ("num_layers", E)]
    assert params(drtk_amd.rasterize_layers) == want
    assert params(drtk_amd.rasterize_layers_with_depth) == want
    assert "rasterize_layers" in drtk_amd.__all__ and "rasterize_layers_with_depth" in drtk_amd.__all__
    # the drop-in keeps the reference's surface
    import drtk

    assert not hasattr(drtk, "rasterize_layers")


def test_operator_schema_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    got = str(th.ops.drtk_amd_ext.rasterize_layers.default._schema)
    want = "drtk_amd_ext::rasterize_layers(Tensor v, Tensor vi, int height, int width, int num_layers) -> (Tensor, Tensor)"
    assert got.replace(" ", "") == want.replace(" ", ""), got
    for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
        assert th._C._dispatch_has_kernel_for_dispatch_key("drtk_amd_ext::rasterize_layers", key), key
    assert not hasattr(th.ops.rasterize_ext, "rasterize_layers")  # that namespace is the reference's schema verbatim


def test_header_declares_and_library_exports_the_entry_points():
    import subprocess

    from drtk_amd import capi

    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "drtk_amd", "libdrtk_amd.so")], capture_output=True, text=True).stdout
    for name in ("drtk_amd_rasterize_layers_workspace_bytes", "drtk_amd_rasterize_layers"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert re.search(r" T " + name + r"$", syms, re.M), name
        assert name in capi.EXPORTS
    m = re.search(r"#define\s+DRTK_AMD_MAX_RASTER_LAYERS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 8 == capi.MAX_RASTER_LAYERS == LO.MAX_LAYERS


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    out = ctypes.c_size_t(0)
    plain = ctypes.c_size_t(0)
    assert L.drtk_amd_rasterize_workspace_bytes(i64(8), i64(100352), i64(2048), i64(2048), ctypes.byref(plain)) == 0
    for K in (1, 4, 8):  # the bins are shared by the layers: the workspace of rasterize
        assert L.drtk_amd_rasterize_layers_workspace_bytes(i64(8), i64(100352), i64(2048), i64(2048), ci(K), ctypes.byref(out)) == 0
        assert out.value == plain.value
    for K in (0, 9, -1):
        assert L.drtk_amd_rasterize_layers_workspace_bytes(i64(1), i64(1), i64(4), i64(4), ci(K), ctypes.byref(out)) == -1
    assert L.drtk_amd_rasterize_layers_workspace_bytes(i64(1), i64(1), i64(0), i64(4), ci(2), ctypes.byref(out)) == -1
    assert L.drtk_amd_rasterize_layers_workspace_bytes(i64(-1), i64(1), i64(4), i64(4), ci(2), ctypes.byref(out)) == -1
    assert L.drtk_amd_rasterize_layers_workspace_bytes(i64(1), i64(-1), i64(4), i64(4), ci(2), ctypes.byref(out)) == -1
    assert L.drtk_amd_rasterize_layers_workspace_bytes(i64(1), i64(1), i64(4), i64(4), ci(2), None) == -1
    z, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)
    big = ctypes.c_size_t(1 << 30)

    def call(K=2, N=1, V=0, F=0, H=4, W=4, depth=a16, index=a16, ws=ctypes.c_void_p(4096), nbytes=big, dtype=0, vi_sN=0):
        return L.drtk_amd_rasterize_layers(ci(dtype), z, z, i64(N), i64(V), i64(F), i64(vi_sN), i64(H), i64(W), ci(K),
                                           depth, index, ws, nbytes, z)

    # num_layers out of range: refused before anything else is looked at (even a bad dtype or a misaligned workspace)
    for K in (0, 9, -3):
        assert call(K=K) == -1
        assert call(K=K, dtype=7, ws=ctypes.c_void_p(4100)) == -1
    assert call(N=-1) == -1 and call(V=-1) == -1 and call(F=-1) == -1 and call(H=0) == -1 and call(W=-2) == -1
    assert call(dtype=7) == -1
    assert call(V=1 << 28) == -5
    assert call(F=2, vi_sN=5) == -1  # vi's batch stride is 0 or F * 3
    # the workspace: 16-byte aligned (checked before its size), then large enough
    for off in (4, 8, 12):
        assert call(ws=ctypes.c_void_p(4096 + off)) == -1
    assert call(nbytes=ctypes.c_size_t(0)) == -2
    # null outputs / workspace with something to write
    assert call(depth=z) == -1 and call(index=z) == -1 and call(ws=z) == -1
    # triangles need vertices
    assert call(F=1, vi_sN=3) == -1
    # N = 0: nothing to write or launch
    assert call(N=0, depth=z, index=z) == 0


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    v = th.zeros(1, 3, 3)
    vi = th.zeros(1, 3, dtype=th.int32)
    with pytest.raises(RuntimeError, match="HIP"):
        drtk_amd.rasterize_layers(v, vi, 4, 4, 2)
    with pytest.raises(RuntimeError, match="HIP"):
        drtk_amd.rasterize_layers_with_depth(v, vi, 4, 4, 2)
    with pytest.raises(RuntimeError, match="HIP"):
        th.ops.drtk_amd_ext.rasterize_layers(v, vi[None], 4, 4, 2)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.rasterize_layers(v, vi, 4, 4, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the random soups (tests/fuzz_layers.py): conditions on what the generator delivers, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
def soup_stats(name):
    c, depth, index = FL.reference(name)
    return c, depth, index, FL.statistics(c, depth, index)


@pytest.mark.parametrize("name", list(FL.CASES))
def test_every_soup_has_culled_and_off_canvas_triangles_big_ones_behind_and_ordered_layers(name):
    c, depth, index, s = soup_stats(name)
    N, F, H, W = c["N"], c["F"], c["H"], c["W"]
    live = c["live"]  # the views that hold a soup: all of them, but for heavy64
    L = len(live)
    assert index.shape == (L, min(F, FL.STAT_LAYERS), H, W) and c["v"].dtype == FL.DTYPES[c["dtype"]]
    assert c["v"].shape == (N, 3 * F, 3) and c["vi"].shape == ((N, F, 3) if c["per_view"] else (F, 3))
    LO.check_layer_properties(depth, index)
    assert int((index >= F).sum()) == 0
    if L < N:
        dead = th.ones(N, dtype=th.bool)
        dead[live] = False
        assert float(c["v"][dead].abs().max()) == 0.0 and live[0] == 0 and live[-1] == N - 1
    vi = (c["vi"][live] if c["per_view"] else c["vi"][None].expand(L, -1, -1)).long()
    tri = c["v"][live][th.arange(L)[:, None, None], vi].double().numpy()  # [L, F, 3 corners, 3]
    assert c["culled_ids"].shape[1] >= 1 and c["off_ids"].shape[1] >= 1
    for n in range(0, L, max(1, L // 7)):
        for f in c["culled_ids"][n]:  # a vertex on or behind the near plane, over the middle of the canvas: drawn nowhere
            assert tri[n, f, :, 2].min() <= 0 and 0 < tri[n, f, :, 0].mean() < W - 1 and 0 < tri[n, f, :, 1].mean() < H - 1
            assert not (index[n] == f).any()
        for f in c["off_ids"][n]:  # wholly left or right of the canvas (pixel centres are at 0 .. W - 1)
            x = tri[n, f, :, 0]
            assert (x.max() <= -1.0 or x.min() >= W) and tri[n, f, :, 2].min() > 0
            assert not (index[n] == f).any()
        seen = np.unique(index[n])
        assert len(seen) > min(F, 40) // 2  # ... while most of the others are somewhere
    assert c["big_ids"].shape == (L, c["big"])
    if c["big"]:
        assert s["big_behind"] > 0  # a screen-filling triangle in some layer >= 1: something of the soup lies in front of it
        assert all(np.isin(index[n, 1:FL.K], c["big_ids"][n]).any() for n in (0, L - 1))
    if c["per_view"]:  # a different triangle order in every view
        assert N >= 2 and not th.equal(c["vi"][0], c["vi"][1]) and th.equal(c["vi"][0].sort(0).values, c["vi"][1].sort(0).values)


def test_the_cases_with_big_triangles_and_with_per_view_topology_exist():
    assert sum(1 for p in FL.CASES.values() if p.get("big", 0) > 0) >= 3
    assert sum(1 for p in FL.CASES.values() if p.get("per_view")) >= 1
    assert sum(1 for p in FL.CASES.values() if p.get("dtype") == "f64") >= 1
    assert set(FL.CASES) >= {"free", "ties", "cap32", "straddle", "cap64", "heavy_tile", "wide", "tiles64"}


@pytest.mark.parametrize("name", ["free", "heavy_tile", "wide", "heavy64"])
def test_soups_with_free_depths_have_deep_overdraw(name):
    c, depth, index, s = soup_stats(name)
    print(name, s)
    if name == "free":
        assert s["ge2"] >= 0.30
    elif name == "heavy64":  # the soup is confined to one of eight tile columns: there
        x0, _, w, _ = c["window"]
        assert ((index >= 0).sum(1)[:, :, int(x0):int(x0 + w)] > 8).mean() >= 0.30
    else:
        assert s["gt8"] >= 0.30  # more fragments than layers
    assert s["most"] >= 12
    assert s["ties"] < 0.01 * index[:, :FL.K].size  # the order is by depth here, not by id


@pytest.mark.parametrize("name", ["ties", "cap32", "cap64"])
def test_soups_with_ties_have_long_runs_of_identical_depth_bits(name):
    c, depth, index, s = soup_stats(name)
    print(name, s)
    assert s["ties"] >= 1000
    if name == "ties":
        assert s["gt8"] >= 0.30
    else:  # beyond the cap every depth is 1 / eps of the vertices' type, cast to float32: every layer is decided by id alone
        cap = np.float32(1e8) if c["dtype"] == "f32" else np.float32(np.float64(1e16))
        filled = index >= 0
        assert filled.sum() > 0 and (depth[filled].view(np.uint32) == cap.view(np.uint32)).all()
        assert s["full"] >= 0.10


def test_the_straddling_soup_has_depths_on_both_sides_of_the_cap():
    c, depth, index, s = soup_stats("straddle")
    d = depth[:, :FL.K][index[:, :FL.K] >= 0]
    capped, below = int((d == np.float32(1e8)).sum()), int((d < np.float32(1e8)).sum())
    print("straddle", s, capped, below)
    assert capped >= 1000 and below >= 1000 and capped + below == d.size
    both = ((depth[:, :FL.K] == np.float32(1e8)) & (index[:, :FL.K] >= 0)).any(1) & ((depth[:, :FL.K] < np.float32(1e8)) & (index[:, :FL.K] >= 0)).any(1)
    assert both.mean() >= 0.10  # ... within one pixel's layers


def test_the_views_of_tiles64_that_are_rasterized_alone_have_peeled_layers():
    c, depth, index, s = soup_stats("tiles64")
    print("tiles64", s)
    for n in (0, 1, c["N"] - 1):
        assert (index[n, 2] >= 0).any()
    assert s["ge3"] >= 0.30


def tiles_touched(c, n, shift):
    """per triangle of view n: how many tiles of side 1 << shift its pixel bbox (from the truncated extremes, clamped to
    the canvas) touches, 0 if the triangle is culled by z or lies off the canvas; and its first and last tile column"""
    H, W = c["H"], c["W"]
    t = c["v"][n][(c["vi"][n] if c["per_view"] else c["vi"]).long()].double().numpy()  # [F, 3 corners, 3]
    lo, hi = t[..., :2].min(1), t[..., :2].max(1)
    live = (t[..., 2].min(1) > 1e-8) & (lo[:, 0] <= W - 1) & (lo[:, 1] <= H - 1) & (hi[:, 0] > 0) & (hi[:, 1] > 0)
    x0, y0 = (np.clip(np.trunc(lo[:, k]), 0, None).astype(np.int64) >> shift for k in (0, 1))
    x1, y1 = (np.clip(np.trunc(hi[:, k]) + 1, None, m - 1).astype(np.int64) >> shift for k, m in ((0, W), (1, H)))
    return np.where(live, (x1 - x0 + 1) * (y1 - y0 + 1), 0), x0, x1


def test_the_soups_are_sized_against_the_kernel_constants_as_the_source_states_them():
    """The constants are listed, with their lines, above CASES in tests/fuzz_layers.py; here their values are read from
    the source, and the cases that target them are checked against them."""
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "rasterize.hip")).read()

    def const(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    max_small = const(r"\bkMaxSmallTiles\s*=\s*(\d+)")
    split_min = const(r"\bkSplit4Min\s*=\s*(\d+)")
    t64_min = const(r"\bt64\s*>=\s*(\d+)")
    coop_min = const(r"\bkCoopMin\s*=\s*(\d+)")
    assert (max_small, split_min, t64_min, coop_min) == (4, 384, 2048, 256)

    def t64(c):
        return c["N"] * -(-c["W"] // 64) * -(-c["H"] // 64)

    for name in FL.CASES:  # 64-pixel tiles for tiles64 and heavy64 alone -- and not for one view of them
        c = FL.reference(name)[0]
        assert (t64(c) >= t64_min) == (name in ("tiles64", "heavy64")), name
        assert t64(c) // c["N"] < t64_min
    # heavy tile: the list of the canvas's one 32-pixel tile is longer than kSplit4Min
    c = FL.reference("heavy_tile")[0]
    tiles = tiles_touched(c, 0, 5)[0]
    assert c["H"] <= 32 and c["W"] <= 32 and int((tiles == 1).sum()) > 3 * split_min and int((tiles > 1).sum()) == 0
    # heavy64: the list of the 64-pixel tile under the soup's window is longer than 4 x kSplit4Min in every view that holds
    # a soup; the canvas ends inside the tile's second row of sub-rectangles
    c = FL.reference("heavy64")[0]
    tx = int(c["window"][0]) >> 6
    assert 16 < c["H"] < 32
    for n in c["live"]:
        tiles, first, last = tiles_touched(c, n, 6)
        assert int(((tiles > 0) & (tiles <= max_small) & (first <= tx) & (tx <= last)).sum()) > 4 * split_min
    # wide: a tenth of the triangles and more touch more than kMaxSmallTiles tiles (the per-view big list), and hold far
    # more pixels than the cooperative pass asks for
    c = FL.reference("wide")[0]
    tiles = tiles_touched(c, 0, 5)[0]
    print("wide: on the big list", int((tiles > max_small).sum()), "of", c["F"])
    assert int((tiles > max_small).sum()) >= c["F"] // 10 and 32 * 32 >= coop_min
    # the screen-filling triangles touch every tile
    for name, p in FL.CASES.items():
        c = FL.reference(name)[0]
        if p.get("big", 0):
            shift = 6 if t64(c) >= t64_min else 5
            tiles = tiles_touched(c, 0, shift)[0]
            assert all(tiles[f] == -(-c["W"] >> shift) * -(-c["H"] >> shift) for f in c["big_ids"][0]), name


def test_the_stack_keeps_the_peel_culls_bound_within_64_ulps_of_the_thresholds():
    """`stack` is the case a peel cull that is wrong by some tens of ulps cannot pass (the reasoning is above CASES in
    tests/fuzz_layers.py): every depth is LEVEL to a few ulps, and for most triangles the cull's own error budget
    delta = 40 * 5.97e-8 * ext^2 / |den| + 2e-6 (rasterize.hip z_upper_bound_bits), plus its 8 ulps and 4 for the
    depths' own rounding, stays below 64 ulps of LEVEL."""
    c, depth, index, s = soup_stats("stack")
    print("stack", s)
    filled = index >= 0
    ulps = np.abs(depth[filled].view(np.uint32).astype(np.int64) - int(np.float32(FL.LEVEL).view(np.uint32)))
    assert int(ulps.max()) <= 4
    assert s["ties"] >= 1000 and s["full"] >= 0.90
    t = c["v"][0][c["vi"].long()].double().numpy()
    ext = (t[..., :2].max(1) - t[..., :2].min(1)).max(1) + 2
    e1, e2 = t[:, 1, :2] - t[:, 0, :2], t[:, 2, :2] - t[:, 0, :2]
    den = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    delta = 40 * 5.97e-8 * ext * ext / np.maximum(den, 1e-30) + 2e-6
    close = delta / 2.0 ** -23 + 8 + 4 < 64  # an ulp of LEVEL, a power of two, is 2^-23 of it
    seen = np.isin(np.arange(c["F"]), index[0, 1:FL.K])
    print("stack: triangles whose bound is within 64 ulps", int(close.sum()), "of them in a layer >= 1", int((close & seen).sum()), "of", c["F"])
    assert int((close & seen).sum()) >= c["F"] // 2
    assert int(tiles_touched(c, 0, 5)[0].max()) <= 4  # none on the big list
