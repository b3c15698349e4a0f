"""CPU: `rasterize_layers` without a GPU -- the committed layer fixtures re-derive from the CPU oracle and agree with
the scenes' own fixtures, the feature is present at every layer of the interface (Python signatures, operator schema
and dispatch keys, header, exported symbols), and the C ABI validates its arguments before anything touches a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch as th
from conftest import GOLDEN, ROOT

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
