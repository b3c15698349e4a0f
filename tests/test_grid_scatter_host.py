"""CPU: `grid_scatter` without a GPU -- the adjoint oracle of tests/grid_scatter_oracle.py reproduces every committed
fixture of the reference's PyTorch model and agrees with the float64 restatement of the reference kernel's rule where
the two rules coincide; the feature is present at every layer of the interface (Python signature and errors, loader,
extension module, operator schema and dispatch keys, header, exported symbols); the C ABI validates its arguments
before anything touches a device."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch as th
from conftest import GOLDEN, ROOT

import grid_scatter_oracle as O

FIXTURES = sorted(f[len("grid_scatter_"):-4] for f in os.listdir(GOLDEN) if f.startswith("grid_scatter_") and f.endswith(".npz"))


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, "grid_scatter_" + name + ".npz"))
    t = lambda k: th.from_numpy(np.ascontiguousarray(z[k]))  # noqa: E731
    mode = {0: "bilinear", 2: "bicubic"}[int(z["in_mode"])]
    args = (t("in_input"), t("in_grid"), t("in_grad_out"), int(z["in_oh"]), int(z["in_ow"]), mode, O.PADDINGS[int(z["in_padding"])], bool(int(z["in_align"])))
    return args, (t("out_out"), t("out_grad_input"), t("out_grad_grid"))


def test_the_fixtures_cover_modes_paddings_align_corners_and_dtypes():
    assert len(FIXTURES) >= 6
    seen = [load_fixture(n)[0] for n in FIXTURES]
    assert {a[5] for a in seen} == set(O.MODES) and {a[6] for a in seen} == set(O.PADDINGS)
    assert {a[7] for a in seen} == {False, True} and {a[0].dtype for a in seen} == {th.float32, th.float64}
    for a in seen:
        assert max(a[0].shape[2:]) <= 64 and max(a[3], a[4]) <= 48
        assert O.rules_coincide(a[1], a[3], a[4], a[5], a[6], a[7])  # the model and the kernel rule say the same there


@pytest.mark.parametrize("name", FIXTURES)
def test_adjoint_oracle_reproduces_the_fixture(name):
    """the same torch, the same kernels, one thread or many: per-pixel results, bit for bit (the forward sums in pixel order)"""
    (inp, grid, gout, oh, ow, mode, pad, al), want = load_fixture(name)
    tol = 0.0 if th.get_num_threads() == 1 else (1e-5 if inp.dtype == th.float32 else 1e-13)
    out = O.scatter(inp, grid, oh, ow, mode, pad, al)
    gi, gg = O.scatter_backward(gout, inp, grid, mode, pad, al)
    assert float((out - want[0]).abs().max()) <= tol * float(want[0].abs().max())
    assert th.equal(gi, want[1]) and th.equal(gg, want[2])
    # ... and the restatement with explicit weights says the same as the double-precision adjoint
    d = [t.double() for t in (inp, grid, gout)]
    a = (O.scatter(d[0], d[1], oh, ow, mode, pad, al),) + O.scatter_backward(d[2], d[0], d[1], mode, pad, al)
    b = O.restate(d[0], d[1], oh, ow, mode, pad, al, d[2])
    for x, y in zip(a, b):
        assert float((x - y).abs().max()) <= 1e-12 * float(x.abs().max())


def test_restatement_is_the_adjoint_wherever_the_rules_coincide_and_differs_outside():
    for mode, pad, al in itertools.product(O.MODES, O.PADDINGS, (False, True)):
        for extent in (1.2, 0.9):
            inp, grid, gout = O.make_case(1, 2, 3, 40, 56, 32, 48, th.float64, "uniform", extent)
            a = (O.scatter(inp, grid, 32, 48, mode, pad, al),) + O.scatter_backward(gout, inp, grid, mode, pad, al)
            b = O.restate(inp, grid, 32, 48, mode, pad, al, gout)
            rel = max(float((x - y).abs().max()) / float(x.abs().max()) for x, y in zip(a, b))
            if O.rules_coincide(grid, 32, 48, mode, pad, al):
                assert rel <= 1e-12, (mode, pad, al, extent, rel)
            elif not (pad == "reflection" and al):
                assert rel > 1e-3, (mode, pad, al, extent, rel)  # the divergence is real: bicubic, clipped / reflected centre


def test_magnitudes_bound_the_results_and_flip_predicate_reads_the_grid_only():
    inp, grid, gout = O.make_case(3, 1, 2, 20, 30, 16, 24, th.float32, "uniform", 1.3)
    for mode, pad in itertools.product(O.MODES, O.PADDINGS):
        r = O.restate(inp.double(), grid.double(), 16, 24, mode, pad, False, gout.double())
        A = O.magnitudes(inp, grid, 16, 24, mode, pad, False, gout)
        S = O.coordinate_sensitivity(inp, grid, 16, 24, mode, pad, False, gout)
        for x, a, s in zip(r, A, S):
            assert bool((x.abs() <= a * (1 + 1e-12) + 1e-300).all()) and bool((s >= 0).all())
        assert O.flip_pixels(grid, 16, 24, pad, False).shape == grid.shape[:3]
    # consecutive float32 coordinates around a texel boundary (unnormalised x = 5): flagged exactly where the float32 and
    # the float64 evaluation of that very coordinate floor differently
    xs = [th.tensor((2 * 5 + 1) / 24 - 1, dtype=th.float32)]
    for _ in range(8):
        xs = [th.nextafter(xs[0], th.tensor(-2.0))] + xs + [th.nextafter(xs[-1], th.tensor(2.0))]
    run = th.stack([th.stack(xs), th.full((17,), 0.3)], -1)[None, None]  # [1,1,17,2]
    u32, u64 = O._unnormalize(run[..., 0], 24, False), O._unnormalize(run[..., 0].double(), 24, False)
    assert bool((u64 < 5).any()) and bool((u64 >= 5).any())
    assert th.equal(O.flip_pixels(run, 16, 24, "zeros", False), th.floor(u32).double() != th.floor(u64))


def test_python_signature_errors_and_exports():
    import drtk_amd

    E = inspect.Parameter.empty
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.grid_scatter).parameters.values()]
    assert got == [("input", E), ("grid", E), ("output_height", E), ("output_width", E), ("mode", "bilinear"),
                   ("padding_mode", "border"), ("align_corners", None)]  # drtk/grid_scatter.py:18-26
    assert "grid_scatter" in drtk_amd.__all__
    x, g = th.zeros(1, 1, 4, 4), th.zeros(1, 4, 4, 2)
    with pytest.raises(ValueError, match="only 'bilinear' and 'bicubic' modes are supported but got: 'nearest'"):
        drtk_amd.grid_scatter(x, g, 4, 4, mode="nearest")
    with pytest.raises(ValueError, match="expected padding_mode to be 'zeros', 'border', or 'reflection', but got: 'wrap'"):
        drtk_amd.grid_scatter(x, g, 4, 4, padding_mode="wrap")
    # the drop-in package keeps the reference's path surface for now (tests/test_host_logic.py pins the message)
    import drtk

    with pytest.raises(AttributeError, match="not provided"):
        drtk.grid_scatter


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    x, g = th.zeros(1, 2, 4, 4), th.zeros(1, 4, 4, 2)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        drtk_amd.grid_scatter(x, g, 4, 4)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        drtk_amd.grid_scatter(x.requires_grad_(True), g, 4, 4, "bicubic", "zeros", True)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.grid_scatter_ext.grid_scatter_2d(x, g, 4, 4, 1, 0, False)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.grid_scatter_2d(x, g, 4, 4)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.grid_scatter_2d_backward(x, x, g)


def test_loader_accepts_the_new_name_and_the_extension_module_imports():
    import importlib

    from drtk_amd.utils import load_torch_ops

    load_torch_ops("drtk.grid_scatter_ext")
    load_torch_ops("drtk_amd.grid_scatter_ext")
    with pytest.raises(ImportError):
        load_torch_ops("drtk.grid_scatter")
    import drtk.utils

    drtk.utils.load_torch_ops("drtk.grid_scatter_ext")
    module = importlib.import_module("drtk.grid_scatter_ext")  # what the reference's loader does (load_torch_ops.py:14-20)
    assert module.__file__.endswith("grid_scatter_ext.so")
    th.ops.load_library(module.__file__)
    syms = subprocess.run(["nm", "-D", "--defined-only", module.__file__], capture_output=True, text=True).stdout
    assert " T PyInit_grid_scatter_ext" in syms
    assert th._C._dispatch_has_kernel_for_dispatch_key("grid_scatter_ext::grid_scatter_2d", "CUDA")


def test_operator_schema_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    got = str(th.ops.grid_scatter_ext.grid_scatter_2d.default._schema)
    want = ("grid_scatter_ext::grid_scatter_2d(Tensor input, Tensor grid, int output_height, int output_width, int padding_mode, "
            "int interpolation_mode, bool align_corners) -> Tensor")
    assert got.replace(" ", "") == want.replace(" ", ""), got
    for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
        assert th._C._dispatch_has_kernel_for_dispatch_key("grid_scatter_ext::grid_scatter_2d", key), key


def test_header_declares_and_library_exports_the_entry_points():
    from drtk_amd import capi

    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "drtk_amd", "libdrtk_amd.so")], capture_output=True, text=True).stdout
    for name in ("drtk_amd_grid_scatter_2d", "drtk_amd_grid_scatter_2d_backward"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert re.search(r" T " + name + r"$", syms, re.M), name
        assert name in capi.EXPORTS


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    z, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def fwd(dtype=0, inp=a16, grid=a16, layout=None, N=1, C=1, H=4, W=4, oh=4, ow=4, pad=1, mode=0, out=a16):
        return L.drtk_amd_grid_scatter_2d(ci(dtype), inp, grid, layout, i64(N), i64(C), i64(H), i64(W), i64(oh), i64(ow), ci(pad), ci(mode),
                                          ci(0), out, z, z)

    def bwd(dtype=0, go=a16, inp=a16, grid=a16, N=1, C=1, H=4, W=4, oh=4, ow=4, pad=1, mode=0, gi=a16, gg=a16, glayout=None):
        return L.drtk_amd_grid_scatter_2d_backward(ci(dtype), go, inp, grid, None, i64(N), i64(C), i64(H), i64(W), i64(oh), i64(ow), ci(pad),
                                                   ci(mode), ci(0), gi, gg, glayout, z)

    for f in (fwd, bwd):
        assert f(dtype=7) == -1
        assert f(N=-1) == -1 and f(C=-1) == -1 and f(H=-1) == -1 and f(W=-1) == -1
        assert f(oh=0) == -1 and f(ow=0) == -1 and f(oh=-3) == -1  # output sizes must be positive
        assert f(H=1 << 16, W=1 << 15) == -1  # H * W < 2^31
        assert f(oh=1 << 16, ow=1 << 15) == -1
        assert f(pad=3) == -1 and f(pad=-1) == -1
        assert f(mode=1) == -1 and f(mode=3) == -1  # nearest is refused, as the reference's wrapper refuses it
        assert f(C=1 << 20) == -1
    assert fwd(out=z) == -1 and fwd(inp=z) == -1 and fwd(grid=z) == -1
    assert bwd(go=z) == -1 and bwd(grid=z) == -1 and bwd(inp=z) == -1
    assert bwd(inp=z, gg=z) in (0, -3)  # input is only read for the grid gradient (passes validation: a launch without a device fails)
    bad = (ctypes.c_int64 * 3)(32, 0, 1)
    assert fwd(layout=bad) == -1 and bwd(glayout=bad) == -1
    # nothing to do: no pointer is looked at
    assert fwd(N=0, inp=z, grid=z, out=z) == 0
    assert bwd(N=0, go=z, inp=z, grid=z, gi=z, gg=z) == 0 and bwd(H=0, go=z, inp=z, grid=z, gi=z, gg=z) == 0
    assert bwd(gi=z, gg=z, go=z, inp=z, grid=z) == 0  # neither gradient asked for
