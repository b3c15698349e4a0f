"""CPU: `ssim` and `photometric_loss` without a GPU -- the feature is present at every layer of the interface (Python export,
operator schemas and dispatch keys, the loud failure on CPU tensors, the argument errors, the C ABI's argument validation),
and the closed-form gradient its backward kernel evaluates is autograd of the definition (tests/image_loss_oracle.py).  Then
what the GPU tests rely on: the structural cases have the tile grids and slot counts they claim, one view left out of a
many-slot case moves each scalar by more than 100 tolerances, and the fuzzer's seeds hold what their test says."""
import ctypes
import inspect

import pytest
import torch as th

import image_loss_oracle as O


def test_python_signatures_and_export():
    import drtk_amd

    E = inspect.Parameter.empty
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.ssim).parameters.values()]
    assert got == [("img", E), ("target", E), ("weight", None), ("window_size", 11), ("sigma", 1.5), ("data_range", 1.0),
                   ("padding", "same"), ("reduction", "mean")]
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.photometric_loss).parameters.values()]
    assert got == [("img", E), ("target", E), ("weight", None), ("l1_weight", 0.8), ("ssim_weight", 0.2), ("window_size", 11),
                   ("sigma", 1.5), ("data_range", 1.0), ("padding", "same")]
    assert "ssim" in drtk_amd.__all__ and "photometric_loss" in drtk_amd.__all__
    import drtk

    assert not hasattr(drtk, "ssim") and not hasattr(drtk, "photometric_loss")  # the drop-in keeps the reference's surface


def test_operator_schemas_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    want = {
        "ssim": "drtk_amd_ext::ssim(Tensor img, Tensor target, Tensor? weight, int window_size, float sigma, float data_range, bool valid) -> Tensor",
        "ssim_map": "drtk_amd_ext::ssim_map(Tensor img, Tensor target, int window_size, float sigma, float data_range, bool valid) -> Tensor",
        "photometric_loss": "drtk_amd_ext::photometric_loss(Tensor img, Tensor target, Tensor? weight, float l1_weight, float ssim_weight, "
                            "int window_size, float sigma, float data_range, bool valid) -> Tensor",
    }
    for name, schema in want.items():
        assert str(getattr(th.ops.drtk_amd_ext, name).default._schema) == schema, name
        for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
            assert th._C._dispatch_has_kernel_for_dispatch_key("drtk_amd_ext::" + name, key), (name, key)


def test_c_abi_names_are_declared_and_bound():
    """tests/test_host_logic.py holds the header's declarations against `nm -D`; here: the three names are among them."""
    import os
    import re

    from conftest import ROOT
    from drtk_amd import capi

    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    for name in ("drtk_amd_image_loss_workspace_bytes", "drtk_amd_image_loss_forward", "drtk_amd_image_loss_backward"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    x, y = th.rand(2, 3, 16, 20), th.rand(2, 3, 16, 20)
    w = th.ones(2, 16, 20, dtype=th.bool)
    for a, b in ((x, y), (x.double(), y.double()), (x.clone().requires_grad_(True), y)):
        for kwargs in ({}, {"weight": w}, {"padding": "valid"}, {"window_size": 7, "sigma": 1.0}):
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                drtk_amd.ssim(a, b, **kwargs)
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                drtk_amd.photometric_loss(a, b, **kwargs)
        with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
            drtk_amd.ssim(a, b, reduction="none")
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.drtk_amd_ext.ssim(x, y, None, 11, 1.5, 1.0, False)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.image_loss_forward(x, y)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.image_loss_backward(x, y, None, th.zeros(3, 2, 3, 16, 20), th.ones(()), th.zeros(4, dtype=th.float64))


def test_value_errors_before_any_launch():
    import drtk_amd

    x, y = th.rand(1, 2, 12, 14), th.rand(1, 2, 12, 14)
    bad = [
        dict(window_size=4), dict(window_size=1), dict(window_size=17), dict(window_size=-3), dict(window_size=11.0),
        dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
        dict(data_range=0.0), dict(data_range=-2.0),
        dict(padding="reflect"), dict(padding="SAME"), dict(padding=None),
        dict(padding="valid", window_size=13),  # H = 12 < 13
        dict(padding="valid", window_size=15),  # W = 14 < 15
    ]
    for kwargs in bad:
        for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
            with pytest.raises(ValueError):
                fn(x, y, **kwargs)
    for kwargs in (dict(reduction="sum"), dict(reduction=None), dict(reduction="none", weight=th.ones(1, 12, 14))):
        with pytest.raises(ValueError):
            drtk_amd.ssim(x, y, **kwargs)
    # the operators judge the same numbers (a caller that goes past the wrappers)
    for args in ((4, 1.5, 1.0, False), (17, 1.5, 1.0, False), (11, 0.0, 1.0, False), (11, 1.5, 0.0, False), (13, 1.5, 1.0, True)):
        with pytest.raises(ValueError):
            th.ops.drtk_amd_ext.ssim(x, y, None, *args)
        with pytest.raises(ValueError):
            th.ops.drtk_amd_ext.ssim_map(x, y, *args)
        with pytest.raises(ValueError):
            th.ops.drtk_amd_ext.photometric_loss(x, y, None, 0.8, 0.2, *args)
    # "valid" at exactly the window's size passes the checks (and then fails as CPU tensors)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        drtk_amd.ssim(th.rand(1, 1, 11, 11), th.rand(1, 1, 11, 11), padding="valid")


def test_shape_and_dtype_errors():
    import drtk_amd

    x = th.rand(2, 3, 16, 20)
    for a, b, kwargs, message in [
        (x[0], x[0], {}, r"expected img.ndim == 4"),
        (x, x[:, :2], {}, "same sizes"),
        (x, x.double(), {}, "same dtype"),
        (x.int(), x.int(), {}, "not implemented for 'Int'"),
        (x.half(), x.half(), {}, "not implemented for 'Half'"),
        (x, x, {"weight": th.ones(2, 3, 16, 20)}, r"expected weight to be \[N, H, W\] or \[N, 1, H, W\]"),
        (x, x, {"weight": th.ones(2, 16, 20, dtype=th.float64)}, "expected weight to be bool or"),
        (th.zeros(0, 3, 16, 20), th.zeros(0, 3, 16, 20), {}, "non-empty"),
    ]:
        for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
            with pytest.raises(RuntimeError, match=message):
                fn(a, b, **kwargs)


def test_target_requiring_a_gradient_names_the_workaround():
    import drtk_amd

    x, y = th.rand(1, 1, 16, 16), th.rand(1, 1, 16, 16).requires_grad_(True)
    for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
        with pytest.raises(RuntimeError, match="arguments exchanged"):
            fn(x, y)
        with th.no_grad(), pytest.raises(RuntimeError, match=r"\(HIP\) path only"):  # without autograd it is no error
            fn(x, y)


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci, cd = ctypes.c_int64, ctypes.c_int, ctypes.c_double
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    s3, s2 = (i64 * 3)(6000, 2000, 50), (i64 * 2)(2000, 50)

    def ws(N=2, H=40, W=50, k=11, valid=0, out="out"):
        o = ctypes.c_size_t(0)
        return lib.drtk_amd_image_loss_workspace_bytes(i64(N), i64(H), i64(W), ci(k), ci(valid), ctypes.byref(o) if out == "out" else None), o.value

    assert ws() == (0, 2 * 2 * 2 * 4 * 8)  # 2 views x (2 x 2 tiles of 32 x 32) x 4 doubles
    assert ws(valid=1) == (0, 2 * 1 * 2 * 4 * 8)  # the map is 30 x 40
    assert ws(out=None)[0] == -1 and ws(k=4)[0] == -1 and ws(k=17)[0] == -1 and ws(k=1)[0] == -1 and ws(N=0)[0] == -1
    assert ws(H=10, valid=1)[0] == -1 and ws(H=11, valid=1)[0] == 0 and ws(H=1 << 16, W=1 << 15)[0] == -1

    def head(dtype=0, x=p, xs=s3, y=p, ys=s3, w=z, kind=0, wst=s2, N=2, C=3, H=40, W=50, k=11, sigma=1.5, dr=1.0, valid=0, mode=1, l1=0.8, ss=0.2):
        return (ci(dtype), x, xs, y, ys, w, ci(kind), wst, i64(N), i64(C), i64(H), i64(W), ci(k), cd(sigma), cd(dr), ci(valid), ci(mode), cd(l1), cd(ss))

    def fwd(out=p, maps=z, scalars=p, wsp=p, nbytes=1 << 20, **kw):
        return lib.drtk_amd_image_loss_forward(*head(**kw), out, maps, scalars, wsp, ctypes.c_size_t(nbytes), z)

    def bwd(maps=p, gout=p, scalars=p, gimg=p, **kw):
        return lib.drtk_amd_image_loss_backward(*head(**kw), maps, gout, scalars, gimg, z)

    for f in (fwd, bwd):  # judged before any pointer is looked at (all of them are junk here)
        assert f(dtype=2) == -1 and f(dtype=7) == -1
        assert f(mode=3) == -1 and f(mode=-1) == -1 and f(kind=3) == -1
        assert f(mode=0, kind=2, w=p) == -1  # the map takes no weight
        assert f(k=4) == -1 and f(k=1) == -1 and f(k=17) == -1
        assert f(sigma=0.0) == -1 and f(sigma=float("nan")) == -1 and f(dr=0.0) == -1 and f(dr=float("inf")) == -1
        assert f(N=0) == -1 and f(C=0) == -1 and f(H=0) == -1 and f(W=-1) == -1
        assert f(H=10, valid=1) == -1
        assert f(x=z) == -1 and f(y=z) == -1 and f(xs=None) == -1 and f(ys=None) == -1
        assert f(kind=1, w=z) == -1 and f(kind=2, w=p, wst=None) == -1
        assert f(xs=(i64 * 3)(6000, -1, 50)) == -1
    assert fwd(out=z) == -1 and fwd(scalars=z) == -1 and fwd(wsp=z) == -1
    assert fwd(nbytes=8) == -2  # workspace too small
    assert bwd(maps=z) == -1 and bwd(gout=z) == -1 and bwd(gimg=z) == -1 and bwd(scalars=z) == -1


def _grid(shape, k, padding):
    """(tiles_x, tiles_y, slots) of the forward, the slots from the library's own workspace size."""
    from conftest import ROOT
    from drtk_amd import capi

    TW, TH, sums, _ = O.tile_constants(ROOT)
    N, _, H, W = shape
    off = k // 2 if padding == "valid" else 0
    nbytes = capi.image_loss_workspace_bytes(N, H, W, k, padding == "valid")
    assert nbytes % (sums * 8) == 0
    return -(-(W - 2 * off) // TW), -(-(H - 2 * off) // TH), nbytes // (sums * 8)


def test_structural_cases_reach_the_tiles_and_slot_counts_they_are_there_for():
    """What tests/test_gpu_image_loss.py, tests/guarded_added_ops.py and image_loss_oracle.STRUCTURAL_CASES say of these
    cases, from the tile constants in csrc/image_loss.hip and drtk_amd_image_loss_workspace_bytes: a change of the tile
    size or of the finalize kernel's width fails here instead of quietly leaving a path without a test."""
    import test_gpu_image_loss as G
    from conftest import ROOT

    TW, TH, _, block = O.tile_constants(ROOT)
    S = O.STRUCTURAL_CASES
    grids = {(name, p): _grid(S[name][0], S[name][1], p) for name in S for p in S[name][2]}
    for (name, p), (tx, ty, slots) in grids.items():
        assert slots == S[name][0][0] * tx * ty, (name, p)
        for weighted in (False, True):  # and the GPU tests run them
            assert (S[name][0], S[name][1], 1.0, p, weighted) in G.PARAMS, (name, p)
    # interior tiles: one with a neighbour on either side, in x and in y, under both paddings -- in "valid" exactly one
    assert grids[("interior_tiles", "same")] == (4, 4, 16) and grids[("interior_tiles", "valid")] == (3, 3, 9)
    shape, k = S["interior_tiles"][:2]
    assert (-(-shape[3] // TW), -(-shape[2] // TH)) == (4, 4)  # the backward's tiles, over the image
    assert (shape[3] - 2 * (k // 2)) % TW != 0 and (shape[2] - 2 * (k // 2)) % TH != 0  # with ragged last tiles
    # more tiles across than down, more than one view
    assert grids[("five_by_two", "same")] == (5, 2, 20) and grids[("five_by_two", "valid")] == (5, 2, 20)
    # the finalize kernel: `block` threads, thread t takes slots t, t + block, ...
    assert grids[("slots256", "same")] == (1, 1, block)          # one pass, every thread one slot
    assert grids[("slots257", "same")] == (1, 1, block + 1)      # thread 0 takes a second
    assert grids[("slots513", "same")] == (1, 1, 2 * block + 1)  # and a third
    assert grids[("tiles_and_views", "same")] == (3, 3, 297) and grids[("tiles_and_views", "valid")] == (3, 3, 297)
    assert block < 297 < 2 * block
    assert O.SLOT_CASES == ["slots256", "slots257", "slots513", "tiles_and_views"]


SLOT_PARAMS = [(name, p) for name in O.SLOT_CASES for p in O.STRUCTURAL_CASES[name][2]]


@pytest.mark.parametrize("name,padding", SLOT_PARAMS, ids=[f"{n}-{p}" for n, p in SLOT_PARAMS])
def test_a_view_left_out_of_a_many_slot_case_moves_each_scalar_by_100_tolerances(name, padding):
    """The condition under which a dropped or mis-owned slot shows in the GPU tests: with the weight of one view zeroed --
    the last, a middle one, and the first of the finalize kernel's second pass -- `ssim` and `photometric_loss` (float64,
    the oracle) move by more than 100 x the tolerance test_float32_within_four_times_the_formulations_own_error applies to
    that scalar, plain and under the mask.  The tolerance is formed as there, from the float32 formulation's error on the map,
    here on the CPU (another summation order in conv2d than on the device; the factor 100 is not that close, the least ratio
    is 160).  In tiles_and_views a view is nine slots: there the weight of one tile of one view, the interior one, is zeroed too."""
    import test_gpu_image_loss as G
    from conftest import ROOT

    shape, k, _, _ = O.STRUCTURAL_CASES[name]
    N, _, H, W = shape
    kw = dict(window_size=k, sigma=1.5 * k / 11, data_range=1.0, padding=padding)
    x32, y32 = O.case_inputs(shape, k, dtype=th.float32)
    x, y = x32.double(), y32.double()
    map_bar = float((O.ssim(x32, y32, reduction="none", **kw).double() - O.ssim(x, y, reduction="none", **kw)).abs().max())
    tol = {"ssim": 4 * map_bar, "photo": G.SSW * 4 * map_bar + G.L1W * 4 * th.finfo(th.float32).eps}

    def scalars(w):
        return {"ssim": float(O.ssim(x, y, w, **kw)), "photo": float(O.photometric_loss(x, y, w, G.L1W, G.SSW, **kw))}

    TW, TH, _, block = O.tile_constants(ROOT)
    off = k // 2 if padding == "valid" else 0
    least = float("inf")
    for w in (th.ones(N, H, W, dtype=th.float64), O.make_mask(shape, seed=k).double()):
        full = scalars(w)
        holes = [(v, slice(None), slice(None)) for v in sorted({N - 1, N // 2, min(block, N - 1)})]
        if name == "tiles_and_views":
            holes.append((N // 2, slice(off + TH, off + 2 * TH), slice(off + TW, off + 2 * TW)))
        for v, rows, cols in holes:
            wz = w.clone()
            assert bool(wz[v, rows, cols].any())
            wz[v, rows, cols] = 0
            for q, value in scalars(wz).items():
                ratio = abs(value - full[q]) / tol[q]
                least = min(least, ratio)
                assert ratio > 100, (name, padding, v, q, value, full[q], tol[q])
    print(f"{name} {padding}: map_bar {map_bar:.3e}, least movement {least:.0f} tolerances")


def test_fuzzer_seeds_of_the_suite_hold_what_the_gpu_test_says():
    """tests/fuzz_image_ops.py, seeds 0 .. 239 (tests/test_gpu_fuzz_image_ops.py), from the drawn numbers alone: legal cases,
    every operator, weight kind, layout, padding and precision, means over more than 256 views, interior tiles."""
    import collections

    import fuzz_image_ops as F
    import test_gpu_fuzz_image_ops as G
    from conftest import ROOT

    TW, TH, _, block = O.tile_constants(ROOT)
    cases = [F.make_case(seed) for seed in range(G.BLOCKS * G.PER_BLOCK)]
    assert cases == [F.make_case(seed) for seed in range(G.BLOCKS * G.PER_BLOCK)] and len(cases) == 240  # seeded
    ops = collections.Counter(c["op"] for c in cases)
    assert set(ops) == set(F.OPS) and min(ops.values()) >= 50, ops
    losses = [c for c in cases if c["op"] != "mipmap_pyramid"]
    for c in losses:
        assert 1 <= c["N"] <= 600 and 1 <= c["C"] <= 4 and 1 <= min(c["H"], c["W"]) and max(c["H"], c["W"]) <= 140, c
        assert c["k"] % 2 == 1 and 3 <= c["k"] <= 15 and 0.5 <= c["sigma"] <= 3.0, c
        assert c["padding"] == "same" or min(c["H"], c["W"]) >= c["k"], c
        assert (c["weight"] == "none") or c["op"] != "ssim_map", c
        assert c["N"] <= 6 or (c["N"] > block and max(c["H"], c["W"]) <= 12 and c["op"] != "ssim_map"), c
    for key, values in (("weight", F.WEIGHTS), ("layout", F.LAYOUTS), ("padding", ("same", "valid")), ("dtype", ("f32", "f64")), ("data_range", (1.0, 255.0))):
        assert {c[key] for c in losses} == set(values), key
    assert {c["k"] for c in losses} == set(range(3, 16, 2))
    assert sum(c["N"] > block for c in losses) == 7
    across = lambda c, size, tile: -(-(size - (2 * (c["k"] // 2) if c["padding"] == "valid" else 0)) // tile)  # noqa: E731
    assert sum(across(c, c["W"], TW) >= 3 for c in losses) >= 60 and sum(across(c, c["H"], TH) >= 3 for c in losses) >= 60
    assert sum(c["padding"] == "valid" and across(c, c["W"], TW) >= 3 and across(c, c["H"], TH) >= 3 for c in losses) == 7
    assert sum(1 in (c["H"], c["W"]) for c in losses) >= 20
    pyramids = [c for c in cases if c["op"] == "mipmap_pyramid"]
    for c in pyramids:
        assert 1 <= c["N"] <= 3 and 1 <= c["C"] <= 5 and 1 <= min(c["H"], c["W"]) and max(c["H"], c["W"]) <= 200, c
        assert 1 <= c["levels"] <= min(11, min(c["H"], c["W"]).bit_length()) and len(c["absent"]) < c["levels"], c
    assert {c["layout"] for c in pyramids} == {"contiguous", "one_element_in"} and {c["dtype"] for c in pyramids} == {"f32", "f64"}
    assert any(0 in c["absent"] for c in pyramids) and any(c["absent"] == () for c in pyramids) and max(c["levels"] for c in pyramids) >= 7


CASES = [((2, 3, 37, 53), 11, 1.5, 1.0), ((1, 2, 20, 17), 7, 1.0, 255.0), ((1, 1, 7, 9), 11, 1.5, 1.0), ((1, 1, 15, 15), 15, 2.5, 1.0)]
# "valid" needs H, W >= window_size
GRADIENT_CASES = [(*c, padding) for c in CASES for padding in ("same", "valid") if padding == "same" or min(c[0][2:]) >= c[1]]


@pytest.mark.parametrize(
    "shape,k,sigma,data_range,padding", GRADIENT_CASES, ids=[f"{'x'.join(map(str, c[0]))}-w{c[1]}-{c[4]}" for c in GRADIENT_CASES])
def test_closed_form_gradient_is_autograd_of_the_definition(shape, k, sigma, data_range, padding):
    """float64; at most 1e-12 (of max(1, max|autograd|)) for a random upstream map, for the weighted mean and for the
    photometric loss."""
    x, y = O.make_images(shape, seed=3, data_range=data_range)
    gen = th.Generator().manual_seed(5)
    kw = dict(window_size=k, sigma=sigma, data_range=data_range, padding=padding)

    def close(a, b):
        err, top = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
        assert err <= 1e-12 * top, (err, top)

    leaf = x.clone().requires_grad_(True)
    S = O.ssim(leaf, y, reduction="none", **kw)
    h = th.rand(S.shape, generator=gen, dtype=th.float64) * 2 - 1
    (S * h).sum().backward()
    close(O.gradient(x, y, h, **kw), leaf.grad)
    for weight in (None, O.make_mask(shape, seed=1), th.rand(shape[0], 1, *shape[2:], generator=gen, dtype=th.float64)):
        leaf = x.clone().requires_grad_(True)
        O.ssim(leaf, y, weight, **kw).backward()
        close(O.gradient(x, y, O.mean_upstream(weight, x, k, padding), **kw), leaf.grad)
        leaf = x.clone().requires_grad_(True)
        O.photometric_loss(leaf, y, weight, 0.7, 0.3, **kw).backward()
        close(O.photometric_gradient(x, y, weight, 0.7, 0.3, **kw), leaf.grad)


def test_oracle_fixed_points():
    """ssim(x, x) == 1 everywhere and in the mean; the losses of a zero weight are 0 with a zero gradient, all finite."""
    x, _ = O.make_images((2, 3, 24, 31), seed=1)
    for padding in ("same", "valid"):
        S = O.ssim(x, x, padding=padding, reduction="none")
        assert float((S - 1).abs().max()) <= 1e-12
        assert abs(float(O.ssim(x, x, padding=padding)) - 1) <= 1e-12
        assert abs(float(O.photometric_loss(x, x, padding=padding))) <= 1e-12
        zero = th.zeros(2, 24, 31, dtype=th.bool)
        y = (x * 0.5).requires_grad_(True)
        s, loss = O.ssim(y, x, zero, padding=padding), O.photometric_loss(y, x, zero, padding=padding)
        assert float(s.detach()) == 0.0 and float(loss.detach()) == 0.2 * (1 - 0.0)
        (s + loss).backward()
        assert bool(th.isfinite(y.grad).all()) and not bool(y.grad.any())
