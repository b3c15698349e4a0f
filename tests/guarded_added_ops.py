"""The operators added after the core pipeline -- filter2d, composite_layers, grid_scatter, msi, transform_distort, the four
geometry entry points, rasterize_layers, the image losses (ssim, photometric_loss), mipmap_pyramid -- through the ctypes
binding of the C ABI with every output and workspace between sentinel elements (DRTK_CAPI_GUARD, drtk_amd/capi.py `_out`): a
fixed list of small cases, each the smallest that still ends in a ragged tail at the end of a tensor, each compared with its
oracle under the bounds of that operator's GPU tests (the guard also leaves every output merely element-aligned: those
paths must be right, not only in bounds), and after each
`capi.check_guards()`.  Not collected by pytest; tests/test_gpu_parity.py starts it in a child process:

    DRTK_CAPI_GUARD=1 DRTK_CAPI_POISON=1 python tests/guarded_added_ops.py [--only NAME]
    python tests/guarded_added_ops.py --list                (no GPU needed)

The first case shows that a damaged guard is reported.  The image losses run their structural cases (interior tiles; 256,
257, 297 and 513 partial sums in the slot workspace, whose size drtk_amd_image_loss_workspace_bytes gave), both precisions
and paddings, plain and weighted, forward with the gradient maps and backward; mipmap_pyramid the ragged shapes of its test
module at full depth, every level and grad_input element-aligned at once, with all gradients and with one absent; then the
first 20 seeds of tests/fuzz_image_ops.py, the first 20 of tests/fuzz_added_ops.py (filter2d, composite_layers, shade,
mesh_laplacian and msi on random shapes, layouts and options) and the first 20 of tests/fuzz_geometry.py (the geometry entry
points on random meshes, UV topologies of their own and partial chunks; the fixed geometry cases are the four fixture
meshes, `seam` with its own UV topology among them).  Oracles, bounds and helpers are those of the operators' own test
modules, which this script imports.  Left out: what the torch operators allocate in C++ (only the binding has guards) and
grad_grid of grid_scatter (allocated with the grid's strides, outside `_out`)."""
import argparse
import os
import sys

import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
F32, F64, F16 = th.float32, th.float64, th.float16
TAG = {F32: "f32", F64: "f64", F16: "f16"}


# ---- the guard itself ------------------------------------------------------------------------------------------------------
def guard_reports_a_write_outside():
    """One element written just past the end and just before the beginning of an allocation of `_out` -- by a torch op on a
    strided view of the same allocation, so nothing leaves it -- makes check_guards raise; an untouched one passes."""
    from drtk_amd import capi

    capi.check_guards()
    for dtype, value in ((F32, 1.0), (F64, 1.0), (th.int32, 1), (th.uint8, 1)):
        for where in ("past the end", "before the beginning", None):
            t = capi._out(3, 5, dtype=dtype, device=DEV)
            if where is not None:
                offset = t.storage_offset() + t.numel() if where == "past the end" else t.storage_offset() - 1
                assert offset >= 0
                t.as_strided((1,), (1,), offset).fill_(value)
            try:
                checked = capi.check_guards()
            except AssertionError:
                assert where is not None, f"{dtype}: an untouched allocation was reported"
                continue
            assert where is None, f"{dtype}: a write {where} of an allocation was not reported"
            assert checked == 1, checked


# ---- filter2d ----------------------------------------------------------------------------------------------------------------
def filter2d_triples():
    import filter2d_oracle as O

    smallest = {}
    for up, down, k in O.FAMILIES:
        smallest[(up, down)] = min(k, smallest.get((up, down), k))
    return [(up, down, k) for (up, down), k in sorted(smallest.items())] + [(1, 1, 65), (3, 2, 12)]


def filter2d_case(up, down, k, dtype):
    import filter2d_oracle as O
    import test_gpu_filter2d as T

    assert ((up, down, k) in O.FAMILIES) == ((up, down, k) != (3, 2, 12))
    for padding in O.BOTH:
        T.check_family(up, down, k, dtype, padding)


# ---- composite_layers --------------------------------------------------------------------------------------------------------
def composite_case(K, H, W, dtype):
    import test_gpu_composite_layers as T

    T.check_grid_point(K, 3, dtype, True, H, W, names=("capi",))
    T.check_grid_point(K, 3, dtype, True, H, W, names=("capi",), use_index=False)
    T.check_grid_point(K, 3, dtype, True, H, W, names=("capi",), use_background=False)


# ---- grid_scatter ------------------------------------------------------------------------------------------------------------
# 17 x 19 pixels: ragged 16 x 16 tiles in both axes; C = 3 and 5: channel blocks of four that do not divide.  An output of
# 13 x 11 fits the window of a tile whatever the grid (143 texels): the windowed route with its flush addressed from the
# tile's box.  61 x 83 under a uniformly random grid does not: the direct route (the full tile; the ragged ones stay windowed).
GRID_SCATTER_OUTPUTS = {"small": (13, 11), "large": (61, 83)}


def grid_scatter_cases():
    import grid_scatter_oracle as O

    cases = []
    for C in (3, 5):
        for kind, output in (("warp", "small"), ("uniform", "small"), ("uniform", "large")):
            for mode in O.MODES:
                for pad in O.PADDINGS:
                    for dtype in (F32, F64):
                        if output == "large" and (C, dtype) not in ((3, F32), (5, F64)):
                            continue
                        cases.append((C, kind, output, mode, pad, dtype))
    return cases


def grid_scatter_case(seed, C, kind, output, mode, pad, dtype):
    import grid_scatter_oracle as O
    import test_gpu_grid_scatter as T

    oh, ow = GRID_SCATTER_OUTPUTS[output]
    al = C == 5
    args = O.make_case(seed, 2, C, 17, 19, oh, ow, dtype=dtype, kind=kind) + (oh, ow, mode, pad, al)
    counts = T.route_counts()
    got = T.hip(*args, api="capi", needs=(True, False), counts=counts)
    assert got[2] is None
    T.compare(got, *args, f"grid_scatter C={C} {kind} {oh}x{ow} {mode} {pad} {TAG[dtype]}")
    windowed, direct = counts.tolist()
    assert 0 < windowed + direct <= T.tiles(2, 17, 19), (windowed, direct)
    if output == "small":
        assert direct == 0, (windowed, direct)
    else:
        assert direct >= 1, (windowed, direct)


# ---- msi, transform_distort: the operators' own C-ABI tests -------------------------------------------------------------------
def msi_case(name, dtype):
    import msi_oracle as O
    import test_gpu_msi as T

    assert name != "inside" or O.case(name)[0][0].shape[0] % 256 != 0  # a ragged last workgroup
    T.test_cases_against_the_oracle(name, dtype, "capi")


def transform_distort_case(name, dtype):
    import test_gpu_transform_distort as T

    T.test_c_abi_matches_the_reference_fixture(name, dtype)  # forward with v_cam, backward; `_shared` names: one vertex set


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def geometry_case(name):
    import test_gpu_geometry as T

    d32, d64 = T._load("f32"), T._load("f64")
    got64 = T._run_all_capi(T._fixture_case(d64, name), F64, DEV)
    got32 = T._run_all_capi(T._fixture_case(d32, name), F32, DEV)
    T._check_against_the_fixtures(name, got64, got32, d32, d64)


# ---- rasterize_layers ----------------------------------------------------------------------------------------------------------
def rasterize_layers_case(scene, K):
    import layers_oracle as LO
    import test_gpu_rasterize_layers as T
    from drtk_amd import capi

    v, vi, H, W = LO.scene_inputs(scene)
    wd, wi = T.load_layers(scene)
    assert wd.shape[1] >= K
    got = capi.rasterize_layers(v.to(DEV), vi.to(DEV), H, W, K)
    T.same(got, (wd[:, :K], wi[:, :K]), f"{scene} K={K}")
    T.check_order(*got)


# ---- image losses, mipmap_pyramid ------------------------------------------------------------------------------------------------
def image_loss_case(name, padding, weighted, dtype):
    import image_loss_oracle as O
    import test_gpu_image_loss as T

    shape, k, paddings, _ = O.STRUCTURAL_CASES[name]
    assert padding in paddings
    T.check_c_abi_case(shape, k, padding, weighted, dtype)  # the map, both means, their maps [3,N,C,OH,OW] and all three backward calls


# of its SHAPES, those with partial tiles: odd on both axes, odd drops inside a tile, a partial last tile of many, 11 levels
MIPMAP_PYRAMID_SHAPES = [(1, 1, 65, 63), (2, 3, 70, 130), (1, 1, 36, 4100), (1, 1, 1100, 1030)]


def mipmap_pyramid_case(shape, dtype, absent):
    import test_gpu_mipmap_pyramid as T
    from drtk_amd import capi

    assert shape in T.SHAPES and (shape[2] % 64 or shape[3] % 64)
    x, want, grads, want_grad = T.problem(shape, None, dtype)
    assert len(want) == T.max_levels(*shape[2:]) > absent >= 0
    out = capi.mipmap_pyramid(x, len(want))
    for l, (a, b) in enumerate(zip(out, want)):
        assert a.shape == b.shape and th.equal(a, b), f"level {l}"
    assert th.equal(capi.mipmap_pyramid_backward(grads), want_grad)
    some = [None if l == absent else g for l, g in enumerate(grads)]
    assert th.equal(capi.mipmap_pyramid_backward(some, grad_input=capi._out(*shape, dtype=dtype, device=DEV)), T.recurrence(some, x))


def fuzz_image_ops_case(seed):
    import fuzz_image_ops as F

    c = F.make_case(seed)
    try:
        F.run_case(c, check_guards=False)  # they are checked, and counted, after the case
    except AssertionError as e:
        raise AssertionError(f"{F.describe(c)}: {e}") from e


def fuzz_added_ops_case(seed):
    import fuzz_added_ops as F

    c = F.make_case(seed)
    try:
        F.run_case(c, check_guards=False)  # they are checked, and counted, after the case
    except AssertionError as e:
        raise AssertionError(f"{F.describe(c)}: {e}") from e


def fuzz_geometry_case(seed):
    import fuzz_geometry as F

    c = F.make_case(seed)
    try:
        F.run_case(c, check_guards=False)  # they are checked, and counted, after the case
    except AssertionError as e:
        raise AssertionError(f"{F.describe(c)}: {e}") from e


def cases():
    """[(name, function, arguments)], in the order they run"""
    import image_loss_oracle
    import msi_oracle
    import test_gpu_composite_layers as TC
    import test_gpu_geometry as TG
    import transform_distort_oracle

    out = [("guard", guard_reports_a_write_outside, ())]
    for up, down, k in filter2d_triples():
        for dtype in (F32, F64, F16):
            out.append((f"filter2d/{up}_{down}_{k}/{TAG[dtype]}", filter2d_case, (up, down, k, dtype)))
    for K in (1, 4, 5, 8):
        for H, W in TC.TAIL_SHAPES:
            for dtype in (F32, F64):
                out.append((f"composite_layers/K{K}/{H}x{W}/{TAG[dtype]}", composite_case, (K, H, W, dtype)))
    for i, (C, kind, output, mode, pad, dtype) in enumerate(grid_scatter_cases()):
        out.append((f"grid_scatter/C{C}/{kind}_{output}/{mode}/{pad}/{TAG[dtype]}", grid_scatter_case, (7000 + i, C, kind, output, mode, pad, dtype)))
    for name in msi_oracle.CASES:
        for dtype in (F32, F64):
            out.append((f"msi/{name}/{TAG[dtype]}", msi_case, (name, dtype)))
    for name in transform_distort_oracle.CASE_NAMES:
        for dtype in (F32, F64):
            out.append((f"transform_distort/{name}/{TAG[dtype]}", transform_distort_case, (name, dtype)))
    for name in TG.NAMES:
        out.append((f"geometry/{name}", geometry_case, (name,)))
    for scene in ("ragged_f32", "edge_cases_f32"):
        for K in (1, 3, 8):
            out.append((f"rasterize_layers/{scene}/K{K}", rasterize_layers_case, (scene, K)))
    for name, (_, _, paddings, _) in image_loss_oracle.STRUCTURAL_CASES.items():
        if name == "five_by_two":  # the interior-tile case and the slot cases: every tile kind and every pass of the finalize kernel
            continue
        for padding in paddings:
            for weighted in (False, True):
                for dtype in (F32, F64):
                    out.append((f"image_loss/{name}/{padding}/{'weighted' if weighted else 'plain'}/{TAG[dtype]}", image_loss_case, (name, padding, weighted, dtype)))
    for i, shape in enumerate(MIPMAP_PYRAMID_SHAPES):
        for dtype in (F32, F64):
            out.append((f"mipmap_pyramid/{'x'.join(map(str, shape))}/{TAG[dtype]}", mipmap_pyramid_case, (shape, dtype, (0, 1, 3, 7)[i])))
    for seed in range(20):
        out.append((f"fuzz_image_ops/seed{seed}", fuzz_image_ops_case, (seed,)))
    for seed in range(20):
        out.append((f"fuzz_added_ops/seed{seed}", fuzz_added_ops_case, (seed,)))
    for seed in range(20):
        out.append((f"fuzz_geometry/seed{seed}", fuzz_geometry_case, (seed,)))
    assert len({c[0] for c in out}) == len(out)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the names of the cases and leave (no GPU needed)")
    ap.add_argument("--only", metavar="NAME", help="run the guard check and the cases called NAME or NAME/...")
    a = ap.parse_args()
    todo = cases()
    if a.only:
        todo = [c for c in todo if c[0] == "guard" or c[0] == a.only or c[0].startswith(a.only + "/")]
        assert len(todo) > 1, f"no case is called {a.only}"
    if a.list:
        print("\n".join(c[0] for c in todo))
        sys.exit(0)
    from drtk_amd import capi

    assert capi._GUARD > 0 and capi._POISON, "run with DRTK_CAPI_GUARD=g (g = 1, 2, 3) and DRTK_CAPI_POISON=1 in the environment"
    bad = 0
    for name, fn, args in todo:
        try:
            fn(*args)
            checked = capi.check_guards()
            assert checked >= 1 or name == "guard", "the case went through no allocation of the binding"
        except AssertionError as e:
            bad += 1
            print(f"FAIL {name}: {str(e)[:600]}", flush=True)
        except Exception as e:  # an error of the runtime or the library: nothing more is started on the device
            print(f"ERROR {name}: {type(e).__name__}: {str(e)[:600]}\nstopped after {name}", flush=True)
            sys.exit(2)
    print(f"{len(todo) - bad}/{len(todo)} cases passed (DRTK_CAPI_GUARD={capi._GUARD})")
    sys.exit(1 if bad else 0)
