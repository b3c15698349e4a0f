"""No GPU: drtk_amd.nearest_points / chamfer_distance -- the header's constants and the cases built from them, the C ABI's
argument checks and workspace sizes on either side of the split threshold, the PyTorch formulation (the route of CPU
tensors) against the independent oracle (tests/nearest_oracle.py) bit for bit forward and to 1e-12 of scale in float64
backward, the weighting rules of chamfer_distance, names, and the guarded script's case list."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch as th
from conftest import ROOT

import nearest_oracle as O
from f64_distance import assert_within_f64_distance

GRADS = ("grad_p", "grad_q")


def assert_exact_zeros(got, ref, what):
    """The elements stated to be exactly 0 (compared with th.equal): the gradient of a query without a neighbour and of a
    target nobody chose -- where the gradient has one row per view (a shared input holds the sum over the views)."""
    idx = ref["idx"]
    n = idx.shape[0]
    gp, gq = got["grad_p"], got["grad_q"]
    if gp.dim() == 3 and gp.shape[0] == n:
        assert th.equal(gp[idx < 0], th.zeros_like(gp[idx < 0])), (what, "grad_p")
    if gq.dim() == 3 and gq.shape[0] == n:
        for v in range(n):
            chosen = th.zeros(gq.shape[1], dtype=th.bool)
            chosen[idx[v][idx[v] >= 0]] = True
            assert th.equal(gq[v][~chosen], th.zeros_like(gq[v][~chosen])), (what, "grad_q")


def test_names_are_exported_and_declared():
    import drtk_amd
    from drtk_amd import capi

    for n in ("nearest_points", "chamfer_distance"):
        assert n in drtk_amd.__all__ and callable(getattr(drtk_amd, n))
        assert getattr(drtk_amd, n).__module__ == "drtk_amd.nearest"
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    for n in ("drtk_amd_nearest_forward", "drtk_amd_nearest_backward", "drtk_amd_nearest_forward_workspace_bytes",
              "drtk_amd_nearest_backward_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in capi.EXPORTS
    for gap in ("K > 1", "ragged", "point-to-triangle", "float16"):
        assert gap in drtk_amd.nearest_points.__doc__
    import drtk

    assert not hasattr(drtk, "nearest_points")  # the drop-in mirrors the reference, which has no such name


def test_header_constants_and_the_cases_built_from_them():
    from drtk_amd import capi

    assert (O.R, O.QUERIES, O.TILE, O.SPLIT_BLOCKS, O.CHUNK) == (capi.NEAREST_R, capi.NEAREST_QUERIES, capi.NEAREST_TILE,
                                                                 capi.NEAREST_SPLIT_BLOCKS, capi.NEAREST_CHUNK)
    assert O.QUERIES == 256 * O.R and O.R % 2 == 0
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "nearest.hip")).read()
    for name in ("R", "QUERIES", "TILE", "SPLIT_BLOCKS", "CHUNK"):
        assert "DRTK_NEAREST_" + name in src

    def shape(name):
        p, q, g = O.case(name)
        n = g.shape[0]
        return n, p.shape[-2], q.shape[-2], O.split(n, p.shape[-2], q.shape[-2])

    assert shape("one")[:3] == (1, 1, 1)
    assert [shape(k)[1] for k in ("queries_minus", "queries_exact", "queries_plus")] == [O.QUERIES - 1, O.QUERIES, O.QUERIES + 1]
    assert shape("not_multiple_of_r")[1] % O.R != 0
    assert [shape(k)[2] for k in ("tile_minus", "tile_exact", "tile_plus_split_short")] == [O.TILE - 1, O.TILE, O.TILE + 1]
    assert shape("tile_minus")[3][0] == 1 and shape("tile_exact")[3][0] == 1 and shape("tile_plus_split_short")[3] == (2, O.TILE)
    assert shape("one_target")[2] == 1 and shape("one_target")[1] > 2 * O.QUERIES
    # either side of the threshold, the same targets: one workgroup fewer and the targets are split
    assert shape("at_split_threshold")[3][0] == 1 and shape("at_split_threshold")[0] == O.SPLIT_BLOCKS
    assert shape("below_split_threshold")[3][0] == 2 and shape("below_split_threshold")[2] == shape("at_split_threshold")[2] > O.TILE
    s, length = shape("split_six")[3]
    assert s == 6 and 0 < shape("split_six")[2] - 5 * length < length
    s, length = shape("split_long_ranges")[3]
    assert s == 2 and length == 3 * O.TILE and shape("split_long_ranges")[2] - length < length
    assert O.case("shared_expand")[0].stride(0) == 0 and O.case("shared_expand")[1].stride(0) == 0
    assert O.case("shared_q_2d")[1].dim() == 2 and O.case("shared_p_2d")[0].dim() == 2 and O.case("shared_p")[0].shape[0] == 1
    # the structure of the chosen indices that the backward cases are named for
    idx = O.reference("all_one_target", th.float32)["idx"]
    assert bool((idx == 2).all()) and idx.shape[1] > 3 * O.CHUNK
    idx = O.reference("own_target", th.float32)["idx"]
    assert th.equal(idx, th.arange(idx.shape[1]).expand_as(idx)) and idx.shape[1] > 2 * O.CHUNK
    counts = th.bincount(O.reference("runs_end_on_chunk_edges", th.float32)["idx"][0], minlength=6).tolist()
    assert counts == [O.CHUNK, O.CHUNK, 0, 2 * O.CHUNK, 5, 0]
    idx = O.reference("minus_one_front", th.float32)["idx"]
    assert int((idx[0] < 0).sum()) == 37 and int((idx[0] == 0).sum()) == O.CHUNK - 37
    for dtype in (th.float32, th.float64):
        r = O.reference("duplicates_across_tiles_and_splits", dtype)
        assert set(r["idx"].unique().tolist()) == {0, 7} and shape("duplicates_across_tiles_and_splits")[3] == (3, O.TILE)
        assert set(O.reference("duplicates_one_range", dtype)["idx"].unique().tolist()) == {5}
        assert bool((O.reference("second_split_wins", dtype)["idx"] >= O.TILE).all())
        r = O.reference("all_rejected", dtype)
        assert bool((r["idx"] == -1).all()) and bool(th.isinf(r["dist2"]).all())
        r = O.reference("rejected_in_second_split", dtype)
        assert int(r["idx"].max()) < O.TILE and int((r["idx"] < 0).sum()) == 1
    q = O.case("lattice")[1]
    assert th.equal(q, q.round())
    r32, r64 = O.reference("overflow_target", th.float32), O.reference("overflow_target", th.float64)
    assert not bool((r32["idx"] == 3).any()) and bool(th.isfinite(r32["dist2"]).all()) and bool(th.isfinite(r64["dist2"]).all())
    shapes = {(tuple(O.build_case(s)[0].shape), tuple(O.build_case(s)[1].shape)) for s in O.SEEDS}
    assert len(shapes) > 30
    for s in O.SEEDS:
        p, q, g = O.build_case(s)
        assert g.shape[0] * p.shape[-2] * q.shape[-2] <= 2 * 4096 * 4096


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("key", list(O.CASES) + list(O.SEEDS))
def test_cpu_formulation_matches_the_oracle(key, dtype):
    import drtk_amd

    p, q, g = O.case(key) if isinstance(key, str) else O.build_case(key)
    got = O.results(drtk_amd.nearest_points, p, q, g, dtype)
    ref = O.reference(key, dtype)
    assert got["dist2"].dtype == dtype and got["idx"].dtype == th.int64
    assert th.equal(got["dist2"], ref["dist2"]) and th.equal(got["idx"], ref["idx"]), key  # bit for bit
    for k in GRADS:
        want = ref[k] if dtype == th.float64 else ref[k + "_own"]
        assert got[k].shape == want.shape and got[k].dtype == dtype, (key, k)
        scale = float(want.abs().max())
        assert scale > 0 or key in O.ALL_ZERO, (key, k)
        if dtype == th.float64:
            assert float((got[k] - want).abs().max()) <= 1e-12 * scale, (key, k)
        else:  # the project's float32 bound: the distance to the float64 result against the float32 oracle's own
            assert_within_f64_distance(got[k], want, ref[k], f"{key} {k}")
    assert_exact_zeros(got, ref, key)


def test_empty_inputs_on_the_cpu():
    import drtk_amd

    p = th.randn(2, 5, 3, dtype=th.float64, requires_grad=True)
    d, i = drtk_amd.nearest_points(p, th.zeros(2, 0, 3, dtype=th.float64))
    assert d.shape == (2, 5) and bool(th.isinf(d).all()) and bool((i == -1).all()) and i.dtype == th.int64
    (g,) = th.autograd.grad(d, p, th.ones_like(d))
    assert th.equal(g, th.zeros_like(p))
    d, i = drtk_amd.nearest_points(th.zeros(2, 0, 3), th.zeros(1, 7, 3))
    assert d.shape == (2, 0) and i.shape == (2, 0)
    d, i = drtk_amd.nearest_points(th.zeros(0, 4, 3), th.zeros(0, 7, 3))
    assert d.shape == (0, 4) and i.shape == (0, 4)


def test_argument_errors_on_the_cpu():
    import drtk_amd

    p, q = th.zeros(2, 5, 3), th.zeros(2, 7, 3)
    for bad in (lambda: drtk_amd.nearest_points(p[..., :2], q), lambda: drtk_amd.nearest_points(p, q[0, 0]),
                lambda: drtk_amd.nearest_points(p, th.zeros(3, 7, 3)), lambda: drtk_amd.nearest_points(p[None], q)):
        with pytest.raises(ValueError, match="expected"):
            bad()
    with pytest.raises(TypeError, match="dtype of p"):
        drtk_amd.nearest_points(p, q.double())
    with pytest.raises(TypeError, match="floating"):
        drtk_amd.nearest_points(p.long(), q.long())


def test_chamfer_distance_against_its_definition_and_its_weighting_rules():
    import drtk_amd

    gen = th.Generator().manual_seed(3)
    x = th.randn(3, 40, 3, dtype=th.float64, generator=gen)
    y = th.randn(3, 55, 3, dtype=th.float64, generator=gen)
    x[1, 4] = float("nan")  # a point without a neighbour: weight 0 on its side, never chosen on the other
    xw = th.rand(3, 40, dtype=th.float64, generator=gen)
    yw = th.rand(3, 55, generator=gen) < 0.5  # bool
    xw[2] = 0  # a view without weight on the x side: that mean is 0, not NaN
    for kw in ({}, {"squared": False}, {"bidirectional": False}, {"x_weights": xw}, {"x_weights": xw, "y_weights": yw},
               {"x_weights": xw, "y_weights": yw, "squared": False}):
        got = drtk_amd.chamfer_distance(x, y, **kw)
        want = O.chamfer(x, y, **kw)
        assert got.shape == () and bool(th.isfinite(got)) and abs(float(got - want)) <= 1e-13 * float(want), kw
    # the definition, spelled out on the unweighted squared form
    d_xy, i_xy = O.nearest(x, y)
    d_yx, _ = O.nearest(y, x)
    per_view = th.stack([d_xy[v][i_xy[v] >= 0].mean() + d_yx[v].mean() for v in range(3)])
    assert abs(float(drtk_amd.chamfer_distance(x, y) - per_view.mean())) <= 1e-13 * float(per_view.mean())
    # all weights zero: exactly 0, and a finite (zero) gradient
    xr = x.clone().nan_to_num(0.0).requires_grad_(True)
    z = drtk_amd.chamfer_distance(xr, y, x_weights=th.zeros(3, 40), bidirectional=False)
    assert float(z.detach()) == 0.0
    z.backward()
    assert th.equal(xr.grad, th.zeros_like(xr))
    # every point NaN: no neighbours at all, 0
    assert float(drtk_amd.chamfer_distance(th.full((2, 4, 3), float("nan")), th.zeros(2, 5, 3))) == 0.0
    # coincident sets with squared=False: the gradient is finite (the subgradient 0 at distance 0)
    yr = y.clone().requires_grad_(True)
    drtk_amd.chamfer_distance(y.clone(), yr, squared=False).backward()
    assert bool(th.isfinite(yr.grad).all())
    # shared sets broadcast like nearest_points
    a = drtk_amd.chamfer_distance(x.nan_to_num(0.0), y[0])
    b = drtk_amd.chamfer_distance(x.nan_to_num(0.0), y[:1].expand(3, -1, -1).contiguous())
    assert th.equal(a, b)
    with pytest.raises(ValueError, match="x_weights"):
        drtk_amd.chamfer_distance(x, y, x_weights=th.ones(3, 41))


def _i64(x):
    return ctypes.c_int64(int(x))


def test_workspace_bytes_follow_the_launch_rule():
    from drtk_amd import capi

    L = capi.lib()
    out = ctypes.c_size_t(123)

    def fwd_bytes(dtype, n, num_p, num_q):
        assert L.drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(dtype), _i64(n), _i64(num_p), _i64(num_q), ctypes.byref(out)) == 0
        return out.value

    for dtype, size in ((0, 4), (1, 8)):
        # S == 1: enough workgroups, or one tile of targets, or nothing to do
        assert fwd_bytes(dtype, O.SPLIT_BLOCKS, 3, O.TILE + 5) == 0
        assert fwd_bytes(dtype, 1, O.SPLIT_BLOCKS * O.QUERIES, 50 * O.TILE) == 0
        assert fwd_bytes(dtype, 1, 70, O.TILE) == 0 and fwd_bytes(dtype, 0, 70, 5 * O.TILE) == 0 and fwd_bytes(dtype, 3, 0, 5 * O.TILE) == 0
        # one workgroup fewer: split, N*S*P partials of a distance and an int32 index
        for n, num_p, num_q in ((O.SPLIT_BLOCKS - 1, 3, O.TILE + 5), (1, 70, O.TILE + 1), (1, 40, 5 * O.TILE + 300), (300, 2, 4 * O.TILE + 7),
                                (8, 5023, 100000), (1, (O.SPLIT_BLOCKS - 1) * O.QUERIES, 50 * O.TILE), (2, 3000, 7 * O.TILE)):
            s, _ = O.split(n, num_p, num_q)
            assert s > 1 and (s, _) == capi.nearest_split(n, num_p, num_q)
            assert fwd_bytes(dtype, n, num_p, num_q) == n * s * num_p * (size + 4), (n, num_p, num_q)
        assert O.split(8, 5023, 100000)[0] * 8 * 5 >= O.SPLIT_BLOCKS  # the small mesh against the scan fills the card
        assert L.drtk_amd_nearest_backward_workspace_bytes(ctypes.c_int(dtype), _i64(3), _i64(101), _i64(7), ctypes.c_int(1), ctypes.byref(out)) == 0
        assert out.value == (3 * 101 * 28 + 7) // 8 * 8
        assert L.drtk_amd_nearest_backward_workspace_bytes(ctypes.c_int(dtype), _i64(3), _i64(101), _i64(7), ctypes.c_int(0), ctypes.byref(out)) == 0
        assert out.value == 0
    assert L.drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(7), _i64(1), _i64(1), _i64(1), ctypes.byref(out)) == -1
    assert L.drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(2), _i64(1), _i64(1), _i64(1), ctypes.byref(out)) == -1  # no float16
    assert L.drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(0), _i64(-1), _i64(1), _i64(1), ctypes.byref(out)) == -1
    assert L.drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(0), _i64(1), _i64(1), _i64(1 << 31), ctypes.byref(out)) == -1
    assert L.drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(0), _i64(1), _i64(1), _i64(1), ctypes.c_void_p(0)) == -1
    assert L.drtk_amd_nearest_backward_workspace_bytes(ctypes.c_int(0), _i64(1), _i64(-1), _i64(1), ctypes.c_int(1), ctypes.byref(out)) == -1


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)

    def fwd(N=1, P=70, M=O.TILE + 1, p_sN=0, p_sP=3, q_sN=0, q_sM=3, dtype=0, pp=p, qq=p, d=p, i=p, ws=4096, nbytes=1 << 20):
        return L.drtk_amd_nearest_forward(ctypes.c_int(dtype), pp, _i64(p_sN), _i64(p_sP), qq, _i64(q_sN), _i64(q_sM), _i64(N), _i64(P),
                                          _i64(M), d, i, ctypes.c_void_p(ws), ctypes.c_size_t(nbytes), z)

    assert fwd(dtype=5) == -1 and fwd(dtype=2) == -1 and fwd(N=-1) == -1 and fwd(P=-1) == -1 and fwd(M=-2) == -1
    assert fwd(p_sP=2) == -1 and fwd(q_sM=0) == -1 and fwd(N=2, p_sN=3 * 70 - 1) == -1 and fwd(N=2, q_sN=-5) == -1
    assert fwd(pp=z) == -1 and fwd(qq=z) == -1 and fwd(d=z) == -1 and fwd(i=z) == -1
    need = 70 * 2 * 8  # S = 2
    assert fwd(ws=0, nbytes=0) == -2 and fwd(nbytes=need - 1) == -2  # DRTK_ERR_WORKSPACE_TOO_SMALL
    assert fwd(ws=4096 + 4) == -1                                    # misaligned
    assert fwd(N=0) == 0 and fwd(P=0) == 0                            # nothing to launch

    def bwd(N=1, P=70, M=9, gp=p, gq=p, gp_B=1, gq_B=1, g=p, idx=p, order=p, ws=4096, nbytes=1 << 20, dtype=0, p_sP=3):
        return L.drtk_amd_nearest_backward(ctypes.c_int(dtype), g, p, _i64(0), _i64(p_sP), p, _i64(0), _i64(3), idx, order, _i64(N), _i64(P),
                                           _i64(M), _i64(gp_B), gp, _i64(gq_B), gq, ctypes.c_void_p(ws), ctypes.c_size_t(nbytes), z)

    assert bwd(gp=z, gq=z) == -1 and bwd(dtype=9) == -1 and bwd(gp_B=2) == -1 and bwd(gq_B=3) == -1 and bwd(p_sP=1) == -1 and bwd(P=-3) == -1
    assert bwd(g=z) == -1 and bwd(idx=z) == -1 and bwd(order=z) == -1
    assert bwd(ws=0, nbytes=0) == -2 and bwd(nbytes=70 * 28 - 1) == -2 and bwd(ws=4096 + 4) == -1
    assert bwd(gq=z, P=0) == 0  # nothing to launch


def test_guarded_script_lists_its_cases():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_nearest.py"), "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    names = r.stdout.split()
    assert len(names) == len(set(names)) >= 2 * len(O.CASES) and all(n.count("/") >= 2 for n in names)
