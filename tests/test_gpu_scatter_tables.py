"""-m gpu: the vertex-table scatters (drtk_amd/csrc/segscatter.hpp) on index images that fill, collide in and bypass their
tables -- render_backward_kernel, interpolate_backward_small_kernel, interpolate_backward_wide_kernel (direct atomics, padded
workspace rows, the workgroup table at 128 / 64 / 32 / 16 slots) and normal_matrix_values_kernel, each through the C-ABI
wrappers of drtk_amd.capi against oracle/oracle.py.  The index images are tests/scatter_table_cases.py's -- a triangle of its
own at every pixel (render backward: in every column -- a lone term's depth component rounds by the whole allowance in the
float32 oracle itself, see per_column), keys of one home slot, hot vertices in overflowing and in calm tiles, runs cut at lanes 15|16, 31|32 and
63|64, one wave of foreground per workgroup, faces that repeat a vertex -- and tests/test_scatter_table_cases_host.py proves
on the CPU that each has the property it is named for, so that the table-full and probes-exhausted fallbacks are REQUIRED
here, not met by accident.

Bounds, none new: float32 vertex gradients element by element (tests/f64_distance.py, ELEMENT_ULPS and FLOOR of
tests/test_gpu_f64_distance.py) against the oracle in double; A^T A values by the bound of tests/fuzz_next_ops.py; double at
1e-10 absolute and relative; the bary gradient within 1e-6 of its magnitude, identical between routes, exactly zero on the
background.  Outputs are allocated poisoned; a vertex no pixel names must read exactly 0.  The route of every interpolate
call is asserted from the kernel timing report by kernel name and, for the wide kernel, template flavour."""
import re

import pytest
import torch as th

import scatter_table_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}  # operator -> (largest element-wise excess of a kernel, the float32 oracle's own use of the allowance, case)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for op, (excess, own, what) in sorted(WORST.items()):
        print(f"\n[scatter tables] {op}: largest element-wise excess {excess:.3f} (1 = the bound), float32 oracle's own {own:.3f} of the ulps allowance -- {what}")


def _note(op, excess, own, what):
    if op not in WORST or excess > WORST[op][0]:
        WORST[op] = (excess, own, what)


def dev(x):
    return x.to(DEV) if isinstance(x, th.Tensor) else x


def _poisoned():
    from drtk_amd import capi

    assert capi._POISON, "conftest.py sets DRTK_CAPI_POISON before drtk_amd.capi is imported"


def _unreferenced(case):
    """[N,V] bool: vertices that no pixel of the view names."""
    used = th.zeros(case.N, case.V, dtype=th.bool)
    for n in range(case.N):
        used[n, P.faces_of(case, n).long()[case.idx[n][case.idx[n] >= 0].long()].flatten()] = True
    assert not bool(used.all())
    return ~used


def _f64_close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got - ref).abs() > 1e-10 + 1e-10 * ref.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beyond 1e-10 + 1e-10 |ref|, worst {float((got - ref).abs().max()):.3e}"


def _vertex_gradient(got, o32, o64, A, op, case, what):
    _poisoned()
    got = got.detach().cpu()
    assert bool((got[_unreferenced(case)] == 0).all()), f"{what}: a vertex no pixel names is not exactly zero"
    if got.dtype == th.float64:
        return _f64_close(got, o64, what)
    excess, own = P.vertex_excess(got, o32, o64, A, op, what)
    print(f"{what}: max|f64| = {float(o64.abs().max()):.3e}, element-wise excess {excess:.3f}, float32 oracle's own {own:.3f}")
    _note(op, excess, own, what)


# ---- render backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("spec", P.RENDER_SPECS, ids=P.spec_id)
def test_render_backward(spec, dtype):
    from drtk_amd import capi

    case = P.build(spec)
    gd, gb = P.render_inputs(case)
    o32, o64, A = P.render_reference_cached(case)
    got = capi.render_backward(dev(case.v.to(dtype)), dev(case.vi), dev(case.idx), dev(gd.to(dtype)), dev(gb.to(dtype)))
    _vertex_gradient(got, o32, o64, A, "render", case, f"render backward {dtype}, {case.name}")


@pytest.mark.parametrize("spec", P.RENDER_F64_SPECS, ids=P.spec_id)
def test_render_backward_double_on_a_triangle_per_pixel(spec):
    """768 distinct vertices in a wave tile, other ones in every row: whatever found a slot in row 0, rows 1 ... 3 go round
    the table.  In double only -- at 1e-10 a lone term's rounding is no matter, while in float32 the oracle's own depth
    component uses the element-wise bound's whole allowance on an element that is ONE term (see per_column)."""
    from drtk_amd import capi

    case = P.build(spec)
    gd, gb = P.render_inputs(case)
    _, o64, _ = P.render_reference_cached(case)
    got = capi.render_backward(dev(case.v.double()), dev(case.vi), dev(case.idx), dev(gd.double()), dev(gb.double()))
    _vertex_gradient(got, None, o64, None, "render", case, f"render backward f64, {case.name}")


# ---- interpolate backward ----------------------------------------------------------------------------------------------------
def _kernels(fn):
    from drtk_amd import capi

    capi.kernel_timing_begin()
    out = fn()
    th.cuda.synchronize()
    return out, [k.strip("()") for k in capi.kernel_timing_report()]


def _route(names):
    """('scan' | 'wide' | 'generic', wide: has the workgroup table -- None if the name did not parse --, compacted padded rows)."""
    base = {n.split("<")[0] for n in names}
    compact = "compact_rows_kernel" in base
    if "interpolate_backward_small_kernel" in base:
        return "scan", None, compact
    if "interpolate_backward_wide_kernel" in base:
        (name,) = [n for n in names if n.startswith("interpolate_backward_wide_kernel")]
        m = re.match(r"interpolate_backward_wide_kernel<(.*)>$", name.replace(" ", ""))
        args = m.group(1).split(",") if m else []
        table = {"true": True, "false": False}.get(args[2]) if len(args) == 5 else None  # <T, HAS_BARY, TABLE, CH, ANYC>
        return "wide", table, compact
    assert "interpolate_backward_kernel" in base, names
    return "generic", None, compact


def _interpolate(case, C, dtype, requests=((True, True),), workspace=None, inputs=None, ref=None, expect=None):
    """capi.interpolate_backward on one case against the oracle; expect = (route, table, compacted) of the both-gradients call.
    Returns {request: (attr_grad, bary_grad)} on the CPU."""
    from drtk_amd import capi

    attr, go = P.interp_inputs(case, C) if inputs is None else inputs
    r = P.interp_reference_cached(case, C) if ref is None else ref
    args = (dev(go.to(dtype)), dev(attr.to(dtype)), dev(case.vi), dev(case.idx), dev(case.bary.to(dtype)))
    out = {}
    for want_a, want_b in requests:
        what = f"interpolate backward C={C} {dtype} workspace={workspace} request=({want_a}, {want_b}), {case.name}"
        (ag, bg), names = _kernels(lambda: capi.interpolate_backward(*args, want_a, want_b, workspace=workspace))
        if expect is not None and (want_a, want_b) == requests[0]:
            route, table, compact = _route(names)
            print(f"{what}: launched {names}")
            assert route == expect[0] and compact == expect[2], (what, names)
            if route == "wide":  # the launch-site name carries <T, HAS_BARY, TABLE, CH, ANYC>: a changed list must fail here
                assert table is not None, f"{what}: the wide kernel's template flavour no longer parses from {names}"
            assert table == expect[1], (what, names)
        assert (ag is None) == (not want_a) and (bg is None) == (not want_b)
        if want_a:
            _vertex_gradient(ag, r["a32"], r["a64"], r["aA"], "interpolate", case, what)
        if want_b:
            bg = bg.detach().cpu()
            _poisoned()
            assert bool((bg[(case.idx == -1)[:, None].expand_as(bg)] == 0).all()), f"{what}: the bary gradient of the background is not exactly zero"
            if dtype == th.float64:
                _f64_close(bg, r["b64"], what)
            else:
                assert float((bg - r["b32"]).abs().max()) <= 1e-6 * float(r["b32"].abs().max()), f"{what}: bary gradient"
        out[want_a, want_b] = (ag.detach().cpu() if want_a else None, bg if want_b else None)
    return out


ALL_REQUESTS = ((True, True), (True, False), (False, True))


def _requests(spec):
    return ALL_REQUESTS if spec in (("per_pixel", *P.DEFAULT), ("mixed", *P.DEFAULT)) else ALL_REQUESTS[:1]


def _ids(v):
    return P.spec_id(v) if isinstance(v, tuple) else str(v).replace("torch.", "")


# (the edge shapes once per kernel: at C = 3 and, for the workgroup table, at C = 20)
@pytest.mark.parametrize("spec,C,dtype", [(s, C, dt) for C, dt in P.REGISTER_SCAN for s in P.interp_specs(edges=C == 3)], ids=_ids)
def test_interpolate_backward_register_scan(spec, C, dtype):
    _interpolate(P.build(spec), C, dtype, _requests(spec), expect=("scan", None, False))


@pytest.mark.parametrize("C", P.WIDE_DIRECT)
@pytest.mark.parametrize("spec", P.interp_specs(), ids=P.spec_id)
def test_interpolate_backward_wide_direct_atomics(spec, C):
    """Rows of whole 64-byte segments (16, 32) and C = 100, whose 400-byte rows are not but whose table would have 8 slots:
    no table, every run's sums straight to global memory."""
    _interpolate(P.build(spec), C, th.float32, _requests(spec), expect=("wide", False, False))


@pytest.mark.parametrize("C", P.WIDE_PADDED)
@pytest.mark.parametrize("spec", P.interp_specs(), ids=P.spec_id)
def test_interpolate_backward_wide_padded_workspace(spec, C):
    """The default call at C = 13: direct atomics into rows padded to 64 bytes, compacted afterwards; the bary gradient is the
    table route's bit for bit."""
    case = P.build(spec)
    padded = _interpolate(case, C, th.float32, expect=("wide", False, True))
    table = _interpolate(case, C, th.float32, workspace=False, expect=("wide", True, False))
    assert th.equal(padded[True, True][1], table[True, True][1]), "the bary gradient does not depend on the route"


@pytest.mark.parametrize("spec,C", [(s, C) for C in P.WIDE_TABLE for s in P.interp_specs(P.wide_log2_slots(C), edges=C == 20)], ids=_ids)
def test_interpolate_backward_wide_workgroup_table(spec, C):
    """workspace=False: the workgroup's table of 128 (C = 12), 64 (13, 20), 32 (37) and 16 (99) slots; `collide` with ids of
    one home slot of THAT table.  C = 20 and 37 end in a chunk of 4 and 5 channels, 99 in one of 3: the sliced form, whose
    slices at pixels 16 / 32 / 48 start without a slot -- one vertex through the table and round it in one row."""
    _interpolate(P.build(spec), C, th.float32, _requests(spec), workspace=False, expect=("wide", True, False))


@pytest.mark.parametrize("spec", P.interp_specs(P.wide_log2_slots(20)), ids=P.spec_id)
def test_interpolate_backward_wide_table_attributes_only(spec):
    """C = 20 without the bary gradient takes the table with or without a workspace (nothing is padded)."""
    _interpolate(P.build(spec), 20, th.float32, ((True, False),), expect=("wide", True, False))


@pytest.mark.parametrize("spec", P.interp_specs(P.wide_log2_slots(P.WIDE_TABLE_F64)), ids=P.spec_id)
def test_interpolate_backward_wide_table_double(spec):
    """double: C = 9 stays with the register scan (rows not 32-byte aligned, C <= 11); C = 12 -- 96-byte rows -- takes the
    table of 128 slots."""
    C = P.WIDE_TABLE_F64
    _interpolate(P.build(spec), C, th.float64, expect=("wide", True, False))


@pytest.mark.parametrize("spec", [("per_pixel", *P.DEFAULT), ("mixed", *P.DEFAULT), ("long_runs", *P.DEFAULT)], ids=P.spec_id)
def test_the_16_slot_table_and_no_table_agree(spec):
    """C = 99 (16 slots) and C = 100 (the table dropped) on the same inputs -- C = 100's are C = 99's and one more channel: the
    first 99 channels of the attribute gradient meet C = 99's bound on either side of the switch, and each other's."""
    case = P.build(spec)
    attr, go = P.interp_inputs(case, 99)
    g = th.Generator().manual_seed(99100)
    one_more = th.rand(case.N, case.V, 1, generator=g), th.rand(case.N, 1, case.H, case.W, generator=g) * 2 - 1
    inputs = (th.cat([attr, one_more[0]], -1).contiguous(), th.cat([go, one_more[1]], 1).contiguous())
    a99 = _interpolate(case, 99, th.float32, workspace=False, expect=("wide", True, False))[True, True][0]
    r100 = P.interp_reference(case, 100, inputs=inputs)
    a100 = _interpolate(case, 100, th.float32, workspace=False, inputs=inputs, ref=r100, expect=("wide", False, False))[True, True][0]
    r = P.interp_reference_cached(case, 99)
    what = f"C = 100's first 99 channels, {case.name}"
    P.vertex_excess(a100[..., :99], r["a32"], r["a64"], r["aA"], "interpolate", what + ", against C = 99's reference")
    # ... and the two routes agree with EACH OTHER to the same element-wise bound: C = 99's result in the double oracle's place
    from f64_distance import elementwise_excess
    from test_gpu_f64_distance import ELEMENT_ULPS, FLOOR

    excess, worst, _ = elementwise_excess(a100[..., :99], r["a32"], a99, r["aA"], ELEMENT_ULPS["interpolate"], floor_rel=FLOOR)
    print(f"{what}: against C = 99's kernel result, element-wise excess {excess:.3f} (element {worst})")
    _note("interpolate, C = 100 against C = 99", excess, 0.0, what)
    assert excess <= 1.0, f"{what}: the two routes differ by {excess:.2f} x the element-wise bound at element {worst}"


def test_the_switch_over_between_register_scan_and_wide():
    """C = 10 (register scan) and C = 11 (wide) on `mixed`: both within the bound of their own reference."""
    case = P.mixed(*P.DEFAULT)
    _interpolate(case, 10, th.float32, expect=("scan", None, False))
    _interpolate(case, 11, th.float32, workspace=False, expect=("wide", True, False))
    _interpolate(case, 11, th.float32, expect=("wide", False, True))


# ---- A^T A values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("spec", P.NORMAL_SPECS, ids=P.spec_id)
def test_normal_matrix_values_and_backward(spec, dtype):
    from drtk_amd import capi
    import fuzz_next_ops as FN
    from f64_distance import elementwise_excess
    from test_gpu_f64_distance import ELEMENT_ULPS, FLOOR

    case = P.build(spec)
    r = P.normal_reference_cached(case)
    _poisoned()
    pair, idx, bary = dev(r["pair"]), dev(case.idx), dev(case.bary.to(dtype))
    got, names = _kernels(lambda: capi.interpolation_normal_matrix_values(pair, idx, bary, r["nnz"]))
    assert {n.split("<")[0] for n in names} >= {"normal_matrix_values_kernel"}, names
    got = got.detach().cpu()
    what = f"A^T A values {dtype}, {case.name}"
    assert bool((got[r["v64"] == 0] == 0).all()), f"{what}: an entry no pixel adds to is not exactly zero"
    bg = capi.interpolation_normal_matrix_values_backward(dev(r["gv"].to(dtype)), pair, idx, bary).detach().cpu()
    assert bool((bg[(case.idx == -1)[:, None].expand_as(bg)] == 0).all())
    if dtype == th.float64:
        _f64_close(got, r["v64"], what)
        _f64_close(bg, r["g64"], what + " backward")
        return
    err, own = P.normal_values_within(got, r, what)
    # (every term is a product of non-negative barycentrics: what was accumulated into an entry is the entry)
    excess, _, own_ratio = elementwise_excess(got, r["v32"], r["v64"], r["v64"], ELEMENT_ULPS["interpolate"], floor_rel=FLOOR)
    print(f"{what}: nnz = {r['nnz']}, |kernel - f64| = {err:.3e}, |oracle_f32 - f64| = {own:.3e}; "
          f"element-wise (reported, not asserted) {excess:.3f}, oracle's own {own_ratio:.3f}")
    _note("normal matrix values (element-wise figure, reported only)", excess, own_ratio, what)
    FN._close(bg, r["g32"], what + " backward", atol=1e-5, rtol=1e-5)  # the fuzzer's bar for this operator (per pixel: no scatter)


# ---- interpolation_matrix on faces that repeat a vertex --------------------------------------------------------------------------
def _row_multisets(cols, values):
    return [sorted(zip(c, v)) for c, v in zip(cols.tolist(), values.tolist())]


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [("repeated", *P.DEFAULT), ("repeated", 5, 65, True)], ids=P.spec_id)
def test_interpolation_matrix_on_repeated_vertices(spec, dtype):
    """Columns ascending per row, bit for bit; values bit for bit where a row's columns differ (the order is defined), and as
    the row's multiset of (column, value) where two or three corners are one vertex and the order among them is a tie."""
    import oracle as O
    from drtk_amd import capi

    case = P.build(spec)
    bary = case.bary.to(dtype)
    crow_o, col_o, val_o, rows_o = O.interpolation_matrix(case.vi, case.idx, bary)
    crow, col, val, rows = (t.cpu() for t in capi.interpolation_matrix(dev(case.vi), dev(case.idx), dev(bary)))
    assert th.equal(crow, crow_o) and th.equal(rows, rows_o) and th.equal(col, col_o), "structure"
    c3, v3, o3 = col_o.view(-1, 3), val.view(-1, 3), val_o.view(-1, 3)
    tie = (c3[:, 0] == c3[:, 1]) | (c3[:, 1] == c3[:, 2])
    assert 0 < int(tie.sum()) < tie.numel() and bool((c3[:, 0] == c3[:, 2]).any())
    assert th.equal(v3[~tie], o3[~tie]), "values of rows with three different columns"
    assert _row_multisets(c3[tie], v3[tie]) == _row_multisets(c3[tie], o3[tie]), "values of rows with a repeated column"
    print(f"{case.name} {dtype}: {int(tie.sum())} of {tie.numel()} rows repeat a column; {int((v3[tie] == o3[tie]).all(1).sum())} of them in the oracle's order")
    g = th.Generator().manual_seed(5)
    gv = (th.rand(val_o.shape, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    bg = capi.interpolation_matrix_backward(dev(gv), dev(case.vi), dev(case.idx), dev(rows_o)).cpu()
    bg_o = O.interpolation_matrix_backward(gv, case.vi, case.idx, bary, rows_o)
    fg = case.idx >= 0
    corner = P.pixel_keys(case)[fg]                                    # [R,3] vertex ids, rows in row_pixels' order
    got3, ref3 = bg.permute(0, 2, 3, 1)[fg], bg_o.permute(0, 2, 3, 1)[fg]
    tie_px = (corner[:, 0] == corner[:, 1]) | (corner[:, 1] == corner[:, 2]) | (corner[:, 0] == corner[:, 2])
    assert th.equal(got3[~tie_px], ref3[~tie_px]), "bary gradient of pixels with three different vertices"
    assert _row_multisets(corner[tie_px], got3[tie_px]) == _row_multisets(corner[tie_px], ref3[tie_px]), "bary gradient of pixels with a repeated vertex"
