"""-m gpu: which kernel instantiation every interpolate call launches (drtk_amd/csrc/interpolate.hip) -- the FULL name with every
template argument, from the kernel timing report: the register scan's channel count, the wide kernel's <T, HAS_BARY, TABLE, CH,
ANYC>, the generic kernel's <T, HAS_VERT, HAS_BARY, CV, CHUNK>, the forward's <T, VEC, CV, PREFETCH, ANYW>, and the compaction
of padded rows.  tests/test_gpu_scatter_tables.py asserts the kernel and the table flag of a few shapes; this file pins the whole
routing rule, cell by cell, and checks every result against the oracle (that file's bounds) so that a kernel cannot pass by name.

The timing report names a launch by the text of its launch site, which may spell a template argument as a constant expression
over the element type (`sizeof(T)`) and the type's chunk (`CH`: 16 channels for float, 8 for double), and may leave defaulted
arguments out; `_instantiation` evaluates and completes them, so that the expected names below are plain values.  T stays T: the
element type is the call's.  (The macro dispatch this file was first run against spelled its sites that way; the launch helpers
that replaced it write the values out, and the expected names are the same for both.)

The expectations are those of the default environment, like the routes asserted in tests/test_gpu_scatter_tables.py: under
DRTK_CAPI_GUARD the binding hands out element-aligned outputs and passes no workspace, so the '+compact' cells take the table and
the forward's whole-quad cells the ANYW kernels -- a guarded run of this file fails there by construction, not by a fault."""
import re

import pytest
import torch as th

import scatter_table_cases as P
import test_gpu_scatter_tables as S

pytestmark = pytest.mark.gpu
dev = S.dev

NAMES = {"S": "interpolate_backward_small_kernel", "W": "interpolate_backward_wide_kernel", "G": "interpolate_backward_kernel",
         "F": "interpolate_kernel"}
FILL, COMPACT = "fill_bytes_kernel", "compact_rows_kernel<T>"  # attr_grad (or its padded workspace) is zeroed first
BOTH, ATTRIBUTES, BARY = (True, True), (True, False), (False, True)
REQUESTS = (BOTH, ATTRIBUTES, BARY)


def _expected(code, zero_fill=False):
    """'W true, false, 12, true +compact' -> the launch list."""
    kernel, _, args = code.partition(" ")
    args, plus, _ = args.partition(" +compact")
    return ([FILL] if zero_fill else []) + [f"{NAMES[kernel]}<T, {args}>"] + ([COMPACT] if plus else [])


def _value(text, itemsize):
    """A template argument as the launch site spells it -> its value, as text."""
    text = text.strip()
    while text.startswith("(") and text.endswith(")"):
        text = text[1:-1].strip()
    if "?" in text:
        cond, rest = text.split("?", 1)
        yes, no = rest.rsplit(":", 1)
        return _value(yes if _value(cond, itemsize) == "true" else no, itemsize)
    if text == "T":
        return text
    py = text.replace("sizeof(T)", str(itemsize)).replace("&&", " and ").replace("||", " or ")
    py = re.sub(r"\bCH\b", "16" if itemsize == 4 else "8", py)
    py = re.sub(r"\btrue\b", "True", re.sub(r"\bfalse\b", "False", py))
    assert re.fullmatch(r"[\w\s<>=!]+", py), text
    v = eval(py, {"__builtins__": {}})
    return {True: "true", False: "false"}.get(v, str(v)) if isinstance(v, bool) else str(v)


def _instantiation(site, itemsize):
    m = re.fullmatch(r"(\w+)<(.*)>", site)
    if not m:  # no template: the name is the instantiation
        assert re.fullmatch(r"\w+", site), site
        return site
    depth, args, cur = 0, [], ""
    for ch in m.group(2):
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            args.append(cur)
            cur = ""
        else:
            cur += ch
    args = [_value(a, itemsize) for a in args + [cur]]
    if m.group(1) == NAMES["F"]:
        args += ["false"] * (5 - len(args))  # PREFETCH and ANYW default to false
    return f"{m.group(1)}<{', '.join(args)}>"


def _launched(fn, dtype):
    out, names = S._kernels(fn)
    return out, [_instantiation(n, th.empty(0, dtype=dtype).element_size()) for n in names]


def _one_element_in(t):
    """The same values in a contiguous view that starts one element into a flat buffer: element-aligned only."""
    flat = th.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.flatten()
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) == t.element_size()
    return v


def test_the_launch_site_names_are_read_as_instantiations():
    assert _instantiation("interpolate_backward_wide_kernel<T, true, false, (sizeof(T) == 4 && true && true ? 12 : CH), true>", 4) == \
        "interpolate_backward_wide_kernel<T, true, false, 12, true>"
    assert _instantiation("interpolate_backward_wide_kernel<T, true, false, (sizeof(T) == 4 && true && true ? 12 : CH), true>", 8) == \
        "interpolate_backward_wide_kernel<T, true, false, 8, true>"
    assert _instantiation("interpolate_backward_wide_kernel<T, false, true, CH, false>", 4) == "interpolate_backward_wide_kernel<T, false, true, 16, false>"
    assert _instantiation("interpolate_backward_small_kernel<T, true, false, (5 <= 12 ? 5 : 1)>", 8) == "interpolate_backward_small_kernel<T, true, false, 5>"
    assert _instantiation("interpolate_kernel<T, 4, 1>", 4) == "interpolate_kernel<T, 4, 1, false, false>"
    assert _instantiation("interpolate_kernel<T, 4, 4, true, true>", 4) == "interpolate_kernel<T, 4, 4, true, true>"
    assert _instantiation("compact_rows_kernel<T>", 4) == COMPACT


# ---- backward ------------------------------------------------------------------------------------------------------------------
# C -> the launches of (both gradients, attributes only, bary only), default workspace; 16-byte aligned attributes
F32 = {
    1: ("S true, true, 1", "S true, false, 1", "S false, true, 1"),
    4: ("S true, true, 4", "S true, false, 4", "S false, true, 4"),
    5: ("S true, true, 5", "S true, false, 5", "S false, true, 5"),
    8: ("S true, true, 8", "S true, false, 8", "S false, true, 8"),
    10: ("S true, true, 10", "S true, false, 10", "S false, true, 10"),
    11: ("W true, false, 12, true +compact", "W false, true, 16, true", "S false, true, 11"),
    12: ("W true, false, 16, false +compact", "W false, true, 16, false", "S false, true, 12"),
    13: ("W true, false, 16, true +compact", "W false, true, 16, true", "G false, true, 1, 16"),
    16: ("W true, false, 16, false", "W false, false, 16, false", "G false, true, 4, 16"),
    17: ("W true, true, 16, true", "W false, true, 16, true", "G false, true, 1, 16"),
    20: ("W true, true, 16, false", "W false, true, 16, false", "G false, true, 4, 16"),
    24: ("W true, true, 16, false", "W false, true, 16, false", "G false, true, 4, 16"),
    37: ("W true, true, 16, true", "W false, true, 16, true", "G false, true, 1, 16"),
    64: ("W true, false, 16, false", "W false, false, 16, false", "G false, true, 4, 16"),
    100: ("W true, false, 16, false", "W false, false, 16, false", "G false, true, 4, 16"),
}
# ... and where workspace=False launches something else: the rows that were padded go through the workgroup's table
F32_NO_WORKSPACE = {11: {BOTH: "W true, true, 12, true"}, 12: {BOTH: "W true, true, 16, false"}, 13: {BOTH: "W true, true, 16, true"}}
# attributes one element into a flat buffer: no channel vectors (ANYC; the generic kernel's CV = 1), at 12 the chunk of 12
F32_ELEMENT_ALIGNED = {
    12: ("W true, false, 12, true +compact", "W false, true, 16, true", "S false, true, 12"),
    16: ("W true, false, 16, true", "W false, false, 16, true", "G false, true, 1, 16"),
    20: ("W true, true, 16, true", "W false, true, 16, true", "G false, true, 1, 16"),
}
F32_ELEMENT_ALIGNED_NO_WORKSPACE = {12: {BOTH: "W true, true, 12, true"}}
F64 = {
    4: ("S true, true, 4", "S true, false, 4", "S false, true, 4"),
    7: ("S true, true, 7", "S true, false, 7", "S false, true, 7"),
    8: ("W true, false, 8, false", "W false, false, 8, false", "S false, true, 8"),
    9: ("S true, true, 9", "S true, false, 9", "S false, true, 9"),
    11: ("S true, true, 11", "S true, false, 11", "S false, true, 11"),
    12: ("W true, true, 8, false", "W false, true, 8, false", "S false, true, 12"),
    13: ("W true, true, 8, true", "W false, true, 8, true", "G false, true, 1, 16"),
    16: ("W true, false, 8, false", "W false, false, 8, false", "G false, true, 4, 16"),
    20: ("W true, true, 8, false", "W false, true, 8, false", "G false, true, 4, 16"),
}
assert sorted(F32) == [1, 4, 5, 8, 10, 11, 12, 13, 16, 17, 20, 24, 37, 64, 100] and sorted(F64) == [4, 7, 8, 9, 11, 12, 13, 16, 20]

BACKWARD_CELLS = ([(th.float32, C, True, F32[C], F32_NO_WORKSPACE.get(C, {})) for C in F32] +
                  [(th.float32, C, False, F32_ELEMENT_ALIGNED[C], F32_ELEMENT_ALIGNED_NO_WORKSPACE.get(C, {})) for C in F32_ELEMENT_ALIGNED] +
                  [(th.float64, C, True, F64[C], None) for C in F64])


def _aligned_id(aligned):
    return "aligned" if aligned else "element-aligned"


@pytest.mark.parametrize("dtype,C,aligned,default,no_workspace", BACKWARD_CELLS,
                         ids=[f"{str(c[0]).replace('torch.', '')}-{c[1]}-{_aligned_id(c[2])}" for c in BACKWARD_CELLS])
def test_backward_instantiations(dtype, C, aligned, default, no_workspace):
    from drtk_amd import capi

    case = P.mixed(*P.DEFAULT)
    assert (case.N, case.H, case.W) == (2, 17, 130)
    attr, go = P.interp_inputs(case, C)
    r = P.interp_reference_cached(case, C)
    attrs = dev(attr.to(dtype)) if aligned else _one_element_in(dev(attr.to(dtype)))
    args = (dev(go.to(dtype)), attrs, dev(case.vi), dev(case.idx), dev(case.bary.to(dtype)))
    cells = [(req, None, code) for req, code in zip(REQUESTS, default)]
    if no_workspace is not None:  # (double never pads: one workspace setting)
        cells += [(req, False, no_workspace.get(req, code)) for req, code in zip(REQUESTS, default)]
    for (want_a, want_b), workspace, code in cells:
        what = f"interpolate backward C={C} {dtype} {'' if aligned else 'element-aligned '}workspace={workspace} request=({want_a}, {want_b})"
        (ag, bg), names = _launched(lambda: capi.interpolate_backward(*args, want_a, want_b, workspace=workspace), dtype)
        print(f"{what}: {names}")
        assert names == _expected(code, zero_fill=want_a), what
        assert (ag is None) == (not want_a) and (bg is None) == (not want_b)
        if want_a:
            S._vertex_gradient(ag, r["a32"], r["a64"], r["aA"], "interpolate", case, what)
        if want_b:
            bg = bg.detach().cpu()
            assert bool((bg[(case.idx == -1)[:, None].expand_as(bg)] == 0).all()), f"{what}: the bary gradient of the background is not exactly zero"
            if dtype == th.float64:
                S._f64_close(bg, r["b64"], what)
            else:
                assert float((bg - r["b32"]).abs().max()) <= 1e-6 * float(r["b32"].abs().max()), f"{what}: bary gradient"


# ---- forward -------------------------------------------------------------------------------------------------------------------
# (W, C, 16-byte aligned attributes) -> <VEC, CV, PREFETCH, ANYW> for float; double never prefetches
FORWARD = {
    (128, 16, True): "F 4, 4, true, false",
    (128, 4, True): "F 4, 4, false, false",
    (128, 5, True): "F 4, 1, false, false",
    (130, 16, True): "F 4, 4, true, true",
    (130, 5, True): "F 4, 1, false, true",
    (3, 8, True): "F 1, 4, false, false",
    (3, 5, True): "F 1, 1, false, false",
    (128, 16, False): "F 4, 1, false, false",
}


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("W,C,aligned", list(FORWARD), ids=lambda v: _aligned_id(v) if isinstance(v, bool) else str(v))
def test_forward_instantiations(W, C, aligned, dtype):
    import oracle as O
    from drtk_amd import capi

    case = P.mixed(17, W) if W >= 64 else P.per_pixel(17, W)
    attr = P.interp_inputs(case, C)[0].to(dtype)
    bary = case.bary.to(dtype)
    code = FORWARD[W, C, aligned]
    if dtype == th.float64:
        code = code.replace("4, 4, true", "4, 4, false")
    attrs = dev(attr) if aligned else _one_element_in(dev(attr))
    for masked in (False, True):
        out, names = _launched(lambda: capi.interpolate(attrs, dev(case.vi), dev(case.idx), dev(bary), masked=masked), dtype)
        print(f"interpolate W={W} C={C} {dtype} aligned={aligned} masked={masked}: {names}")
        assert names == _expected(code)
        ref = O.interpolate(attr, case.vi, case.idx, bary, nthreads=0)
        if masked:
            ref = ref * (case.idx != -1)[:, None]
        assert th.equal(out.cpu(), ref), "interpolate forward is not bit-identical"
