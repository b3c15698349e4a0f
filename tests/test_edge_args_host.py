"""No GPU: what the two C entry points of the edge backward (drtk_amd/csrc/edge_grad.hip) answer to bad arguments, and their
workspace queries.  The two entries share one argument check and one size helper; this file pins every status either can
return before it touches the device, and which of two coinciding faults wins.

Every call here stops in the argument check or in the early return of an empty batch: each carries a workspace one byte
short of the query's answer unless it is rejected earlier, so that none can reach a launch."""
import ctypes

import pytest

OK, INVALID, TOO_SMALL = 0, -1, -2  # DRTK_OK, DRTK_ERR_INVALID_ARGUMENT, DRTK_ERR_WORKSPACE_TOO_SMALL
FAKE = 0x1000  # non-null, 16-byte aligned, never dereferenced

QUERIES = ("drtk_amd_edge_grad_backward_workspace_bytes", "drtk_amd_edge_grad_backward_fused_workspace_bytes")


def _query(name, dtype, N, H, W, null_bytes=False):
    from drtk_amd import capi

    out = ctypes.c_size_t(0)
    i64 = ctypes.c_int64
    st = getattr(capi.lib(), name)(ctypes.c_int(dtype), i64(N), i64(H), i64(W), ctypes.c_void_p(0) if null_bytes else ctypes.byref(out))
    return st, out.value


def _call(fused, **over):
    """One call with made-up pointers.  `short` = how far the workspace falls short of the query's answer."""
    from drtk_amd import capi

    F = 7
    a = dict(dtype=capi.DRTK_F32, v_pix=FAKE, img=FAKE, index_img=FAKE, vi=FAKE, bary_img=FAKE, grad_output=FAKE, N=2, V=5, C=3,
             F=F, vi_sN=3 * F, H=6, W=9, out=FAKE, workspace=FAKE, short=1)
    a.update(over)
    st, need = _query(QUERIES[fused], a["dtype"], a["N"], a["H"], a["W"])
    ws_bytes = a.get("workspace_bytes", need - a["short"] if st == OK else 0)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    head = [ctypes.c_int(a["dtype"]), p(a["v_pix"]), p(a["img"]), p(a["index_img"]), p(a["vi"])]
    if fused:
        head.append(p(a["bary_img"]))
    tail = [p(a["grad_output"]), i64(a["N"]), i64(a["V"]), i64(a["C"]), i64(a["F"]), i64(a["vi_sN"]), i64(a["H"]), i64(a["W"]),
            ctypes.c_double(1e4), p(a["out"]), p(a["workspace"]), ctypes.c_size_t(ws_bytes), p(0)]
    fn = capi.lib().drtk_amd_edge_grad_backward_fused if fused else capi.lib().drtk_amd_edge_grad_backward
    return fn(*head, *tail)


@pytest.mark.parametrize("fused", [0, 1])
def test_bad_sizes_dtype_and_workspace_alignment_are_invalid(fused):
    bad = [dict(N=-1), dict(V=-1), dict(C=-1), dict(F=-1, vi_sN=-3), dict(F=-1, vi_sN=0), dict(H=-1), dict(W=-1),
           dict(vi_sN=1), dict(vi_sN=3 * 7 + 1), dict(vi_sN=-21), dict(F=0, vi_sN=3),
           dict(H=1 << 16, W=1 << 15),  # H W = 2^31
           dict(dtype=2), dict(dtype=-1),
           dict(workspace=FAKE + 8), dict(workspace=FAKE + 4), dict(workspace=FAKE + 1)]
    for over in bad:
        assert _call(fused, **over) == INVALID, over
    # judged before any pointer and before the size of the batch: with nothing to do, with every pointer null
    nulls = dict(v_pix=0, img=0, index_img=0, vi=0, bary_img=0, grad_output=0, out=0)
    for over in (dict(V=-1), dict(vi_sN=1), dict(dtype=2), dict(H=1 << 16, W=1 << 15), dict(workspace=8)):
        assert _call(fused, N=0, **nulls, **over) == INVALID, over
    # one below the limit is a size like any other: it gets as far as the workspace
    assert _call(fused, H=(1 << 16) - 1, W=1 << 15, N=1) == TOO_SMALL


@pytest.mark.parametrize("fused", [0, 1])
def test_each_required_pointer_null_in_turn(fused):
    required = ["index_img", "workspace", "v_pix", "vi", "img", "grad_output", "bary_img" if fused else "out"]
    for k in required:
        assert _call(fused, **{k: 0}) == INVALID, k
    if fused:
        assert _call(1, out=0) == INVALID  # grad_v_pix, N V > 0
        assert _call(1, out=0, H=0) == INVALID  # ... also without a pixel
        assert _call(1, out=0, W=0, index_img=0, bary_img=0, workspace=0) == INVALID
    # a pointer is required only under its size condition: without it the call gets as far as the workspace
    assert _call(fused, v_pix=0, V=0) == TOO_SMALL
    assert _call(fused, vi=0, F=0, vi_sN=0) == TOO_SMALL
    assert _call(fused, img=0, grad_output=0, C=0) == TOO_SMALL
    assert _call(fused, img=0, C=0) == TOO_SMALL
    if fused:
        assert _call(1, out=0, V=0) == TOO_SMALL  # no vertex: nothing to write
        assert _call(1, out=0, v_pix=0, V=0) == TOO_SMALL
    else:
        # no pixel: nothing to write, nothing to read
        assert _call(0, out=0, index_img=0, workspace=0, v_pix=0, vi=0, img=0, grad_output=0, H=0) == OK
        assert _call(0, out=0, index_img=0, workspace=0, W=0) == OK
    # fused, no pixel and no vertex: nothing to clear either
    assert _call(1, out=0, index_img=0, bary_img=0, workspace=0, v_pix=0, vi=0, img=0, grad_output=0, V=0, H=0) == OK
    assert _call(1, out=0, index_img=0, bary_img=0, workspace=0, V=0, W=0) == OK


@pytest.mark.parametrize("fused", [0, 1])
def test_workspace_too_small_and_coinciding_faults(fused):
    from drtk_amd import capi

    assert _call(fused) == TOO_SMALL  # one byte short
    assert _call(fused, workspace_bytes=0) == TOO_SMALL
    assert _call(fused, dtype=capi.DRTK_F64) == TOO_SMALL
    assert _call(fused, dtype=capi.DRTK_F64, workspace_bytes=2 * 2 * 6 * 9 * 4) == TOO_SMALL  # the float size does not do for double
    # a bad argument beats the short workspace, the alignment included; sizes beat the alignment (both are INVALID)
    for over in (dict(N=-1), dict(dtype=2), dict(vi_sN=1), dict(workspace=FAKE + 8), dict(index_img=0), dict(v_pix=0), dict(vi=0),
                 dict(img=0), dict(grad_output=0), dict(workspace=0), dict(N=-1, workspace=FAKE + 8)):
        assert _call(fused, workspace_bytes=0, **over) == INVALID, over
    assert _call(fused, workspace_bytes=0, **{"bary_img" if fused else "out": 0}) == INVALID
    if fused:
        assert _call(1, workspace_bytes=0, out=0) == INVALID
    # an unaligned workspace is invalid even where no workspace is needed
    assert _call(fused, V=0, H=0, workspace=FAKE + 8) == INVALID


@pytest.mark.parametrize("fused", [0, 1])
def test_an_empty_batch_is_ok_whatever_the_pointers(fused):
    from drtk_amd import capi

    nulls = dict(v_pix=0, img=0, index_img=0, vi=0, bary_img=0, grad_output=0, out=0, workspace=0)
    for dtype in (capi.DRTK_F32, capi.DRTK_F64):
        assert _call(fused, N=0, dtype=dtype) == OK
        assert _call(fused, N=0, dtype=dtype, **nulls) == OK
        assert _call(fused, N=0, dtype=dtype, **nulls, workspace_bytes=0) == OK
        assert _call(fused, N=0, dtype=dtype, workspace_bytes=1 << 20) == OK
        for k in nulls:
            assert _call(fused, N=0, dtype=dtype, **{k: 0}) == OK, k
        assert _call(fused, N=0, dtype=dtype, V=0, C=0, F=0, vi_sN=0, H=0, W=0, **nulls) == OK


# (dtype, N, H, W)
SHAPES = [(0, 0, 0, 0), (0, 3, 0, 5), (0, 2, 7, 0), (1, 0, 4, 4), (0, 1, 1, 1), (0, 2, 6, 9), (1, 2, 6, 9), (0, 8, 2048, 2048),
          (1, 3, 253, 251), (0, 1, (1 << 16) - 1, 1 << 15)]


def test_the_two_workspace_queries_agree():
    assert len(SHAPES) >= 8
    for dtype, N, H, W in SHAPES:
        a, b = _query(QUERIES[0], dtype, N, H, W), _query(QUERIES[1], dtype, N, H, W)
        assert a == b, (dtype, N, H, W)
        # two planes of the element type; never an empty allocation
        assert a == (OK, 2 * N * H * W * (8 if dtype else 4) or 16), (dtype, N, H, W)


@pytest.mark.parametrize("name", QUERIES)
def test_the_workspace_queries_reject_bad_arguments(name):
    assert _query(name, 0, 2, 6, 9, null_bytes=True)[0] == INVALID
    assert _query(name, 0, 0, 0, 0, null_bytes=True)[0] == INVALID
    for dtype, N, H, W in ((0, -1, 6, 9), (0, 2, -1, 9), (0, 2, 6, -1), (1, -1, -1, -1), (2, 2, 6, 9), (-1, 2, 6, 9), (3, 0, 0, 0)):
        st, value = _query(name, dtype, N, H, W)
        assert st == INVALID, (dtype, N, H, W)
        assert value == 0  # nothing is written on failure
