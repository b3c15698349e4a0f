"""No GPU: what the C entry points of interpolate (drtk_amd/csrc/interpolate.hip) answer to bad arguments, and the workspace
query of the backward.  drtk_amd_interpolate, _interpolate_masked, _interpolate_backward and _interpolate_backward_ws share one
argument check; this file pins every status they can return before they touch the device, and which of two coinciding
faults wins.

No call here reaches a device call: a rejected one stops in the check, an accepted one has N V C == 0 and N H W == 0 and
returns before any fill or launch."""
import ctypes

import pytest

OK, INVALID = 0, -1  # DRTK_OK, DRTK_ERR_INVALID_ARGUMENT
FAKE = 0x1000  # non-null, 64-byte aligned, never dereferenced
ENTRIES = ("interpolate", "interpolate_masked", "interpolate_backward", "interpolate_backward_ws")
BACKWARD = ENTRIES[2:]


def _call(entry, **over):
    """One call with made-up pointers.  By default nothing is wrong with it and there is something to do (it is only ever
    sent with a fault); `empty=True` takes the vertices and the pixels away: V = 0 and H = 0."""
    from drtk_amd import capi

    F = 7
    a = dict(dtype=capi.DRTK_F32, grad_out=FAKE, attrs=FAKE, vi=FAKE, index_img=FAKE, bary_img=FAKE, N=2, V=5, C=3, F=F, vi_sN=3 * F,
             H=6, W=9, out=FAKE, attr_grad=FAKE, bary_grad=FAKE, workspace=0, workspace_bytes=0)
    if over.pop("empty", False):
        a.update(V=0, H=0)
    a.update(over)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    sizes = [i64(a[k]) for k in ("N", "V", "C", "F", "vi_sN", "H", "W")]
    head = [ctypes.c_int(a["dtype"])] + ([p(a["grad_out"])] if entry in BACKWARD else []) + [p(a[k]) for k in ("attrs", "vi", "index_img", "bary_img")]
    if entry in BACKWARD:
        tail = [p(a["attr_grad"]), p(a["bary_grad"])] + ([p(a["workspace"]), ctypes.c_size_t(a["workspace_bytes"])] if entry.endswith("_ws") else [])
    else:
        tail = [p(a["out"])]
    return getattr(capi.lib(), "drtk_amd_" + entry)(*head, *sizes, *tail, p(0))


def _accepted(entry, **over):
    """An accepted call must be an empty one, or it would go on to the device."""
    a = dict(N=2, V=0, C=3, H=0, W=9)
    a.update({k: v for k, v in over.items() if k in a})
    assert a["N"] * a["V"] * a["C"] == 0 and a["N"] * a["H"] * a["W"] == 0, over
    return _call(entry, empty=True, **over)


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_sizes_strides_and_limits_are_invalid(entry):
    bad = [dict(N=-1), dict(V=-1), dict(C=-1), dict(F=-1, vi_sN=-3), dict(F=-1, vi_sN=0), dict(H=-1), dict(W=-1),
           dict(C=1 << 20), dict(C=(1 << 20) + 1),
           dict(vi_sN=1), dict(vi_sN=3 * 7 + 1), dict(vi_sN=-21), dict(vi_sN=7), dict(F=0, vi_sN=3),
           dict(H=1 << 16, W=1 << 15), dict(H=1 << 31, W=1), dict(H=1, W=1 << 31)]  # H W = 2^31
    nulls = dict(grad_out=0, attrs=0, vi=0, index_img=0, bary_img=0, out=0)
    for over in bad:
        assert _call(entry, **over) == INVALID, over
        # judged before any pointer and before the size of the batch: with nothing to do, with every input pointer null
        assert _call(entry, **dict(dict(N=0, **nulls), **over)) == INVALID, over
    # one below each limit is a size like any other (no views: nothing to do)
    for over in (dict(C=(1 << 20) - 1), dict(H=(1 << 16) - 1, W=1 << 15), dict(H=(1 << 31) - 1, W=1), dict(vi_sN=0), dict(F=0, vi_sN=0, vi=0),
                 dict(V=0), dict(C=0), dict(H=0), dict(W=0)):
        assert _accepted(entry, N=0, **over) == OK, over


@pytest.mark.parametrize("entry", ENTRIES)
def test_each_required_pointer_null_in_turn(entry):
    required = ["attrs", "vi", "index_img", "bary_img"] + (["grad_out"] if entry in BACKWARD else ["out"])
    for k in required:
        assert _call(entry, **{k: 0}) == INVALID, k
    # a pointer is required only under its size condition
    assert _accepted(entry, attrs=0) == OK  # V = 0: no attribute
    assert _accepted(entry, index_img=0, bary_img=0, grad_out=0, out=0) == OK  # H = 0: no pixel
    assert _accepted(entry, vi=0, F=0, vi_sN=0) == OK
    assert _accepted(entry, vi=0) == INVALID  # F > 0 asks for the faces whatever else is empty
    assert _accepted(entry, attrs=0, index_img=0, bary_img=0, grad_out=0, out=0, vi=0, F=0, vi_sN=0) == OK
    assert _call(entry, attrs=0, C=0, index_img=0, bary_img=0, grad_out=0, out=0, N=0) == OK
    # vertices without pixels still need their attributes, pixels without vertices their images
    assert _call(entry, H=0, attrs=0) == INVALID
    assert _call(entry, V=0, index_img=0) == INVALID
    assert _call(entry, V=0, bary_img=0) == INVALID
    assert _call(entry, V=0, **{"grad_out" if entry in BACKWARD else "out": 0}) == INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_bad_dtype_is_invalid_also_for_an_empty_batch(entry):
    for dtype in (2, 7, -1):
        assert _call(entry, dtype=dtype) == INVALID
        assert _accepted(entry, dtype=dtype) == INVALID
        assert _accepted(entry, dtype=dtype, N=0) == INVALID
    assert _accepted(entry, dtype=1) == OK and _accepted(entry, dtype=0) == OK


def test_a_misaligned_workspace_is_invalid():
    ws = "interpolate_backward_ws"
    for off in (1, 4, 8, 16, 32, 48):
        assert _call(ws, workspace=FAKE + off, workspace_bytes=1 << 20) == INVALID, off
        assert _accepted(ws, workspace=FAKE + off, workspace_bytes=1 << 20) == INVALID, off
        assert _accepted(ws, workspace=FAKE + off, workspace_bytes=0, N=0) == INVALID, off
    for nbytes in (0, 1, 1 << 20):  # absent, aligned, of any size: all accepted
        assert _accepted(ws, workspace=FAKE, workspace_bytes=nbytes) == OK
        assert _accepted(ws, workspace=FAKE + 64, workspace_bytes=nbytes) == OK
        assert _accepted(ws, workspace=0, workspace_bytes=nbytes) == OK


@pytest.mark.parametrize("entry", BACKWARD)
def test_nothing_requested_in_both_of_its_outcomes(entry):
    none = dict(attr_grad=0, bary_grad=0)
    # both gradients would have had elements: an error
    assert _call(entry, **none) == INVALID
    # an output that is null because it is empty was not forgotten: nothing to write
    assert _call(entry, V=0, **none) == OK
    assert _call(entry, H=0, **none) == OK
    assert _call(entry, W=0, **none) == OK
    assert _call(entry, C=0, **none) == OK
    assert _call(entry, N=0, **none) == OK
    assert _accepted(entry, **none) == OK
    # one gradient requested is a request
    assert _accepted(entry, attr_grad=0) == OK and _accepted(entry, bary_grad=0) == OK


@pytest.mark.parametrize("entry", BACKWARD)
def test_coinciding_faults_in_the_backward(entry):
    none = dict(attr_grad=0, bary_grad=0)
    # a bad size beats "nothing requested, nothing to write"
    for over in (dict(N=-1), dict(C=1 << 20), dict(vi_sN=1), dict(H=1 << 16, W=1 << 15)):
        assert _call(entry, V=0, **dict(none, **over)) == INVALID, over
    # "nothing requested, nothing to write" is answered before the pointers, the dtype and the workspace are looked at
    for over in (dict(grad_out=0), dict(index_img=0), dict(bary_img=0), dict(attrs=0), dict(vi=0), dict(dtype=7), dict(workspace=FAKE + 8),
                 dict(dtype=7, workspace=FAKE + 8, vi=0)):
        assert _call(entry, V=0, **dict(none, **over)) == OK, over
        assert _call(entry, H=0, **dict(none, **over)) == OK, over
    # ... and so is its error
    assert _call(entry, dtype=7, **none) == INVALID
    # with a request: null pointers, the dtype and the alignment are all invalid, alone or together
    for over in (dict(vi=0, dtype=7), dict(dtype=7, workspace=FAKE + 8), dict(attrs=0, workspace=FAKE + 8), dict(grad_out=0, dtype=7)):
        assert _call(entry, **over) == INVALID, over


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_coinciding_faults_in_the_forward(entry):
    # an empty batch does not excuse a bad size, a bad dtype or missing faces
    for over in (dict(N=-1), dict(vi_sN=1), dict(dtype=7), dict(vi=0), dict(dtype=7, vi=0), dict(N=-1, dtype=7)):
        assert _accepted(entry, **over) == INVALID, over
    # null images are no fault where there is no pixel, whatever the dtype says afterwards
    assert _accepted(entry, index_img=0, bary_img=0, out=0, dtype=7) == INVALID
    assert _accepted(entry, index_img=0, bary_img=0, out=0, dtype=1) == OK


# ---- drtk_amd_interpolate_backward_workspace_bytes ---------------------------------------------------------------------------
def _query(dtype, N, V, C, null_bytes=False, before=0):
    from drtk_amd import capi

    out = ctypes.c_size_t(before)
    i64 = ctypes.c_int64
    st = capi.lib().drtk_amd_interpolate_backward_workspace_bytes(ctypes.c_int(dtype), i64(N), i64(V), i64(C),
                                                                  ctypes.c_void_p(0) if null_bytes else ctypes.byref(out))
    return st, out.value


def _rule(dtype, N, V, C):
    """The rule, once: float rows of 11 ... 15 channels are accumulated in a workspace whose rows are padded to whole 64-byte
    segments -- C rounded up to 16 floats --; nothing else takes a workspace, and no vertex means no workspace."""
    if dtype != 0 or not 11 <= C <= 15 or N * V == 0:
        return 0
    pitch = -(-C // 16) * 16
    return 4 * N * V * pitch


def test_workspace_bytes_for_every_channel_count():
    for dtype in (0, 1):
        for C in range(0, 71):
            for N, V in ((8, 1000), (1, 1), (3, 7), (0, 1000), (8, 0), (0, 0)):
                assert _query(dtype, N, V, C, before=12345) == (OK, _rule(dtype, N, V, C)), (dtype, N, V, C)
    nonzero = {(dtype, C) for dtype in (0, 1) for C in range(0, 71) if _query(dtype, 2, 5, C)[1] != 0}
    assert nonzero == {(0, C) for C in (11, 12, 13, 14, 15)}
    for C in (11, 12, 13, 14, 15):  # the padded pitch: C rounded up to 16 floats
        assert _query(0, 2, 5, C)[1] == 2 * 5 * 16 * 4


def test_the_workspace_query_rejects_bad_arguments():
    assert _query(0, 2, 5, 13, null_bytes=True)[0] == INVALID
    assert _query(0, 0, 0, 0, null_bytes=True)[0] == INVALID
    for dtype, N, V, C in ((0, -1, 5, 13), (0, 2, -1, 13), (0, 2, 5, -1), (1, -1, -1, -1), (2, 2, 5, 13), (-1, 2, 5, 13), (7, 0, 0, 0)):
        st, value = _query(dtype, N, V, C, before=12345)
        assert st == INVALID, (dtype, N, V, C)
        assert value == 12345  # nothing is written on failure
