"""No GPU: what drtk_amd_transform_pinhole and drtk_amd_transform_pinhole_backward (drtk_amd/csrc/transform.hip) answer to
bad arguments.  The two entries share one argument check; this file pins every status either can return before it touches
the device.

Non-null pointers are made up.  Every call here stops in the argument check or returns early with no vertex to transform:
none can reach a launch."""
import ctypes

import pytest

OK, INVALID = 0, -1  # DRTK_OK, DRTK_ERR_INVALID_ARGUMENT
FAKE = 0x1000  # non-null, 16-byte aligned, never dereferenced
V = 5
CAMERA = ("campos", "camrot", "focal", "princpt")
POINTERS = {0: ("v", *CAMERA, "v_pix", "v_cam"), 1: ("v", *CAMERA, "grad_v_pix", "grad_v")}
REQUIRED = {0: ("v", *CAMERA, "v_pix"), 1: POINTERS[1]}


def _call(backward, **over):
    from drtk_amd import capi

    a = dict(dtype=capi.DRTK_F32, N=2, V=V, v_sN=3 * V)
    a.update({k: FAKE for k in POINTERS[backward]})
    a.update(over)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    head = [ctypes.c_int(a["dtype"]), p(a["v"]), i64(a["v_sN"]), *(p(a[k]) for k in CAMERA)]
    if backward:
        return capi.lib().drtk_amd_transform_pinhole_backward(*head, p(a["grad_v_pix"]), i64(a["N"]), i64(a["V"]), p(a["grad_v"]), p(0))
    return capi.lib().drtk_amd_transform_pinhole(*head, i64(a["N"]), i64(a["V"]), p(a["v_pix"]), p(a["v_cam"]), p(0))


def _nulls(backward):
    return {k: 0 for k in POINTERS[backward]}


@pytest.mark.parametrize("backward", [0, 1])
def test_bad_sizes_strides_and_dtype_are_invalid(backward):
    bad = [dict(N=-1), dict(V=-1, v_sN=-3), dict(V=-1, v_sN=0), dict(V=1 << 31, v_sN=0), dict(V=1 << 31, v_sN=3 << 31),
           dict(v_sN=1), dict(v_sN=3 * V + 1), dict(v_sN=-3 * V), dict(V=0, v_sN=3),
           dict(dtype=2), dict(dtype=-1), dict(dtype=7)]
    for over in bad:
        assert _call(backward, **over) == INVALID, over
        # ... also with nothing to do and every pointer null
        assert _call(backward, **{**_nulls(backward), "N": 0, **over}) == INVALID, over
    # one below the limit on V passes the size test
    for v_sN in (0, 3 * ((1 << 31) - 1)):
        assert _call(backward, N=0, V=(1 << 31) - 1, v_sN=v_sN, **_nulls(backward)) == OK
        assert _call(backward, N=1, V=(1 << 31) - 1, v_sN=v_sN, v=0) == INVALID


@pytest.mark.parametrize("backward", [0, 1])
def test_each_required_pointer_null_in_turn(backward):
    for v_sN in (0, 3 * V):  # shared and per-view vertices
        for k in REQUIRED[backward]:
            assert _call(backward, v_sN=v_sN, **{k: 0}) == INVALID, k
    # required only where there is a vertex to transform
    for k in REQUIRED[backward]:
        assert _call(backward, N=0, **{k: 0}) == OK, k
        assert _call(backward, V=0, v_sN=0, **{k: 0}) == OK, k
    if not backward:
        assert _call(0, N=0, v_cam=0) == OK  # v_cam is optional
        assert _call(0, v_cam=0, v_pix=0) == INVALID


@pytest.mark.parametrize("backward", [0, 1])
def test_nothing_to_do_is_ok_with_every_pointer_null(backward):
    from drtk_amd import capi

    for dtype in (capi.DRTK_F32, capi.DRTK_F64):
        assert _call(backward, dtype=dtype, N=0, **_nulls(backward)) == OK
        assert _call(backward, dtype=dtype, N=0, v_sN=0, **_nulls(backward)) == OK
        assert _call(backward, dtype=dtype, V=0, v_sN=0, **_nulls(backward)) == OK
        assert _call(backward, dtype=dtype, N=0, V=0, v_sN=0, **_nulls(backward)) == OK


@pytest.mark.parametrize("backward", [0, 1])
def test_more_views_than_a_launch_takes(backward):
    """The forward slices any batch of more than 65 535 views, the backward only one with per-view vertices (shared vertices:
    one launch sums the views); either way behind the whole argument check, so the first slice's status is the call's."""
    for v_sN in (0, 3 * V):
        for k in REQUIRED[backward]:
            assert _call(backward, N=65536, v_sN=v_sN, **{k: 0}) == INVALID, k
        assert _call(backward, N=65536, v_sN=v_sN, dtype=2) == INVALID
    assert _call(backward, N=65536, v_sN=1) == INVALID
    assert _call(backward, N=65536, V=0, v_sN=0, **_nulls(backward)) == OK
    assert _call(backward, N=2 * 65535 + 1, V=0, v_sN=0) == OK
