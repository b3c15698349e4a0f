"""No GPU: what drtk_amd_render and drtk_amd_render_backward (drtk_amd/csrc/render.hip) answer to bad arguments.  The two
entries share one argument check; this file pins every status either can return before it touches the device.

Non-null pointers are made up.  Every call here stops in the argument check or returns early with nothing to do: none has
a pixel (forward) or a pixel or a vertex (backward) unless it is rejected, so that none can reach a fill or a launch."""
import ctypes

import pytest

OK, INVALID = 0, -1  # DRTK_OK, DRTK_ERR_INVALID_ARGUMENT
FAKE = 0x1000  # non-null, 16-byte aligned, never dereferenced
F = 7
POINTERS = {0: ("v", "vi", "index_img", "depth_img", "bary_img"),
            1: ("v", "vi", "index_img", "grad_depth_img", "grad_bary_img", "grad_v")}


def _call(backward, **over):
    from drtk_amd import capi

    a = dict(dtype=capi.DRTK_F32, N=2, V=5, F=F, vi_sN=3 * F, H=6, W=9)
    a.update({k: FAKE for k in POINTERS[backward]})
    a.update(over)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    sizes = [i64(a[k]) for k in ("N", "V", "F", "vi_sN", "H", "W")]
    head = [ctypes.c_int(a["dtype"]), p(a["v"]), p(a["vi"]), p(a["index_img"])]
    if backward:
        return capi.lib().drtk_amd_render_backward(*head, p(a["grad_depth_img"]), p(a["grad_bary_img"]), *sizes, p(a["grad_v"]), p(0))
    return capi.lib().drtk_amd_render(*head, *sizes, p(a["depth_img"]), p(a["bary_img"]), p(0))


def _nulls(backward, **over):
    """One call with every pointer null -- so without a triangle, which would require `vi`."""
    return _call(backward, **{**{k: 0 for k in POINTERS[backward]}, "F": 0, "vi_sN": 0, **over})


@pytest.mark.parametrize("backward", [0, 1])
def test_bad_sizes_strides_and_dtype_are_invalid(backward):
    bad = [dict(N=-1), dict(V=-1), dict(F=-1, vi_sN=-3), dict(F=-1, vi_sN=0), dict(H=-1), dict(W=-1),
           dict(vi_sN=1), dict(vi_sN=3 * F + 1), dict(vi_sN=-3 * F), dict(F=0, vi_sN=3),
           dict(H=1 << 16, W=1 << 15), dict(H=1, W=1 << 31),  # H W = 2^31
           dict(dtype=2), dict(dtype=-1), dict(dtype=7)]
    for over in bad:
        assert _call(backward, **over) == INVALID, over
        # ... also with nothing to do and every pointer null
        assert _nulls(backward, **{"N": 0, **over}) == INVALID, over
    # one below the limit passes the size test
    for hw in (dict(H=1, W=(1 << 31) - 1), dict(H=(1 << 16) - 1, W=1 << 15)):
        assert _nulls(backward, N=0, **hw) == OK, hw
        assert _call(backward, N=1, **hw, index_img=0) == INVALID, hw


@pytest.mark.parametrize("backward", [0, 1])
def test_each_required_pointer_null_in_turn(backward):
    for k in POINTERS[backward]:
        assert _call(backward, **{k: 0}) == INVALID, k
    # the images are required only where there is a pixel, the vertices and the triangles also without one
    images = {k: 0 for k in POINTERS[backward] if k.endswith("_img")}
    assert _call(backward, H=0, V=0, **images, **({"grad_v": 0} if backward else {})) == OK
    assert _call(backward, W=0, V=0, v=0, **images, **({"grad_v": 0} if backward else {})) == OK
    assert _call(backward, H=0, v=0) == INVALID
    assert _call(backward, H=0, vi=0) == INVALID
    assert _call(backward, H=0, V=0, vi=0, F=0, vi_sN=0, **({"grad_v": 0} if backward else {})) == OK  # vi is optional with F = 0
    if backward:
        # grad_v is required as soon as there is a vertex, pixels or not
        assert _call(1, H=0, grad_v=0) == INVALID
        assert _call(1, W=0, grad_v=0, **images) == INVALID
        assert _call(1, H=0, V=0, grad_v=0, v=0) == OK
    else:
        assert _call(0, H=0, V=0, v=0) == OK


@pytest.mark.parametrize("backward", [0, 1])
def test_nothing_to_do_is_ok_with_every_pointer_null(backward):
    from drtk_amd import capi

    for dtype in (capi.DRTK_F32, capi.DRTK_F64):
        assert _nulls(backward, dtype=dtype, N=0) == OK
        assert _nulls(backward, dtype=dtype, N=0, V=0, H=0, W=0) == OK
        assert _nulls(backward, dtype=dtype, V=0, H=0) == OK


@pytest.mark.parametrize("backward", [0, 1])
def test_more_views_than_a_launch_takes(backward):
    """Both entries call themselves on slices of 65 535 views behind the whole argument check: the first slice's status is
    what the call returns."""
    for k in POINTERS[backward]:
        assert _call(backward, N=65536, **{k: 0}) == INVALID, k
    assert _call(backward, N=65536, dtype=2) == INVALID
    assert _call(backward, N=65536, vi_sN=1) == INVALID
    assert _nulls(backward, N=65536, V=0, H=0) == OK
    assert _call(backward, N=2 * 65535 + 1, V=0, W=0, v=0, **({"grad_v": 0} if backward else {})) == OK
