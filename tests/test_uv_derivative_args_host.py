"""No GPU: what drtk_amd_screen_space_uv_derivative (drtk_amd/csrc/uv_derivative.hip) answers to bad arguments: every status
it can return before it touches the device.

Non-null pointers are made up.  Every call here stops in the argument check or returns early without a pixel: none can
reach a launch."""
import ctypes

OK, INVALID = 0, -1  # DRTK_OK, DRTK_ERR_INVALID_ARGUMENT
FAKE = 0x1000  # non-null, 16-byte aligned, never dereferenced
V, T, F = 5, 6, 7
ORDER = ("v", "vt", "vi", "vti", "index_img", "bary_img", "mask", "campos", "camrot", "focal", "out")
ALWAYS = ("index_img", "bary_img", "out", "campos", "camrot", "focal")  # required wherever there is a pixel
MESH = ("vi", "vti", "v", "vt")  # required where there is a pixel and a triangle
NULLS = {k: 0 for k in ORDER}


def _call(**over):
    from drtk_amd import capi

    a = dict(dtype=capi.DRTK_F32, N=2, V=V, T=T, F=F, v_sN=3 * V, vt_sN=2 * T, H=6, W=9)
    a.update({k: FAKE for k in ORDER})
    a.update(over)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    return capi.lib().drtk_amd_screen_space_uv_derivative(
        ctypes.c_int(a["dtype"]), p(a["v"]), i64(a["v_sN"]), p(a["vt"]), i64(a["vt_sN"]), p(a["vi"]), p(a["vti"]), p(a["index_img"]),
        p(a["bary_img"]), p(a["mask"]), p(a["campos"]), p(a["camrot"]), p(a["focal"]), i64(a["N"]), i64(a["V"]), i64(a["T"]),
        i64(a["F"]), i64(a["H"]), i64(a["W"]), p(a["out"]), p(0))


def test_bad_sizes_strides_and_dtype_are_invalid():
    bad = [dict(N=-1), dict(V=-1, v_sN=-3), dict(V=-1, v_sN=0), dict(T=-1, vt_sN=-2), dict(T=-1, vt_sN=0), dict(F=-1), dict(H=-1),
           dict(W=-1), dict(v_sN=1), dict(v_sN=3 * V + 1), dict(v_sN=-3 * V), dict(v_sN=2 * V), dict(V=0, v_sN=3),
           dict(vt_sN=1), dict(vt_sN=2 * T + 1), dict(vt_sN=-2 * T), dict(vt_sN=3 * T), dict(T=0, vt_sN=2),
           dict(H=1 << 16, W=1 << 15), dict(H=1, W=1 << 31),  # H W = 2^31
           dict(dtype=2), dict(dtype=-1), dict(dtype=7)]
    for over in bad:
        assert _call(**over) == INVALID, over
        # judged before the size of the batch and before any pointer
        assert _call(**{**NULLS, "N": 0, **over}) == INVALID, over
    # one below the limit passes the size test
    for hw in (dict(H=1, W=(1 << 31) - 1), dict(H=(1 << 16) - 1, W=1 << 15)):
        assert _call(N=0, **hw, **NULLS) == OK, hw
        assert _call(N=1, **hw, out=0) == INVALID, hw


def test_each_required_pointer_null_in_turn():
    for v_sN, vt_sN in ((3 * V, 2 * T), (0, 0)):  # per-view and shared vertices
        for k in ALWAYS + MESH:
            assert _call(v_sN=v_sN, vt_sN=vt_sN, **{k: 0}) == INVALID, k
    for k in ALWAYS:
        assert _call(F=0, **{k: 0}) == INVALID, k
        assert _call(F=0, vi=0, vti=0, v=0, vt=0, **{k: 0}) == INVALID, k
    # no pointer is looked at without a pixel
    for k in ORDER:
        for empty in (dict(N=0), dict(H=0), dict(W=0)):
            assert _call(**empty, **{k: 0}) == OK, (k, empty)
    assert _call(H=0, mask=0) == OK  # the mask is optional
    assert _call(H=0, F=0, vi=0, vti=0) == OK  # so are the triangles of an empty mesh


def test_nothing_to_do_is_ok_with_every_pointer_null():
    from drtk_amd import capi

    for dtype in (capi.DRTK_F32, capi.DRTK_F64):
        assert _call(dtype=dtype, N=0, **NULLS) == OK
        assert _call(dtype=dtype, H=0, **NULLS) == OK
        assert _call(dtype=dtype, W=0, v_sN=0, vt_sN=0, **NULLS) == OK
        assert _call(dtype=dtype, N=0, V=0, T=0, F=0, v_sN=0, vt_sN=0, H=0, W=0, **NULLS) == OK


def test_more_views_than_a_launch_takes():
    """The entry calls itself on slices of 65 535 views behind the whole argument check: the first slice's status is what the
    call returns."""
    for k in ALWAYS + MESH:
        assert _call(N=65536, **{k: 0}) == INVALID, k
    assert _call(N=65536, dtype=2) == INVALID
    assert _call(N=65536, vt_sN=1) == INVALID
    assert _call(N=65536, H=0, **NULLS) == OK
    assert _call(N=2 * 65535 + 1, W=0) == OK
