"""No GPU: what the C entry points of the rasterizer (drtk_amd/csrc/rasterize.hip) answer to bad arguments.  drtk_amd_rasterize
and drtk_amd_rasterize_layers share one argument check (check_raster_args); this file pins every status they and the two
workspace queries return before they touch the device, and which of two coinciding faults wins:

    sizes -> workspace alignment -> V >= 2^28 (TOO_MANY_VERTICES) -> dtype -> vi_sN -> [view slices] -> limits -> null pointers,
    num_layers in front of all of them, WORKSPACE_TOO_SMALL behind all of them.

No call here reaches a device call.  A call with made-up pointers is always one that a check rejects or that returns
DRTK_ERR_WORKSPACE_TOO_SMALL from the size test in front of the first fill; the only accepted calls have N = 0 and EVERY pointer
null, and return from the line after that test."""
import ctypes

import pytest

OK, INVALID, TOO_SMALL, TOO_MANY_VERTICES = 0, -1, -2, -5  # include/drtk_amd.h
FAKE = 0x1000  # non-null, 16-byte aligned, never dereferenced
ENTRIES = ("rasterize", "wireframe", "layers")  # drtk_amd_rasterize with wireframe = 0 / 1, drtk_amd_rasterize_layers
BINNED = ("rasterize", "layers")
HUGE = 1 << 62  # a workspace size that no layout of this file exceeds


def _call(entry, **over):
    """One call with made-up pointers and a workspace of 0 bytes: with nothing else wrong it is TOO_SMALL."""
    from drtk_amd import capi

    F = 7
    a = dict(dtype=capi.DRTK_F32, v=FAKE, vi=FAKE, N=2, V=5, F=F, vi_sN=3 * F, H=6, W=9, K=3, depth=FAKE, index=FAKE, workspace=FAKE,
             workspace_bytes=0)
    a.update(over)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    head = [ctypes.c_int(a["dtype"]), p(a["v"]), p(a["vi"])] + [i64(a[k]) for k in ("N", "V", "F", "vi_sN", "H", "W")]
    tail = [p(a["depth"]), p(a["index"]), p(a["workspace"]), ctypes.c_size_t(a["workspace_bytes"]), p(0)]
    if entry == "layers":
        return capi.lib().drtk_amd_rasterize_layers(*head, ctypes.c_int(a["K"]), *tail)
    return capi.lib().drtk_amd_rasterize(*head, ctypes.c_int(1 if entry == "wireframe" else 0), *tail)


NULLS = dict(v=0, vi=0, depth=0, index=0, workspace=0)


def _empty(entry, **over):
    """What an accepted call looks like here: no views, every pointer null, any workspace size."""
    a = dict(NULLS, N=0, workspace_bytes=HUGE)
    a.update(over)
    assert a["N"] <= 0 and not any(a[k] for k in NULLS), over
    return _call(entry, **a)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_base_call_stops_at_the_workspace_size(entry):
    assert _call(entry) == TOO_SMALL
    assert _call(entry, workspace_bytes=255) == TOO_SMALL  # every layout is at least 256 bytes; 8 N H W for wireframe
    assert _call(entry, dtype=1) == TOO_SMALL
    assert _call(entry, vi_sN=0) == TOO_SMALL


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_sizes_dtype_stride_and_alignment_are_invalid(entry):
    bad = [dict(N=-1), dict(V=-1), dict(F=-1, vi_sN=-3), dict(F=-1, vi_sN=0), dict(H=0), dict(H=-1), dict(W=0), dict(W=-1),
           dict(dtype=2), dict(dtype=7), dict(dtype=-1),
           dict(vi_sN=1), dict(vi_sN=3 * 7 + 1), dict(vi_sN=-21), dict(vi_sN=7), dict(F=0, vi_sN=3),
           dict(workspace=FAKE + 1), dict(workspace=FAKE + 4), dict(workspace=FAKE + 8)]
    for over in bad:
        assert _call(entry, **over) == INVALID, over
        assert _call(entry, workspace_bytes=HUGE, **over) == INVALID, over
        if "workspace" not in over:  # judged before any pointer and before the size of the batch
            assert _empty(entry, **over) == INVALID, over
    assert _call(entry, H=1 << 20, W=1 << 20) == INVALID and _call(entry, H=1 << 20, W=1 << 20, workspace_bytes=HUGE) == INVALID
    assert _call(entry, N=1, H=1 << 20, W=1 << 20) == INVALID  # N H W = 2^40
    assert _call(entry, N=1, K=1, H=1 << 20, W=(1 << 20) - 1) == TOO_SMALL  # one row below it
    assert _call(entry, workspace=FAKE + 16) == TOO_SMALL
    assert _call(entry, V=0, F=0, vi_sN=0, v=0, vi=0) == TOO_SMALL  # no triangles: no vertices, no faces


def test_the_image_limit_counts_the_layers():
    at = dict(N=1, H=1 << 20, W=1 << 19)  # N H W = 2^39
    assert _call("layers", K=2, **at) == INVALID
    assert _call("layers", K=1, **at) == TOO_SMALL
    assert _call("rasterize", **at) == TOO_SMALL


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_limits_of_the_bins_hold_for_the_binned_calls_only(entry):
    want = INVALID if entry in BINNED else TOO_SMALL  # the wireframe mode has no bins: it goes on to its own workspace test
    for over in (dict(N=1, H=65535 * 32 + 1, W=1), dict(N=1, H=1, W=65535 * 32 + 1), dict(N=2, F=1 << 28, vi_sN=0),
                 dict(N=1, F=1 << 29, vi_sN=0), dict(N=1 << 15, F=1 << 14, vi_sN=0)):
        assert _call(entry, **over) == want, over
    for over in (dict(N=1, H=65535 * 32, W=1), dict(N=1, H=1, W=65535 * 32), dict(N=1, F=(1 << 29) - 1, vi_sN=0)):
        assert _call(entry, **over) == TOO_SMALL, over


def test_the_wireframe_modes_own_checks():
    # it takes its workspace test before its limit on F, and a null workspace is too small, not invalid
    assert _call("wireframe", workspace=0, workspace_bytes=HUGE) == TOO_SMALL
    assert _call("wireframe", workspace_bytes=8 * 2 * 6 * 9 - 1) == TOO_SMALL
    assert _call("wireframe", F=1 << 31, vi_sN=0, workspace_bytes=0) == TOO_SMALL
    assert _call("wireframe", F=1 << 31, vi_sN=0, workspace_bytes=8 * 2 * 6 * 9) == INVALID
    assert _call("wireframe", F=1 << 31, vi_sN=0, workspace_bytes=HUGE) == INVALID
    for entry in BINNED:
        assert _call(entry, workspace=0, workspace_bytes=HUGE) == INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_each_required_pointer_null_in_turn(entry):
    for k in ("v", "vi", "depth", "index"):
        assert _call(entry, **{k: 0}) == INVALID, k
        assert _call(entry, workspace_bytes=HUGE, **{k: 0}) == INVALID, k
    # a pointer is required only under its size condition
    assert _call(entry, F=0, vi_sN=0, v=0, vi=0) == TOO_SMALL
    assert _call(entry, F=0, vi_sN=0, V=0, v=0, vi=0) == TOO_SMALL
    assert _call(entry, V=0, v=0) == INVALID  # triangles need vertices
    assert _call(entry, N=0, depth=0, index=0, workspace=0, v=0, vi=0) == (OK if entry == "wireframe" else TOO_SMALL)


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_views(entry):
    """H W > 0 with N = 0 and valid sizes: the binned calls still ask for the (then smallest) workspace, the wireframe mode
    returns first."""
    assert _empty(entry) == OK
    assert _empty(entry, F=0, vi_sN=0, V=0) == OK
    assert _empty(entry, workspace_bytes=0) == (OK if entry == "wireframe" else TOO_SMALL)
    assert _empty(entry, workspace_bytes=255) == (OK if entry == "wireframe" else TOO_SMALL)
    if entry in BINNED:
        assert _call(entry, N=0, workspace_bytes=0) == TOO_SMALL  # the pointers are not looked at
    assert _empty(entry, dtype=7) == INVALID and _empty(entry, vi_sN=1) == INVALID and _empty(entry, H=0) == INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_too_many_vertices_and_what_it_coincides_with(entry):
    big = dict(V=1 << 28)
    assert _call(entry, **big) == TOO_MANY_VERTICES
    assert _call(entry, V=(1 << 28) - 1) == TOO_SMALL
    assert _call(entry, V=1 << 40) == TOO_MANY_VERTICES
    # in front of the dtype, the stride, the limits, the null pointers and the size of the workspace
    for over in (dict(dtype=7), dict(vi_sN=1), NULLS, dict(v=0), dict(depth=0), dict(H=1 << 20, W=1 << 20), dict(N=1, F=1 << 29, vi_sN=0),
                 dict(workspace_bytes=HUGE), dict(dtype=7, vi_sN=1, v=0), dict(N=0)):
        assert _call(entry, **dict(big, **over)) == TOO_MANY_VERTICES, over
    assert _empty(entry, **big) == TOO_MANY_VERTICES
    # behind the sizes and the alignment of the workspace
    for over in (dict(N=-1), dict(H=0), dict(W=-1), dict(F=-1), dict(workspace=FAKE + 8)):
        assert _call(entry, **dict(big, **over)) == INVALID, over


def test_num_layers_is_judged_first():
    for K in (0, 9, -1, 1 << 20):
        assert _call("layers", K=K) == INVALID, K
        assert _call("layers", K=K, V=1 << 28) == INVALID, K
        assert _call("layers", K=K, workspace_bytes=HUGE) == INVALID, K
        assert _empty("layers", K=K) == INVALID, K
    for K in (1, 8):
        assert _call("layers", K=K) == TOO_SMALL
        assert _call("layers", K=K, V=1 << 28) == TOO_MANY_VERTICES
        assert _empty("layers", K=K) == OK


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_invalid_argument_beats_a_workspace_that_is_too_small(entry):
    for over in (dict(N=-1), dict(dtype=7), dict(vi_sN=1), dict(v=0), dict(vi=0), dict(depth=0), dict(index=0), dict(workspace=FAKE + 8),
                 dict(H=1 << 20, W=1 << 20)):
        assert _call(entry, workspace_bytes=0, **over) == INVALID, over
    for entry_b in BINNED:
        assert _call(entry_b, workspace_bytes=0, workspace=0) == INVALID
        assert _call(entry_b, workspace_bytes=0, N=1, F=1 << 29, vi_sN=0) == INVALID
    # the size alone: one byte short of what the query says
    if entry in BINNED:
        need = _query(entry, 2, 7, 6, 9)[1]
        assert need >= 256 and _call(entry, workspace_bytes=need - 1) == TOO_SMALL


@pytest.mark.parametrize("entry", ENTRIES)
def test_more_views_than_a_launch_takes_are_judged_slice_by_slice(entry):
    """The entry points call themselves on slices of 65 535 views in front of the limits and the pointers: a batch whose N F
    is beyond the bins' limit as a whole and within it per slice is not invalid."""
    F = (1 << 29) // 70000 + 1
    assert 70000 * F >= 1 << 29 > 65535 * F
    assert _call(entry, N=70000, F=F, vi_sN=0) == TOO_SMALL
    assert _call(entry, N=65536) == TOO_SMALL
    assert _call(entry, N=65536, v=0) == INVALID  # found by the first slice
    assert _call(entry, N=65536, dtype=7) == INVALID and _call(entry, N=65536, V=1 << 28) == TOO_MANY_VERTICES
    F1 = (1 << 29) // 65535 + 1  # beyond the limit in the first slice, too
    assert _call(entry, N=65536, F=F1, vi_sN=0) == (INVALID if entry in BINNED else TOO_SMALL)


# ---- the workspace queries ----------------------------------------------------------------------------------------------------
def _query(entry, N, F, H, W, K=3, null_bytes=False, before=0):
    from drtk_amd import capi

    out = ctypes.c_size_t(before)
    i64 = ctypes.c_int64
    dst = ctypes.c_void_p(0) if null_bytes else ctypes.byref(out)
    if entry == "layers":
        st = capi.lib().drtk_amd_rasterize_layers_workspace_bytes(i64(N), i64(F), i64(H), i64(W), ctypes.c_int(K), dst)
    else:
        st = capi.lib().drtk_amd_rasterize_workspace_bytes(i64(N), i64(F), i64(H), i64(W), dst)
    return st, out.value


@pytest.mark.parametrize("entry", BINNED)
def test_the_workspace_queries(entry):
    assert _query(entry, 2, 7, 6, 9, null_bytes=True)[0] == INVALID
    for N, F, H, W in ((-1, 7, 6, 9), (2, -1, 6, 9), (2, 7, 0, 9), (2, 7, 6, 0), (2, 7, -1, 9), (2, 7, 6, -1)):
        assert _query(entry, N, F, H, W, before=12345) == (INVALID, 12345), (N, F, H, W)  # nothing is written on failure
    for N, F, H, W in ((2, 7, 6, 9), (0, 7, 6, 9), (2, 0, 6, 9), (0, 0, 1, 1), (8, 100000, 2048, 2048)):
        st, nbytes = _query(entry, N, F, H, W)
        assert st == OK and nbytes >= 256 and nbytes % 256 == 0, (N, F, H, W)
        assert nbytes == _query("rasterize", N, F, H, W)[1]  # the bins are shared by all layers
    if entry == "layers":
        for K in (0, 9, -1):
            assert _query(entry, 2, 7, 6, 9, K=K, before=12345) == (INVALID, 12345), K
        assert _query(entry, 2, 7, 6, 9, K=1)[1] == _query(entry, 2, 7, 6, 9, K=8)[1]
