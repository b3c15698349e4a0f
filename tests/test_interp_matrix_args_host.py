"""No GPU: what the four C entry points of drtk_amd/csrc/interp_matrix.hip answer to bad arguments -- the CSR pair
(drtk_amd_interpolation_matrix, _matrix_backward) and the normal-matrix pair (drtk_amd_interpolation_normal_matrix_values,
_values_backward), each pair behind one argument check.  This file pins every status they can return before they touch the
device.

Non-null pointers are made up.  Every call here stops in the argument check or returns early with nothing to write: a call
that is accepted has no row (R = 0), no entry (nnz = 0) and no pixel, so that none can reach a zero fill or a launch."""
import ctypes

import pytest

OK, INVALID = 0, -1  # DRTK_OK, DRTK_ERR_INVALID_ARGUMENT
FAKE = 0x1000  # non-null, 16-byte aligned, never dereferenced
F = 7
ENTRIES = ("matrix", "matrix_backward", "normal", "normal_backward")
CSR = ENTRIES[:2]
POINTERS = {
    "matrix": ("vi", "index_img", "bary_img", "row_pixels", "col_indices", "values"),
    "matrix_backward": ("grad_values", "vi", "index_img", "row_pixels", "bary_grad"),
    "normal": ("pair_indices", "index_img", "bary_img", "values"),
    "normal_backward": ("grad_values", "pair_indices", "index_img", "bary_img", "bary_grad"),
}


def _call(entry, **over):
    from drtk_amd import capi

    a = dict(dtype=capi.DRTK_F32, N=2, F=F, H=6, W=9, R=11, nnz=13, sN=(3 if entry in CSR else 9) * F)
    a.update({k: FAKE for k in POINTERS[entry]})
    a.update(over)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    dt, L = ctypes.c_int(a["dtype"]), capi.lib()
    image = [i64(a[k]) for k in ("N", "F", "sN", "H", "W")]
    if entry == "matrix":
        return L.drtk_amd_interpolation_matrix(dt, p(a["vi"]), p(a["index_img"]), p(a["bary_img"]), p(a["row_pixels"]), i64(a["R"]),
                                               *image, p(a["col_indices"]), p(a["values"]), p(0))
    if entry == "matrix_backward":
        return L.drtk_amd_interpolation_matrix_backward(dt, p(a["grad_values"]), p(a["vi"]), p(a["index_img"]), p(a["row_pixels"]),
                                                        i64(a["R"]), *image, p(a["bary_grad"]), p(0))
    if entry == "normal":
        return L.drtk_amd_interpolation_normal_matrix_values(dt, p(a["pair_indices"]), p(a["index_img"]), p(a["bary_img"]), *image,
                                                             i64(a["nnz"]), p(a["values"]), p(0))
    return L.drtk_amd_interpolation_normal_matrix_values_backward(dt, p(a["grad_values"]), p(a["pair_indices"]), p(a["index_img"]),
                                                                  p(a["bary_img"]), *image, p(a["bary_grad"]), p(0))


def _idle(entry):
    """Nothing to do and every pointer null."""
    return dict(N=0, R=0, nnz=0, **{k: 0 for k in POINTERS[entry]})


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_sizes_and_strides_are_invalid(entry):
    per_view = (3 if entry in CSR else 9) * F
    bad = [dict(N=-1), dict(F=-1, sN=-per_view // F), dict(F=-1, sN=0), dict(H=-1), dict(W=-1),
           dict(sN=1), dict(sN=per_view + 1), dict(sN=-per_view), dict(sN=(9 if entry in CSR else 3) * F), dict(F=0, sN=per_view // F),
           dict(H=1 << 16, W=1 << 15), dict(H=1, W=1 << 31)]  # H W = 2^31
    bad.append(dict(R=-1) if entry in CSR else dict(nnz=-1) if entry == "normal" else dict(N=-2))
    for over in bad:
        assert _call(entry, **over) == INVALID, over
        assert _call(entry, **{**_idle(entry), **over}) == INVALID, over
    # one below the limit passes the size test
    for hw in (dict(H=1, W=(1 << 31) - 1), dict(H=(1 << 16) - 1, W=1 << 15)):
        assert _call(entry, **_idle(entry), **hw) == OK, hw


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_bad_dtype_is_invalid(entry):
    for dtype in (2, -1, 7):
        assert _call(entry, dtype=dtype) == INVALID
        assert _call(entry, dtype=dtype, **{k: 0 for k in POINTERS[entry]}) == INVALID
        if entry == "matrix":
            continue
        assert _call(entry, dtype=dtype, **_idle(entry)) == INVALID
        assert _call(entry, dtype=dtype, R=0, nnz=0, H=0) == INVALID


def test_a_bad_dtype_is_invalid_without_a_row_too():
    # entry-point refactor, intended change (a): drtk_amd_interpolation_matrix returned DRTK_OK for these before -- it looked
    # at dtype only behind `R == 0`, its three siblings in front of it
    for dtype in (2, -1, 7):
        assert _call("matrix", dtype=dtype, **_idle("matrix")) == INVALID
        assert _call("matrix", dtype=dtype, R=0) == INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_more_views_than_a_launch_takes(entry):
    """The two normal-matrix kernels take the view from blockIdx.y and sum into one values array: no slicing, 65 535 views at
    the most.  The CSR pair addresses rows, not views: any N."""
    if entry in CSR:
        assert _call(entry, **{**_idle(entry), "N": 65536, "H": 0}) == OK
        assert _call(entry, N=65536, vi=0, H=0) == INVALID
    else:
        assert _call(entry, N=65536) == INVALID
        assert _call(entry, **{**_idle(entry), "N": 65536}) == INVALID
        assert _call(entry, **{**_idle(entry), "N": 65535, "H": 0}) == OK


def test_matrix_requires_every_pointer_with_a_row():
    for k in POINTERS["matrix"]:
        assert _call("matrix", **{k: 0}) == INVALID, k
        assert _call("matrix", F=0, sN=0, **{k: 0}) == INVALID, k  # vi too: the kernel is not told F
        assert _call("matrix", R=0, **{k: 0}) == OK, k
    assert _call("matrix", R=0, N=0, H=0, F=0, sN=0, **{k: 0 for k in POINTERS["matrix"]}) == OK


def test_matrix_backward_pointers():
    # bary_grad is required (and cleared) wherever there is a pixel, rows or not
    assert _call("matrix_backward", bary_grad=0) == INVALID
    assert _call("matrix_backward", bary_grad=0, R=0) == INVALID
    assert _call("matrix_backward", bary_grad=0, R=0, grad_values=0, vi=0, index_img=0, row_pixels=0) == INVALID
    # the others wherever there is a row; without a pixel there is nothing to clear in front of them
    for k in ("grad_values", "vi", "index_img", "row_pixels"):
        for empty in (dict(N=0), dict(H=0), dict(W=0)):
            assert _call("matrix_backward", **empty, **{k: 0}) == INVALID, (k, empty)
            assert _call("matrix_backward", **empty, bary_grad=0, **{k: 0}) == INVALID, (k, empty)
            assert _call("matrix_backward", **empty, R=0, **{k: 0}) == OK, (k, empty)
    assert _call("matrix_backward", H=0, R=0, bary_grad=0) == OK
    assert _call("matrix_backward", **_idle("matrix_backward")) == OK


def test_normal_matrix_values_pointers():
    # values is required (and cleared) wherever there is an entry, pixels or not
    assert _call("normal", values=0) == INVALID
    assert _call("normal", values=0, H=0) == INVALID
    assert _call("normal", values=0, N=0, pair_indices=0, index_img=0, bary_img=0) == INVALID
    # no entry: nothing to clear, nothing to add, no pointer looked at
    for k in POINTERS["normal"]:
        assert _call("normal", nnz=0, **{k: 0}) == OK, k
    assert _call("normal", nnz=0, H=0, **{k: 0 for k in POINTERS["normal"]}) == OK
    assert _call("normal", **_idle("normal")) == OK


def test_normal_matrix_values_backward_pointers():
    for k in POINTERS["normal_backward"]:
        assert _call("normal_backward", **{k: 0}) == INVALID, k
    assert _call("normal_backward", F=0, sN=0, bary_grad=0) == INVALID  # cleared even with no triangle
    assert _call("normal_backward", F=0, sN=0, bary_grad=0, grad_values=0, pair_indices=0, index_img=0, bary_img=0) == INVALID
    # no pointer is looked at without a pixel
    for k in POINTERS["normal_backward"]:
        for empty in (dict(N=0), dict(H=0), dict(W=0)):
            assert _call("normal_backward", **empty, **{k: 0}) == OK, (k, empty)
    assert _call("normal_backward", **_idle("normal_backward")) == OK
