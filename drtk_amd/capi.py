"""ctypes binding of the C ABI (include/drtk_amd.h) on torch device tensors.

This is the same entry-point set the torch-op shim uses, callable without the dispatcher: parity
tests and the benchmark's per-kernel timing go through here.  Tensors must live on a HIP device;
every call enqueues on the given stream (default: torch's current stream) and returns new
output tensors.  There is no CPU path.
"""
import ctypes
import os
from typing import Optional, Tuple

import torch as th

from drtk_amd.utils import native_library_paths

_lib = None

DRTK_F32, DRTK_F64, DRTK_F16 = 0, 1, 2  # DRTK_F16: filter2d only


_lib_path = None

_POISON = os.environ.get("DRTK_CAPI_POISON", "") not in ("", "0")


# DRTK_CAPI_GUARD=g (tests): every output / workspace of this binding is carved out of a larger flat allocation with g
# sentinel elements on either side (16 g bytes for byte workspaces, which must stay 16-byte aligned) -- so outputs are
# only element-aligned (g = 1, 2, 3), and `check_guards()` tells whether a kernel wrote outside what it was given.
_GUARD = int(os.environ.get("DRTK_CAPI_GUARD", "0") or 0)
_guards = []


def _sentinel(dtype):
    return 0x5A if dtype == th.uint8 else (-7.25 if dtype.is_floating_point else -(2 ** 29) - 3)


def _out(*shape, dtype, device):
    """Output / workspace allocation of this binding: uninitialised memory -- or, with DRTK_CAPI_POISON=1 in the
    environment (the fuzzers and the GPU suite set it), memory pre-filled with NaN / a large negative integer / 0xA5
    bytes, so that an element a kernel forgot to write cannot pass for a value (freshly allocated device memory reads as
    zeros, which is a plausible image; see profiles/NOTES.md 3.1, round 3)."""
    if _GUARD:
        n = 1
        for d in shape:
            n *= int(d)
        g = _GUARD * (16 if dtype == th.uint8 else 1)
        flat = th.full((n + 2 * g,), _sentinel(dtype), dtype=dtype, device=device)
        _guards.append((flat, g, n))
        t = flat[g:g + n].view(*shape)
    else:
        t = th.empty(*shape, dtype=dtype, device=device)
    if _POISON and t.numel():
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        elif t.dtype == th.uint8:
            t.fill_(0xA5)
        else:
            t.fill_(-(2 ** 30) - 7)
    return t


def check_guards() -> int:
    """DRTK_CAPI_GUARD: assert that the sentinel elements around every output and workspace handed out since the last
    call are intact (synchronises); returns how many allocations were checked.  Without the variable: 0."""
    th.cuda.synchronize()
    k = len(_guards)
    for flat, g, n in _guards:
        s = _sentinel(flat.dtype)
        ok = bool((flat[:g] == s).all()) and bool((flat[g + n:] == s).all())
        if not ok:
            _guards.clear()
            raise AssertionError(f"a kernel wrote outside a {flat.dtype} output / workspace of {n} elements")
    _guards.clear()
    return k



def use_profiling_library(path: str) -> None:
    """profiles/kernel_bench.py --flags only: bind this module to the ablation build of the same sources
    (profiles/libdrtk_amd_ablate.so, `python drtk_amd/build.py --ablation`) instead of the product library.
    Must be called before the first C-ABI call of the process."""
    global _lib_path
    assert _lib is None, "the C-ABI library is already loaded"
    _lib_path = path


DEPTH_ORDERS = {"strict": 0, "fastmath": 1}  # drtk_depth_order_t


def use_depth_order(order: str) -> None:
    """The rasterizer's depth-order setting (include/drtk_amd.h: drtk_amd_set_depth_order): `"fastmath"` evaluates the
    depth sum in the order of the reference AS BUILT by its setup.py (`-O3 --fast-math`), `"strict"` (the default) in the
    order its source spells.  One setting per process and library -- the torch operators call the same library and
    follow it; DRTK_AMD_DEPTH_ORDER=fastmath in the environment sets the initial value.  Affects later launches.
    A captured graph replays the order that was active at capture, not the one set when it is replayed.  The setting is
    process-wide: every thread and stream that uses the library shares it."""
    assert order in DEPTH_ORDERS, order
    _check(lib().drtk_amd_set_depth_order(DEPTH_ORDERS[order]), "set_depth_order")


def depth_order() -> str:
    o = lib().drtk_amd_get_depth_order()
    return next(k for k, v in DEPTH_ORDERS.items() if v == o)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        path = _lib_path or native_library_paths()[0]
        if not os.path.isfile(path):
            build_py = os.path.join(os.path.dirname(os.path.abspath(__file__)), "build.py")
            raise ImportError(f"{path} is missing: run `python {build_py}`")
        L = ctypes.CDLL(path)
        L.drtk_amd_status_string.restype = ctypes.c_char_p
        L.drtk_amd_status_string.argtypes = [ctypes.c_int]
        L.drtk_amd_version.restype = ctypes.c_char_p
        for name in EXPORTS:
            if name not in ("drtk_amd_status_string", "drtk_amd_version"):
                getattr(L, name).restype = ctypes.c_int
        _lib = L
    return _lib


EXPORTS = [
    "drtk_amd_status_string",
    "drtk_amd_version",
    "drtk_amd_set_depth_order",
    "drtk_amd_get_depth_order",
    "drtk_amd_rasterize_workspace_bytes",
    "drtk_amd_rasterize_lines_workspace_bytes",
    "drtk_amd_rasterize",
    "drtk_amd_rasterize_layers_workspace_bytes",
    "drtk_amd_rasterize_layers",
    "drtk_amd_render",
    "drtk_amd_render_backward",
    "drtk_amd_interpolate",
    "drtk_amd_interpolate_masked",
    "drtk_amd_interpolate_backward",
    "drtk_amd_interpolate_backward_workspace_bytes",
    "drtk_amd_interpolate_backward_ws",
    "drtk_amd_edge_grad_backward_workspace_bytes",
    "drtk_amd_edge_grad_backward",
    "drtk_amd_edge_grad_backward_fused_workspace_bytes",
    "drtk_amd_edge_grad_backward_fused",
    "drtk_amd_interpolation_matrix",
    "drtk_amd_interpolation_matrix_backward",
    "drtk_amd_interpolation_normal_matrix_values",
    "drtk_amd_interpolation_normal_matrix_values_backward",
    "drtk_amd_mipmap_grid_sampler_2d",
    "drtk_amd_mipmap_grid_sampler_2d_backward",
    "drtk_amd_grid_scatter_2d",
    "drtk_amd_grid_scatter_2d_backward",
    "drtk_amd_msi_forward",
    "drtk_amd_msi_backward",
    "drtk_amd_composite_layers",
    "drtk_amd_composite_layers_backward",
    "drtk_amd_mipmap_pyramid",
    "drtk_amd_mipmap_pyramid_backward",
    "drtk_amd_image_loss_workspace_bytes",
    "drtk_amd_image_loss_forward",
    "drtk_amd_image_loss_backward",
    "drtk_amd_shade_workspace_bytes",
    "drtk_amd_shade_forward",
    "drtk_amd_shade_backward",
    "drtk_amd_filter2d_output_size",
    "drtk_amd_filter2d",
    "drtk_amd_screen_space_uv_derivative",
    "drtk_amd_transform_pinhole",
    "drtk_amd_transform_pinhole_backward",
    "drtk_amd_transform_distort",
    "drtk_amd_transform_distort_backward",
    "drtk_amd_geometry_face_forward",
    "drtk_amd_geometry_face_backward",
    "drtk_amd_geometry_face_gather",
    "drtk_amd_geometry_vertex_gather_workspace_bytes",
    "drtk_amd_geometry_vertex_gather",
    "drtk_amd_geometry_cot_weights",
    "drtk_amd_geometry_cot_weights_backward",
    "drtk_amd_geometry_laplacian_workspace_bytes",
    "drtk_amd_geometry_laplacian",
    "drtk_amd_geometry_laplacian_grad_weights",
    "drtk_amd_skin_forward",
    "drtk_amd_skin_backward_workspace_bytes",
    "drtk_amd_skin_backward",
    "drtk_amd_kinematics_forward",
    "drtk_amd_kinematics_backward_workspace_bytes",
    "drtk_amd_kinematics_backward",
    "drtk_amd_nearest_forward_workspace_bytes",
    "drtk_amd_nearest_forward",
    "drtk_amd_nearest_backward_workspace_bytes",
    "drtk_amd_nearest_backward",
    "drtk_amd_selftest_exact_div",
    "drtk_amd_kernel_timing_begin",
    "drtk_amd_kernel_timing_report",
]


class DrtkAmdError(RuntimeError):
    pass


def _check(status: int, what: str):
    if status != 0:
        raise DrtkAmdError(f"{what}: {lib().drtk_amd_status_string(status).decode()} (status {status})")


def _dt(t: th.Tensor) -> int:
    if t.dtype == th.float32:
        return DRTK_F32
    if t.dtype == th.float64:
        return DRTK_F64
    raise TypeError(f"drtk_amd: unsupported dtype {t.dtype}")


def _p(t: Optional[th.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _i(x) -> ctypes.c_int64:
    return ctypes.c_int64(int(x))


def _on_tensor_device(fn):
    """Runs `fn` with the device of its first tensor argument made current.  The library sizes its grids from, and
    launches on, hipGetDevice() -- the torch-op shim installs a device guard for that, this is the same guard for
    ctypes callers: tensors on cuda:1 while cuda:0 is current would otherwise be launched against the wrong device.
    Tensors of one call that live on different devices are an error."""
    import functools

    def tensors(args):
        for a in args:
            if isinstance(a, th.Tensor):
                yield a
            elif isinstance(a, (list, tuple)):
                yield from (x for x in a if isinstance(x, th.Tensor))

    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        ts = list(tensors(list(args) + list(kwargs.values())))
        if not ts:
            return fn(*args, **kwargs)
        if not ts[0].is_cuda:
            raise DrtkAmdError("drtk_amd implements the MI355X (HIP) path only; got a CPU tensor")
        devs = {t.device for t in ts}
        if len(devs) != 1:
            raise DrtkAmdError(f"drtk_amd: tensors of one call on different devices: {sorted(map(str, devs))}")
        with th.cuda.device(ts[0].device):
            return fn(*args, **kwargs)

    return guarded


def _stream(t: th.Tensor, stream) -> ctypes.c_void_p:
    if not t.is_cuda:
        raise DrtkAmdError("drtk_amd implements the MI355X (HIP) path only; got a CPU tensor")
    s = th.cuda.current_stream(t.device) if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


def _vi(vi: th.Tensor, n: int):
    assert vi.dtype == th.int32
    if vi.ndim == 2:
        c = vi.contiguous()
        return c, 0, c.shape[0]
    if vi.shape[0] > 1 and vi.stride(0) == 0:
        c = vi[0].contiguous()
        return c, 0, c.shape[0]
    c = vi.contiguous()
    return c, c.shape[1] * 3, c.shape[1]


def rasterize_workspace_bytes(N, F, H, W) -> int:
    out = ctypes.c_size_t(0)
    _check(lib().drtk_amd_rasterize_workspace_bytes(_i(N), _i(F), _i(H), _i(W), ctypes.byref(out)), "rasterize")
    return out.value


def rasterize_lines_workspace_bytes(N, H, W) -> int:
    out = ctypes.c_size_t(0)
    _check(lib().drtk_amd_rasterize_lines_workspace_bytes(_i(N), _i(H), _i(W), ctypes.byref(out)), "rasterize")
    return out.value


@_on_tensor_device
def rasterize(v, vi, height, width, stream=None, workspace=None, wireframe=False, out=None) -> Tuple[th.Tensor, th.Tensor]:
    """`out` = (depth_img, index_img) to write into (contiguous [N,H,W] float32 / int32): tests pre-fill them with a
    sentinel to see that every pixel is written."""
    v = v.contiguous()
    N, V, _ = v.shape
    vi_c, vi_sN, F = _vi(vi, N)
    if out is not None:
        depth, index = out
        assert depth.shape == (N, height, width) and index.shape == (N, height, width) and depth.is_contiguous() and index.is_contiguous()
        assert depth.dtype == th.float32 and index.dtype == th.int32
    else:
        depth = _out(N, height, width, dtype=th.float32, device=v.device)
        index = _out(N, height, width, dtype=th.int32, device=v.device)
    nbytes = rasterize_lines_workspace_bytes(N, height, width) if wireframe else rasterize_workspace_bytes(N, F, height, width)
    ws = workspace if workspace is not None else _out(nbytes, dtype=th.uint8, device=v.device)
    _check(
        lib().drtk_amd_rasterize(
            ctypes.c_int(_dt(v)), _p(v), _p(vi_c), _i(N), _i(V), _i(F), _i(vi_sN), _i(height), _i(width),
            ctypes.c_int(1 if wireframe else 0), _p(depth), _p(index), _p(ws), ctypes.c_size_t(ws.numel()),
            _stream(v, stream)),
        "rasterize")
    return depth, index


MAX_RASTER_LAYERS = 8  # DRTK_AMD_MAX_RASTER_LAYERS (include/drtk_amd.h)


def rasterize_layers_workspace_bytes(N, F, H, W, num_layers) -> int:
    out = ctypes.c_size_t(0)
    _check(
        lib().drtk_amd_rasterize_layers_workspace_bytes(_i(N), _i(F), _i(H), _i(W), ctypes.c_int(int(num_layers)), ctypes.byref(out)),
        "rasterize_layers")
    return out.value


@_on_tensor_device
def rasterize_layers(v, vi, height, width, num_layers, stream=None, workspace=None, out=None) -> Tuple[th.Tensor, th.Tensor]:
    """The `num_layers` nearest triangles per pixel: (depth_img, index_img), [N,K,H,W] float32 / int32.
    `out` = (depth_img, index_img) to write into (contiguous, any element offset of a larger buffer)."""
    v = v.contiguous()
    N, V, _ = v.shape
    K = int(num_layers)
    vi_c, vi_sN, F = _vi(vi, N)
    nbytes = rasterize_layers_workspace_bytes(N, F, height, width, K)  # raises on a bad num_layers, before any allocation
    if out is not None:
        depth, index = out
        assert depth.shape == (N, K, height, width) and index.shape == (N, K, height, width) and depth.is_contiguous() and index.is_contiguous()
        assert depth.dtype == th.float32 and index.dtype == th.int32
    else:
        depth = _out(N, K, height, width, dtype=th.float32, device=v.device)
        index = _out(N, K, height, width, dtype=th.int32, device=v.device)
    ws = workspace if workspace is not None else _out(nbytes, dtype=th.uint8, device=v.device)
    _check(
        lib().drtk_amd_rasterize_layers(
            ctypes.c_int(_dt(v)), _p(v), _p(vi_c), _i(N), _i(V), _i(F), _i(vi_sN), _i(height), _i(width),
            ctypes.c_int(K), _p(depth), _p(index), _p(ws), ctypes.c_size_t(ws.numel()), _stream(v, stream)),
        "rasterize_layers")
    return depth, index


@_on_tensor_device
def render(v, vi, index_img, stream=None):
    v = v.contiguous()
    index_img = index_img.contiguous()
    N, V, _ = v.shape
    H, W = index_img.shape[1:]
    vi_c, vi_sN, F = _vi(vi, N)
    depth = _out(N, H, W, dtype=v.dtype, device=v.device)
    bary = _out(N, 3, H, W, dtype=v.dtype, device=v.device)
    _check(
        lib().drtk_amd_render(
            ctypes.c_int(_dt(v)), _p(v), _p(vi_c), _p(index_img), _i(N), _i(V), _i(F), _i(vi_sN), _i(H), _i(W),
            _p(depth), _p(bary), _stream(v, stream)),
        "render")
    return depth, bary


@_on_tensor_device
def render_backward(v, vi, index_img, grad_depth_img, grad_bary_img, stream=None):
    v = v.contiguous()
    index_img = index_img.contiguous()
    gd, gb = grad_depth_img.contiguous(), grad_bary_img.contiguous()
    N, V, _ = v.shape
    H, W = index_img.shape[1:]
    vi_c, vi_sN, F = _vi(vi, N)
    grad_v = _out(N, V, 3, dtype=v.dtype, device=v.device)
    _check(
        lib().drtk_amd_render_backward(
            ctypes.c_int(_dt(v)), _p(v), _p(vi_c), _p(index_img), _p(gd), _p(gb), _i(N), _i(V), _i(F), _i(vi_sN),
            _i(H), _i(W), _p(grad_v), _stream(v, stream)),
        "render_backward")
    return grad_v


@_on_tensor_device
def interpolate(attrs, vi, index_img, bary_img, stream=None, masked=False):
    attrs = attrs.contiguous()
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    N, V, C = attrs.shape
    H, W = index_img.shape[1:]
    vi_c, vi_sN, F = _vi(vi, N)
    out = _out(N, C, H, W, dtype=attrs.dtype, device=attrs.device)
    fn = lib().drtk_amd_interpolate_masked if masked else lib().drtk_amd_interpolate
    _check(
        fn(ctypes.c_int(_dt(attrs)), _p(attrs), _p(vi_c), _p(index_img), _p(bary_img), _i(N), _i(V), _i(C), _i(F),
           _i(vi_sN), _i(H), _i(W), _p(out), _stream(attrs, stream)),
        "interpolate_masked" if masked else "interpolate")
    return out


def interpolate_masked(attrs, vi, index_img, bary_img, stream=None):
    """drtk_amd extension: `interpolate` with the background pixels written as 0 (include/drtk_amd.h)."""
    return interpolate(attrs, vi, index_img, bary_img, stream, masked=True)


@_on_tensor_device
def interpolate_backward(grad_out, attrs, vi, index_img, bary_img, vert_requires_grad=True,
                         bary_requires_grad=True, stream=None, workspace=None):
    """workspace=False: the entry point's unpadded route (no scratch buffer), for A/B and for the parity tests of both routes."""
    grad_out = grad_out.contiguous()
    attrs = attrs.contiguous()
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    N, V, C = attrs.shape
    H, W = index_img.shape[1:]
    vi_c, vi_sN, F = _vi(vi, N)
    ag = _out(N, V, C, dtype=attrs.dtype, device=attrs.device) if vert_requires_grad else None
    bg = _out(N, 3, H, W, dtype=attrs.dtype, device=attrs.device) if bary_requires_grad else None
    ws, nbytes = None, 0
    if os.environ.get("DRTK_CAPI_NO_INTERP_WS"):  # A/B of the two routes from the command line (profiles/shape_bench.py)
        workspace = False
    if vert_requires_grad and workspace is not False:  # the optional scratch of the padded-row route (include/drtk_amd.h)
        out = ctypes.c_size_t(0)
        _check(lib().drtk_amd_interpolate_backward_workspace_bytes(ctypes.c_int(_dt(attrs)), _i(N), _i(V), _i(C), ctypes.byref(out)), "interpolate_backward")
        nbytes = int(out.value)
        if nbytes:
            ws = _out((nbytes + 3) // 4, dtype=th.float32, device=attrs.device)
            assert ws.data_ptr() % 64 == 0 or os.environ.get("DRTK_CAPI_GUARD"), "torch allocations are 256-byte aligned"
            if ws.data_ptr() % 64 != 0:  # (guarded allocations are only element-aligned: no workspace then)
                ws, nbytes = None, 0
    _check(
        lib().drtk_amd_interpolate_backward_ws(
            ctypes.c_int(_dt(attrs)), _p(grad_out), _p(attrs), _p(vi_c), _p(index_img), _p(bary_img), _i(N), _i(V),
            _i(C), _i(F), _i(vi_sN), _i(H), _i(W), _p(ag), _p(bg), _p(ws), ctypes.c_size_t(nbytes), _stream(attrs, stream)),
        "interpolate_backward")
    return ag, bg


@_on_tensor_device
def interpolation_matrix(vi, index_img, bary_img, stream=None):
    """-> (crow_indices, col_indices, values, row_pixels); row_pixels/crow are built with torch ops
    (the caller's side of the C ABI), columns and values by drtk_amd_interpolation_matrix."""
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    N, H, W = index_img.shape
    vi_c, vi_sN, F = _vi(vi, N)
    row_pixels = th.nonzero(index_img.reshape(-1).ne(-1)).reshape(-1)
    R = row_pixels.numel()
    crow = th.arange(0, 3 * R + 1, 3, dtype=th.int64, device=index_img.device)
    col = _out(3 * R, dtype=th.int64, device=index_img.device)
    values = _out(3 * R, dtype=bary_img.dtype, device=bary_img.device)
    _check(
        lib().drtk_amd_interpolation_matrix(
            ctypes.c_int(_dt(bary_img)), _p(vi_c), _p(index_img), _p(bary_img), _p(row_pixels), _i(R), _i(N), _i(F),
            _i(vi_sN), _i(H), _i(W), _p(col), _p(values), _stream(bary_img, stream)),
        "interpolation_matrix")
    return crow, col, values, row_pixels


@_on_tensor_device
def interpolation_matrix_backward(grad_values, vi, index_img, row_pixels, stream=None):
    grad_values = grad_values.contiguous()
    index_img = index_img.contiguous()
    row_pixels = row_pixels.contiguous()
    N, H, W = index_img.shape
    vi_c, vi_sN, F = _vi(vi, N)
    bg = _out(N, 3, H, W, dtype=grad_values.dtype, device=grad_values.device)
    _check(
        lib().drtk_amd_interpolation_matrix_backward(
            ctypes.c_int(_dt(grad_values)), _p(grad_values), _p(vi_c), _p(index_img), _p(row_pixels),
            _i(row_pixels.numel()), _i(N), _i(F), _i(vi_sN), _i(H), _i(W), _p(bg), _stream(grad_values, stream)),
        "interpolation_matrix_backward")
    return bg


def _pairs(pair_indices, N):
    assert pair_indices.dtype == th.int32 and pair_indices.shape[-1] == 9
    if pair_indices.ndim == 2:
        return pair_indices.contiguous(), 0, pair_indices.shape[0]
    if pair_indices.shape[0] == N and N > 1 and pair_indices.stride(0) == 0:
        return pair_indices[0].contiguous(), 0, pair_indices.shape[1]
    p = pair_indices.contiguous()
    return p, p.shape[1] * 9, p.shape[1]


@_on_tensor_device
def interpolation_normal_matrix_values(pair_indices, index_img, bary_img, nnz, stream=None):
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    N, H, W = index_img.shape
    pr, pair_sN, F = _pairs(pair_indices, N)
    values = _out(nnz, dtype=bary_img.dtype, device=bary_img.device)
    _check(
        lib().drtk_amd_interpolation_normal_matrix_values(
            ctypes.c_int(_dt(bary_img)), _p(pr), _p(index_img), _p(bary_img), _i(N), _i(F), _i(pair_sN), _i(H), _i(W),
            _i(nnz), _p(values), _stream(bary_img, stream)),
        "interpolation_normal_matrix_values")
    return values


@_on_tensor_device
def interpolation_normal_matrix_values_backward(grad_values, pair_indices, index_img, bary_img, stream=None):
    grad_values = grad_values.contiguous()
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    N, H, W = index_img.shape
    pr, pair_sN, F = _pairs(pair_indices, N)
    bg = _out(N, 3, H, W, dtype=bary_img.dtype, device=bary_img.device)
    _check(
        lib().drtk_amd_interpolation_normal_matrix_values_backward(
            ctypes.c_int(_dt(bary_img)), _p(grad_values), _p(pr), _p(index_img), _p(bary_img), _i(N), _i(F),
            _i(pair_sN), _i(H), _i(W), _p(bg), _stream(bary_img, stream)),
        "interpolation_normal_matrix_values_backward")
    return bg


def _level_table(levels):
    """Device pointers, sizes and view strides of a mip pyramid.  A level whose views are contiguous [C,h,w] blocks is
    passed as it is, whatever its batch stride -- in particular a [1,C,h,w] texture expanded to N views (stride 0) is
    not materialised N times; anything else is made contiguous first."""
    lv = []
    for t in levels:
        ok = t.dim() == 4 and (t.shape[0] == 0 or t[0].is_contiguous()) and (t.stride(0) == 0 or t.stride(0) >= t[0].numel() or t.shape[0] <= 1)
        lv.append(t if ok else t.contiguous())
    n = len(lv)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in lv])
    lh = (ctypes.c_int64 * n)(*[t.shape[2] for t in lv])
    lw = (ctypes.c_int64 * n)(*[t.shape[3] for t in lv])
    lsn = (ctypes.c_int64 * n)(*[(t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2] * t.shape[3]) for t in lv])
    return lv, ptrs, lh, lw, lsn


def _grid_layout(grid):
    """(tensor to pass, {sN, sP, sC} in elements): a uv field [N,H,W,2] whose pixels are evenly spaced in memory is read
    in place -- contiguous, or the channel-first image of `interpolate` seen through permute(0, 2, 3, 1); anything else
    (overlapping views, rows with padding, other permutations) is made contiguous first."""
    N, H, W, two = grid.shape
    sN, sH, sW, sC = grid.stride()
    P = H * W
    rows_ok = H <= 1 or sH == W * sW
    pixel_major = sC == 1 and sW == 2 and rows_ok and (N <= 1 or sN >= 2 * P)             # [N,H,W,2]
    channel_major = sW == 1 and sC >= P and rows_ok and (N <= 1 or sN >= sC + P)          # [N,2,H,W] seen as [N,H,W,2]
    if not (two == 2 and P > 0 and (pixel_major or channel_major)):
        grid = grid.contiguous()
        sN, sW, sC = 2 * P, 2, 1
    return grid, (ctypes.c_int64 * 3)(sN if N > 1 else 2 * P, sW, sC)


@_on_tensor_device
def mipmap_grid_sampler_2d(levels, grid, vt_dxdy_img, max_aniso, padding_mode=0, interpolation_mode=0,
                           align_corners=False, force_max_aniso=False, clip_grad=False, stream=None):
    lv, ptrs, lh, lw, lsn = _level_table(levels)
    grid, glayout = _grid_layout(grid)
    vt = vt_dxdy_img.contiguous()
    N, C = lv[0].shape[:2]
    H, W = grid.shape[1:3]
    out = _out(N, C, H, W, dtype=lv[0].dtype, device=lv[0].device)
    _check(
        lib().drtk_amd_mipmap_grid_sampler_2d(
            ctypes.c_int(_dt(lv[0])), ptrs, lh, lw, lsn, ctypes.c_int(len(lv)), _p(grid), glayout, _p(vt), _i(N), _i(C), _i(H), _i(W),
            ctypes.c_int(max_aniso), ctypes.c_int(padding_mode), ctypes.c_int(interpolation_mode),
            ctypes.c_int(bool(align_corners)), ctypes.c_int(bool(force_max_aniso)), ctypes.c_int(bool(clip_grad)),
            _p(out), _stream(lv[0], stream)),
        "mipmap_grid_sampler_2d")
    return out


@_on_tensor_device
def mipmap_grid_sampler_2d_backward(grad_out, levels, grid, vt_dxdy_img, max_aniso, padding_mode=0,
                                    interpolation_mode=0, align_corners=False, force_max_aniso=False,
                                    clip_grad=False, stream=None):
    lv, ptrs, lh, lw, lsn = _level_table(levels)
    grid, glayout = _grid_layout(grid)
    vt = vt_dxdy_img.contiguous()
    grad_out = grad_out.contiguous()
    N, C = lv[0].shape[:2]
    H, W = grid.shape[1:3]
    # contiguous even for an expanded pyramid, and back to back in one buffer: the call then zeroes them with one launch
    flat = _out(sum(t.numel() for t in lv), dtype=lv[0].dtype, device=lv[0].device)
    glv, off = [], 0
    for t in lv:
        glv.append(flat[off:off + t.numel()].view(t.shape))
        off += t.numel()
    gptrs = (ctypes.c_void_p * len(lv))(*[t.data_ptr() for t in glv])
    ggrid = th.empty_strided(grid.shape, grid.stride(), dtype=grid.dtype, device=grid.device)  # laid out like the grid it belongs to
    _check(
        lib().drtk_amd_mipmap_grid_sampler_2d_backward(
            ctypes.c_int(_dt(lv[0])), _p(grad_out), ptrs, lh, lw, lsn, ctypes.c_int(len(lv)), _p(grid), glayout, _p(vt), _i(N), _i(C),
            _i(H), _i(W), ctypes.c_int(max_aniso), ctypes.c_int(padding_mode), ctypes.c_int(interpolation_mode),
            ctypes.c_int(bool(align_corners)), ctypes.c_int(bool(force_max_aniso)), ctypes.c_int(bool(clip_grad)),
            gptrs, _p(ggrid), glayout, _stream(lv[0], stream)),
        "mipmap_grid_sampler_2d_backward")
    return glv, ggrid


@_on_tensor_device
def grid_scatter_2d(input, grid, output_height, output_width, padding_mode=1, interpolation_mode=0, align_corners=False,
                    stream=None, route_counts=None):
    """out [N,C,output_height,output_width]: every pixel of input [N,C,H,W] added, weighted, to the texels grid_sample
    would read at grid [N,H,W,2].  `route_counts`: an int32 / uint32 device tensor of two ZEROED counters that receives
    the number of workgroups per kernel route (windowed, direct) -- include/drtk_amd.h."""
    input = input.contiguous()
    grid, glayout = _grid_layout(grid)
    N, C, H, W = input.shape
    assert grid.shape == (N, H, W, 2) and grid.dtype == input.dtype, (grid.shape, input.shape)
    if route_counts is not None:
        assert route_counts.numel() == 2 and route_counts.element_size() == 4 and route_counts.is_contiguous() and route_counts.device == input.device
    out = _out(N, C, int(output_height), int(output_width), dtype=input.dtype, device=input.device)
    _check(
        lib().drtk_amd_grid_scatter_2d(
            ctypes.c_int(_dt(input)), _p(input), _p(grid), glayout, _i(N), _i(C), _i(H), _i(W), _i(output_height),
            _i(output_width), ctypes.c_int(padding_mode), ctypes.c_int(interpolation_mode), ctypes.c_int(bool(align_corners)),
            _p(out), _p(route_counts), _stream(input, stream)),
        "grid_scatter_2d")
    return out


@_on_tensor_device
def grid_scatter_2d_backward(grad_out, input, grid, padding_mode=1, interpolation_mode=0, align_corners=False,
                             input_requires_grad=True, grid_requires_grad=True, stream=None):
    """(grad_input [N,C,H,W] or None, grad_grid laid out like `grid` or None)."""
    input = input.contiguous()
    grad_out = grad_out.contiguous()
    grid, glayout = _grid_layout(grid)
    N, C, H, W = input.shape
    OH, OW = grad_out.shape[2:]
    assert grad_out.shape[:2] == (N, C) and grid.shape == (N, H, W, 2)
    gi = _out(N, C, H, W, dtype=input.dtype, device=input.device) if input_requires_grad else None
    gg = None
    if grid_requires_grad:  # laid out like the grid it belongs to
        gg = th.empty_strided(grid.shape, grid.stride(), dtype=grid.dtype, device=grid.device)
        if _POISON and gg.numel():
            gg.fill_(float("nan"))
    _check(
        lib().drtk_amd_grid_scatter_2d_backward(
            ctypes.c_int(_dt(input)), _p(grad_out), _p(input), _p(grid), glayout, _i(N), _i(C), _i(H), _i(W), _i(OH), _i(OW),
            ctypes.c_int(padding_mode), ctypes.c_int(interpolation_mode), ctypes.c_int(bool(align_corners)), _p(gi), _p(gg),
            glayout, _stream(input, stream)),
        "grid_scatter_2d_backward")
    return gi, gg


def _msi_args(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh):
    assert ray_o.dtype == th.float32 and ray_d.dtype == th.float32 and ray_o.shape == ray_d.shape and ray_o.shape[1:] == (3,)
    assert texture.ndim == 4 and texture.shape[1] == 4, texture.shape
    L, _, H, W = texture.shape
    return (_i(ray_o.shape[0]), _i(L), _i(H), _i(W), ctypes.c_int(int(sub_step_count)), ctypes.c_double(min_inv_r),
            ctypes.c_double(max_inv_r), ctypes.c_double(stop_thresh))


@_on_tensor_device
def msi_forward(ray_o, ray_d, texture, sub_step_count=2, min_inv_r=1.0, max_inv_r=0.0, stop_thresh=1e-7, stream=None):
    """out [N,4] = (r, g, b, log_transmit) of the rays ray_o, ray_d [N,3] (float32) marched through the multi-sphere image
    texture [L,4,H,W] -- include/drtk_amd.h."""
    ray_o, ray_d, texture = ray_o.contiguous(), ray_d.contiguous(), texture.contiguous()
    out = _out(ray_o.shape[0], 4, dtype=texture.dtype, device=texture.device)
    _check(
        lib().drtk_amd_msi_forward(
            ctypes.c_int(_dt(texture)), _p(ray_o), _p(ray_d), _p(texture),
            *_msi_args(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh), _p(out), _stream(texture, stream)),
        "msi_forward")
    return out


@_on_tensor_device
def msi_backward(grad_out, out, ray_o, ray_d, texture, sub_step_count=2, min_inv_r=1.0, max_inv_r=0.0, stop_thresh=1e-7, stream=None):
    """grad_texture [L,4,H,W] from grad_out [N,4] (column 3 is not read) and the forward's `out`."""
    ray_o, ray_d, texture = ray_o.contiguous(), ray_d.contiguous(), texture.contiguous()
    grad_out, out = grad_out.contiguous(), out.contiguous()
    assert grad_out.shape == out.shape == (ray_o.shape[0], 4) and grad_out.dtype == out.dtype == texture.dtype
    gt = _out(*texture.shape, dtype=texture.dtype, device=texture.device)
    _check(
        lib().drtk_amd_msi_backward(
            ctypes.c_int(_dt(texture)), _p(grad_out), _p(out), _p(ray_o), _p(ray_d), _p(texture),
            *_msi_args(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh), _p(gt), _stream(texture, stream)),
        "msi_backward")
    return gt


def _composite_args(color, alpha, index_img, background):
    """(color [N,K,C,H,W], alpha [N,K,H,W], index, background, the C arguments they make): the layers of composite_layers
    as views whose H x W planes are contiguous -- `alpha=None` takes `color` as rgba with alpha as its last channel."""
    assert color.ndim == 5, color.shape
    if alpha is None:
        assert color.shape[2] >= 2, color.shape
        color, alpha = color[:, :, :-1], color[:, :, -1]
    elif alpha.ndim == 5:
        assert alpha.shape[2] == 1, alpha.shape
        alpha = alpha[:, :, 0]
    N, K, C, H, W = color.shape
    assert alpha.shape == (N, K, H, W) and alpha.dtype == color.dtype, (alpha.shape, color.shape)

    def planes(t):
        ok = (W <= 1 or t.stride(-1) == 1) and (H <= 1 or t.stride(-2) == W)
        return t if ok else t.contiguous()

    color, alpha = planes(color), planes(alpha)
    if index_img is not None:
        assert index_img.shape == (N, K, H, W) and index_img.dtype == th.int32, index_img.shape
        index_img = index_img.contiguous()
    bg_sN = 0
    if background is not None:
        assert background.shape == (N, C, H, W) and background.dtype == color.dtype, background.shape
        if N > 1 and background.stride(0) == 0:
            background = background[0].contiguous()
        else:
            background, bg_sN = background.contiguous(), C * H * W
    args = (_p(color), (ctypes.c_int64 * 3)(*color.stride()[:3]), _p(alpha), (ctypes.c_int64 * 2)(*alpha.stride()[:2]),
            _p(index_img), _p(background), _i(bg_sN), _i(N), _i(K), _i(C), _i(H), _i(W))
    return color, alpha, index_img, background, args


@_on_tensor_device
def composite_layers(color, alpha=None, index_img=None, background=None, stream=None):
    """(img [N,C,H,W], transmittance [N,1,H,W]): the K layers color [N,K,C,H,W] / alpha [N,K,H,W] (or rgba [N,K,C+1,H,W] with
    `alpha=None`) composited front to back, layers whose index_img is -1 skipped, over `background` -- include/drtk_amd.h."""
    color, alpha, index_img, background, args = _composite_args(color, alpha, index_img, background)
    N, K, C, H, W = color.shape
    img = _out(N, C, H, W, dtype=color.dtype, device=color.device)
    trans = _out(N, 1, H, W, dtype=color.dtype, device=color.device)
    _check(
        lib().drtk_amd_composite_layers(ctypes.c_int(_dt(color)), *args, _p(img), _p(trans), _stream(color, stream)),
        "composite_layers")
    return img, trans


@_on_tensor_device
def composite_layers_backward(grad_img, grad_transmittance, color, alpha=None, index_img=None, background=None,
                              want_color=True, want_alpha=True, want_background=True, stream=None):
    """(grad_color, grad_alpha, grad_background), None where not wanted (or where there is no background); grad_img
    [N,C,H,W] / grad_transmittance [N,1,H,W] may be None.  With `alpha=None` (rgba) grad_color is the one [N,K,C+1,H,W]
    gradient, made if either of the two is wanted, and grad_alpha is None."""
    rgba = alpha is None
    shape, alpha_shape = color.shape, (None if rgba else alpha.shape)
    color, alpha, index_img, background, args = _composite_args(color, alpha, index_img, background)
    N, K, C, H, W = color.shape
    if grad_img is not None:
        grad_img = grad_img.contiguous()
        assert grad_img.shape == (N, C, H, W) and grad_img.dtype == color.dtype
    if grad_transmittance is not None:
        grad_transmittance = grad_transmittance.contiguous()
        assert grad_transmittance.shape == (N, 1, H, W) and grad_transmittance.dtype == color.dtype
    gc = ga = gb = gc_view = ga_view = None
    if rgba:
        if want_color or want_alpha:
            gc = _out(*shape, dtype=color.dtype, device=color.device)
            gc_view, ga_view = gc[:, :, :-1], gc[:, :, -1]
    else:
        if want_color:
            gc = gc_view = _out(*shape, dtype=color.dtype, device=color.device)
        if want_alpha:
            ga = _out(*alpha_shape, dtype=color.dtype, device=color.device)
            ga_view = ga[:, :, 0] if ga.ndim == 5 else ga
    if want_background and background is not None:
        gb = _out(N, C, H, W, dtype=color.dtype, device=color.device)
    gcs = (ctypes.c_int64 * 3)(*(gc_view.stride()[:3] if gc_view is not None else (0, 0, 0)))
    gas = (ctypes.c_int64 * 2)(*(ga_view.stride()[:2] if ga_view is not None else (0, 0)))
    _check(
        lib().drtk_amd_composite_layers_backward(
            ctypes.c_int(_dt(color)), _p(grad_img), _p(grad_transmittance), *args, _p(gc_view), gcs, _p(ga_view), gas, _p(gb),
            _stream(color, stream)),
        "composite_layers_backward")
    return gc, ga, gb


def _pyramid_views(t, shape):
    """A level [N,C,h,w] as the C ABI takes it: contiguous views, any view stride."""
    assert tuple(t.shape) == tuple(shape), (t.shape, shape)
    return t if (t.shape[0] == 0 or t[0].is_contiguous()) else t.contiguous()


@_on_tensor_device
def mipmap_pyramid(input, levels, out=None, stream=None):
    """The `levels` mip levels of input [N,C,H,W], finest first: element 0 is `input` itself, level l is [N,C,H >> l,W >> l]
    -- include/drtk_amd.h.  `out`: `levels` tensors to write the levels into (entry 0 is not looked at), each with
    contiguous views; by default they are allocated here, one by one."""
    assert input.ndim == 4, input.shape
    N, C, H, W = input.shape
    planes_ok = (W <= 1 or input.stride(3) == 1) and (H <= 1 or input.stride(2) == W)
    x = input if planes_ok else input.contiguous()
    levels = int(levels)
    if not 1 <= levels <= 11:
        _check(-1, "mipmap_pyramid")
    if out is None:
        out = [None] + [_out(N, C, H >> l, W >> l, dtype=x.dtype, device=x.device) for l in range(1, levels)]
    assert len(out) == levels, (len(out), levels)
    for l in range(1, levels):
        assert out[l].dtype == x.dtype and _pyramid_views(out[l], (N, C, H >> l, W >> l)) is out[l], l
    ptrs = (ctypes.c_void_p * levels)(*[0 if l == 0 else out[l].data_ptr() for l in range(levels)])
    sn = (ctypes.c_int64 * levels)(*[0 if l == 0 else (out[l].stride(0) if N > 1 else out[l][0].numel() if N else 0) for l in range(levels)])
    _check(
        lib().drtk_amd_mipmap_pyramid(
            ctypes.c_int(_dt(x)), _p(x), _i(x.stride(0)), _i(x.stride(1)), _i(N), _i(C), _i(H), _i(W), ctypes.c_int(levels), ptrs, sn,
            _stream(x, stream)),
        "mipmap_pyramid")
    return [input] + list(out[1:])


@_on_tensor_device
def mipmap_pyramid_backward(grad_levels, grad_input=None, stream=None):
    """grad_input [N,C,H,W] of the gradients of the `len(grad_levels)` levels: tensors [N,C,H >> l,W >> l], or None where a
    level received none (taken as zeros, never read); entry 0 or `grad_input` (a contiguous tensor to write into) says what
    H and W are, so one of the two must be given."""
    levels = len(grad_levels)
    given = [g for g in grad_levels if g is not None]
    like = grad_input if grad_input is not None else grad_levels[0]
    assert given and like is not None, "mipmap_pyramid_backward: no gradient, or neither grad_levels[0] nor grad_input"
    N, C, H, W = like.shape
    if not 1 <= levels <= 11:
        _check(-1, "mipmap_pyramid_backward")
    gl = [None if g is None else _pyramid_views(g, (N, C, H >> l, W >> l)) for l, g in enumerate(grad_levels)]
    assert all(g is None or g.dtype == like.dtype for g in gl)
    if grad_input is None:
        grad_input = _out(N, C, H, W, dtype=like.dtype, device=like.device)
    assert grad_input.is_contiguous() and grad_input.dtype == like.dtype
    ptrs = (ctypes.c_void_p * levels)(*[0 if g is None else g.data_ptr() for g in gl])
    sn = (ctypes.c_int64 * levels)(*[0 if g is None else (g.stride(0) if N > 1 else g[0].numel() if N else 0) for g in gl])
    _check(
        lib().drtk_amd_mipmap_pyramid_backward(
            ctypes.c_int(_dt(like)), ptrs, sn, _i(N), _i(C), _i(H), _i(W), ctypes.c_int(levels), _p(grad_input),
            _stream(like, stream)),
        "mipmap_pyramid_backward")
    return grad_input


IMAGE_LOSS_MODES = {"map": 0, "ssim": 1, "photometric": 2}


def image_loss_workspace_bytes(N, H, W, window_size=11, valid=False) -> int:
    out = ctypes.c_size_t(0)
    _check(
        lib().drtk_amd_image_loss_workspace_bytes(_i(N), _i(H), _i(W), ctypes.c_int(int(window_size)), ctypes.c_int(bool(valid)), ctypes.byref(out)),
        "image_loss")
    return out.value


def _image_loss_rows(t):
    """An image [N,C,H,W] as the C ABI takes it: rows contiguous, any view / channel / row stride."""
    assert t.ndim == 4, t.shape
    return t if (t.shape[3] <= 1 or t.stride(3) == 1) else t.contiguous()


def _image_loss_weight(weight, like):
    """(tensor or None, weight_kind, strides {sN, sH}) of a weight [N,H,W] / [N,1,H,W], bool or the images' dtype."""
    if weight is None:
        return None, 0, (ctypes.c_int64 * 2)(0, 0)
    N, _, H, W = like.shape
    w = weight[:, 0] if weight.ndim == 4 else weight
    assert tuple(w.shape) == (N, H, W) and w.dtype in (th.bool, like.dtype), (weight.shape, weight.dtype)
    if W > 1 and w.stride(2) != 1:
        w = w.contiguous()
    return w, (1 if w.dtype == th.bool else 2), (ctypes.c_int64 * 2)(w.stride(0), w.stride(1))


def _image_loss_common(img, target, weight, window_size, sigma, data_range, valid, mode, l1_weight, ssim_weight):
    assert img.shape == target.shape and img.dtype == target.dtype, (img.shape, target.shape, img.dtype, target.dtype)
    x, y = _image_loss_rows(img), _image_loss_rows(target)
    w, kind, ws = _image_loss_weight(weight, x)
    N, C, H, W = x.shape
    strides = [(ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (x, y)]
    head = (ctypes.c_int(_dt(x)), _p(x), strides[0], _p(y), strides[1], _p(w), ctypes.c_int(kind), ws, _i(N), _i(C), _i(H), _i(W),
            ctypes.c_int(int(window_size)), ctypes.c_double(sigma), ctypes.c_double(data_range), ctypes.c_int(bool(valid)),
            ctypes.c_int(IMAGE_LOSS_MODES[mode]), ctypes.c_double(l1_weight), ctypes.c_double(ssim_weight))
    return x, (x, y, w), head


@_on_tensor_device
def image_loss_forward(img, target, weight=None, mode="ssim", window_size=11, sigma=1.5, data_range=1.0, valid=False, l1_weight=0.8,
                       ssim_weight=0.2, with_maps=False, stream=None):
    """(out, maps, scalars) of drtk_amd_image_loss_forward -- include/drtk_amd.h.  `mode`: "map" (out = S [N,C,OH,OW]),
    "ssim" or "photometric" (out has one element).  `maps` [3,N,C,OH,OW] only `with_maps` (what the backward needs),
    `scalars` (4 doubles) only for the two means."""
    x, keep, head = _image_loss_common(img, target, weight, window_size, sigma, data_range, valid, mode, l1_weight, ssim_weight)
    N, C, H, W = x.shape
    nbytes = image_loss_workspace_bytes(N, H, W, window_size, valid)  # raises on a bad window or shape, before any allocation
    off = (int(window_size) // 2) if valid else 0
    OH, OW = H - 2 * off, W - 2 * off
    out = _out(N, C, OH, OW, dtype=x.dtype, device=x.device) if mode == "map" else _out(1, dtype=x.dtype, device=x.device)
    maps = _out(3, N, C, OH, OW, dtype=x.dtype, device=x.device) if with_maps else None
    scalars = ws = None
    if mode != "map":
        scalars = _out(4, dtype=th.float64, device=x.device)
        ws = _out(nbytes // 8, dtype=th.float64, device=x.device)
    _check(
        lib().drtk_amd_image_loss_forward(*head, _p(out), _p(maps), _p(scalars), _p(ws), ctypes.c_size_t(nbytes), _stream(x, stream)),
        "image_loss_forward")
    return (out if mode == "map" else out[0]), maps, scalars


@_on_tensor_device
def image_loss_backward(img, target, weight, maps, grad_out, scalars, mode="ssim", window_size=11, sigma=1.5, data_range=1.0,
                        valid=False, l1_weight=0.8, ssim_weight=0.2, stream=None):
    """grad_img [N,C,H,W] of drtk_amd_image_loss_backward; `grad_out` is the gradient of the map (mode "map") or of the
    scalar, `maps` and `scalars` what image_loss_forward(..., with_maps=True) returned."""
    x, keep, head = _image_loss_common(img, target, weight, window_size, sigma, data_range, valid, mode, l1_weight, ssim_weight)
    image_loss_workspace_bytes(x.shape[0], x.shape[2], x.shape[3], window_size, valid)
    grad_out = grad_out.to(x.dtype).contiguous()
    assert maps.is_contiguous() and maps.dtype == x.dtype
    assert grad_out.numel() == (maps[0].numel() if mode == "map" else 1), grad_out.shape
    grad = _out(*x.shape, dtype=x.dtype, device=x.device)
    _check(
        lib().drtk_amd_image_loss_backward(*head, _p(maps), _p(grad_out), _p(scalars), _p(grad), _stream(x, stream)),
        "image_loss_backward")
    return grad


def shade_workspace_bytes(dtype, N, H, W) -> int:
    out = ctypes.c_size_t(0)
    dt = DRTK_F32 if dtype == th.float32 else DRTK_F64 if dtype == th.float64 else -1
    _check(lib().drtk_amd_shade_workspace_bytes(ctypes.c_int(dt), _i(N), _i(H), _i(W), ctypes.byref(out)), "shade")
    return out.value


def _shade_args(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma):
    """(the tensors kept alive, the C arguments of the inputs, (N, C, H, W)) of the two shade entry points: images whose W
    stride is 1 as they are with their strides {sN, sC, sH}, parameters contiguous with sN = 0 ([K]) or K ([N, K])."""
    N, _, H, W = normal_img.shape
    C = ambient.shape[-1]
    keep, none3 = [], (ctypes.c_int64 * 3)(0, 0, 0)

    def image(t, shape, dtype):
        if t is None:
            return _p(None), none3
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, (t.shape, shape, t.dtype)
        t = t if (W <= 1 or t.stride(-1) == 1) else t.contiguous()
        keep.append(t)
        return _p(t), (ctypes.c_int64 * 3)(*(tuple(t.stride()[:-1]) + (0,))[:3])

    def param(t, count):
        if t is None:
            return _p(None), _i(0)
        assert t.dtype == normal_img.dtype and tuple(t.shape) in ((count,), (N, count)), (t.shape, count)
        t = t.contiguous()
        keep.append(t)
        return _p(t), _i(count if t.ndim == 2 else 0)

    dt = normal_img.dtype
    albedo_img = albedo if albedo.ndim == 4 else None
    args = (*image(normal_img, (N, 3, H, W), dt), *image(pos_img if specular is not None else None, (N, 3, H, W), dt),
            *image(albedo_img, (N, C, H, W), dt), *image(background, (N, C, H, W), dt), *image(index_img, (N, H, W), th.int32),
            *param(light_dir, 3), *param(None if albedo_img is not None else albedo, C), *param(ambient, C), *param(specular, C),
            *param(shininess if specular is not None else None, 1), ctypes.c_double(0.0 if gamma is None else float(gamma)),
            _i(N), _i(C), _i(H), _i(W))
    return keep, args, (N, C, H, W)


@_on_tensor_device
def shade_forward(normal_img, light_dir, albedo, ambient, index_img=None, pos_img=None, specular=None, shininess=None,
                  background=None, gamma=None, stream=None):
    """out [N,C,H,W] of drtk_amd_shade_forward -- include/drtk_amd.h; the arguments of drtk_amd.shade."""
    keep, args, (N, C, H, W) = _shade_args(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma)
    out = _out(N, C, H, W, dtype=normal_img.dtype, device=normal_img.device)
    _check(lib().drtk_amd_shade_forward(ctypes.c_int(_dt(normal_img)), *args, _p(out), _stream(normal_img, stream)), "shade_forward")
    return out


SHADE_GRADS = ("normal_img", "pos_img", "albedo", "background", "light_dir", "ambient", "specular", "shininess")


@_on_tensor_device
def shade_backward(grad_out, normal_img, light_dir, albedo, ambient, index_img=None, pos_img=None, specular=None, shininess=None,
                   background=None, gamma=None, want=SHADE_GRADS, stream=None):
    """The gradients named in `want` (of SHADE_GRADS) as a dict, each in the shape of its argument -- a parameter given as
    [K] receives the sum over the views; a name whose argument is absent (or pos_img / shininess without specular) is left
    out.  drtk_amd_shade_backward -- include/drtk_amd.h."""
    keep, args, (N, C, H, W) = _shade_args(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma)
    given = {"normal_img": normal_img, "pos_img": pos_img if specular is not None else None, "albedo": albedo, "background": background,
             "light_dir": light_dir, "ambient": ambient, "specular": specular, "shininess": shininess if specular is not None else None}
    grads = {k: _out(*given[k].shape, dtype=normal_img.dtype, device=normal_img.device) for k in SHADE_GRADS
             if k in want and given[k] is not None}
    grad_out = grad_out.to(normal_img.dtype).contiguous()
    assert tuple(grad_out.shape) == (N, C, H, W), grad_out.shape
    albedo_is_image = albedo.ndim == 4

    def image(k, on=True):
        return _p(grads.get(k) if on else None)

    def param(k, count, on=True):
        g = grads.get(k) if on else None
        return _p(g), _i(count if g is not None and g.ndim == 2 else 0)

    params = [k for k in ("light_dir", "ambient", "specular", "shininess") if k in grads] + (["albedo"] if "albedo" in grads and not albedo_is_image else [])
    nbytes, ws = 0, None
    if params:
        nbytes = shade_workspace_bytes(normal_img.dtype, N, H, W)
        ws = _out(nbytes, dtype=th.uint8, device=normal_img.device)
    _check(
        lib().drtk_amd_shade_backward(
            ctypes.c_int(_dt(normal_img)), _p(grad_out), *args, image("normal_img"), image("pos_img"), image("albedo", albedo_is_image),
            image("background"), *param("light_dir", 3), *param("albedo", C, not albedo_is_image), *param("ambient", C),
            *param("specular", C), *param("shininess", 1), _p(ws), ctypes.c_size_t(nbytes), _stream(normal_img, stream)),
        "shade_backward")
    return grads


def filter2d_output_size(size, k, up=1, down=1) -> int:
    """Output length of one axis (host only): (size * up + pad0 + pad1 - k + down) // down -- include/drtk_amd.h."""
    out = ctypes.c_int64(0)
    _check(lib().drtk_amd_filter2d_output_size(_i(size), _i(k), _i(up), _i(down), ctypes.byref(out)), "filter2d_output_size")
    return out.value


_FILTER2D_DTYPES = {th.float32: DRTK_F32, th.float64: DRTK_F64, th.float16: DRTK_F16}


@_on_tensor_device
def filter2d(x, f, up=1, down=1, reflect=False, backward=False, force_generic=False, stream=None):
    """y [N,C,OH,OW] of x [N,C,H,W] (float16, float32 or float64) filtered with the float32 taps f [k]: zero-insertion by
    `up`, f along both axes, decimation by `down`; `backward` makes the call the gradient of the operator with the factors
    exchanged; `force_generic` (tests) sends a tuned (up, down, k) through the generic kernel -- include/drtk_amd.h."""
    x, f = x.contiguous(), f.contiguous()
    assert x.ndim == 4 and f.ndim == 1 and f.dtype == th.float32, (x.shape, f.shape, f.dtype)
    N, C, H, W = x.shape
    k = f.shape[0]
    y = _out(N, C, filter2d_output_size(H, k, up, down), filter2d_output_size(W, k, up, down), dtype=x.dtype, device=x.device)
    _check(
        lib().drtk_amd_filter2d(
            ctypes.c_int(_FILTER2D_DTYPES[x.dtype]), _p(x), _p(f), _i(N * C), _i(H), _i(W), _i(k), _i(up), _i(down),
            ctypes.c_int(bool(reflect)), ctypes.c_int(bool(backward)), ctypes.c_int(bool(force_generic)), _p(y), _stream(x, stream)),
        "filter2d")
    return y


@_on_tensor_device
def screen_space_uv_derivative(v, vt, vi, vti, index_img, bary_img, mask, campos, camrot, focal, stream=None):
    """v [N,V,3] or shared [V,3]; vt [N,T,2] or shared [T,2]; mask bool/uint8 [N,H,W] or None."""
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    N, H, W = index_img.shape
    v_c, vt_c = v.contiguous(), vt.contiguous()
    v_sN = 0 if v_c.ndim == 2 else v_c.shape[1] * 3
    vt_sN = 0 if vt_c.ndim == 2 else vt_c.shape[1] * 2
    V, T = v_c.shape[-2], vt_c.shape[-2]
    vi_c, vti_c = vi.contiguous(), vti.contiguous()
    m = None if mask is None else mask.to(th.uint8).contiguous()
    out = _out(N, H, W, 2, 2, dtype=bary_img.dtype, device=bary_img.device)
    _check(
        lib().drtk_amd_screen_space_uv_derivative(
            ctypes.c_int(_dt(bary_img)), _p(v_c), _i(v_sN), _p(vt_c), _i(vt_sN), _p(vi_c), _p(vti_c), _p(index_img),
            _p(bary_img), _p(m), _p(campos.contiguous()), _p(camrot.contiguous()), _p(focal.contiguous()), _i(N), _i(V),
            _i(T), _i(vi_c.shape[0]), _i(H), _i(W), _p(out), _stream(bary_img, stream)),
        "screen_space_uv_derivative")
    return out


def _transform_distort_args(v, campos, camrot, focal, princpt, coeff, fov, mode, mode_per_view, cull_outside_fov, lut, lut_spacing):
    """The arguments drtk_amd_transform_distort and its backward share; returns (tensors kept alive, ctypes list, N, V)."""
    dt = v.dtype
    N = campos.shape[0]
    assert v.ndim == 3 and v.shape[0] in (1, N) and v.shape[2] == 3, v.shape
    keep = [v.contiguous()] + [t.to(dt).contiguous() for t in (campos, camrot, focal, princpt, coeff)] + [fov.to(dt).reshape(N).contiguous()]
    V = v.shape[1]
    v_sN = 0 if (v.shape[0] == 1 and N != 1) else 3 * V
    modes = None
    if mode_per_view is not None:
        assert mode_per_view.dtype == th.int32 and mode_per_view.shape == (N,)
        modes = mode_per_view.contiguous()
    Hl = Wl = 0
    if lut is not None:
        assert lut.shape[:2] == (N, 2) and lut_spacing is not None and lut_spacing.shape == (N, 2)
        lut, lut_spacing = lut.to(dt).contiguous(), lut_spacing.to(dt).contiguous()
        Hl, Wl = lut.shape[2:]
    keep += [modes, lut, lut_spacing]
    vc, cp, cr, fo, pp, D, fv = keep[:7]
    args = [ctypes.c_int(_dt(v)), _p(vc), _i(v_sN), _p(cp), _p(cr), _p(fo), _p(pp), ctypes.c_int(int(mode)), _p(modes), _p(D),
            ctypes.c_int(int(coeff.shape[1])), _p(fv), ctypes.c_int(int(bool(cull_outside_fov))), _p(lut), _p(lut_spacing), _i(Hl), _i(Wl)]
    return keep, args, N, V


@_on_tensor_device
def transform_distort(v, campos, camrot, focal, princpt, coeff, fov, mode=0, mode_per_view=None, cull_outside_fov=False,
                      lut=None, lut_spacing=None, want_v_cam=True, stream=None):
    """(v_pix, v_cam or None), [N,V,3]: `transform` with the distortion models -- include/drtk_amd.h.  v [N,V,3] or one
    shared [1,V,3]; `mode` 0 pinhole, 1 radial-tangential, 2 fisheye, 3 fisheye62, or `mode_per_view` int32 [N]."""
    keep, args, N, V = _transform_distort_args(v, campos, camrot, focal, princpt, coeff, fov, mode, mode_per_view, cull_outside_fov, lut, lut_spacing)
    v_pix = _out(N, V, 3, dtype=v.dtype, device=v.device)
    v_cam = _out(N, V, 3, dtype=v.dtype, device=v.device) if want_v_cam else None
    _check(lib().drtk_amd_transform_distort(*args, _i(N), _i(V), _p(v_pix), _p(v_cam), _stream(v, stream)), "transform_distort")
    return v_pix, v_cam


@_on_tensor_device
def transform_distort_backward(grad_v_pix, grad_v_cam, v, campos, camrot, focal, princpt, coeff, fov, mode=0, mode_per_view=None,
                               cull_outside_fov=False, lut=None, lut_spacing=None, stream=None):
    """grad_v, shaped like v ([1,V,3]: summed over the views), from grad_v_pix and / or grad_v_cam ([N,V,3] or None)."""
    keep, args, N, V = _transform_distort_args(v, campos, camrot, focal, princpt, coeff, fov, mode, mode_per_view, cull_outside_fov, lut, lut_spacing)
    gp = None if grad_v_pix is None else grad_v_pix.to(v.dtype).contiguous()
    gc = None if grad_v_cam is None else grad_v_cam.to(v.dtype).contiguous()
    assert all(g is None or g.shape == (N, V, 3) for g in (gp, gc))
    grad_v = _out(*v.shape, dtype=v.dtype, device=v.device)
    _check(lib().drtk_amd_transform_distort_backward(*args, _p(gp), _p(gc), _i(N), _i(V), _p(grad_v), _stream(v, stream)), "transform_distort_backward")
    return grad_v


GEOMETRY_CHUNK = 256  # DRTK_GEOMETRY_CHUNK of include/drtk_amd.h


def vertex_incidence_numpy(vi, num_vertices: int, chunk: int = GEOMETRY_CHUNK):
    """The vertex incidence the geometry entry points take (include/drtk_amd.h, "Mesh geometry"), built with numpy from
    vi [F,3] or [B,F,3]: (crow [B*V+1], entries [3BF], chunk_ptr [B*V+1], chunk_begin [C], chunk_row [C]), int32."""
    import numpy as np

    t = np.asarray(vi, dtype=np.int64)
    t = t[None] if t.ndim == 2 else t
    B, F = t.shape[0], t.shape[1]
    V = int(num_vertices)
    keys = (t + (np.arange(B, dtype=np.int64) * V)[:, None, None]).reshape(-1)
    perm = np.argsort(keys, kind="stable")
    entries = (perm % max(3 * F, 1)).astype(np.int32)
    crow = np.searchsorted(keys[perm], np.arange(B * V + 1), side="left").astype(np.int64)
    length = np.diff(crow)
    nch = np.where(length > chunk, (length + chunk - 1) // chunk, 0)
    chunk_ptr = np.concatenate([[0], np.cumsum(nch)]).astype(np.int64)
    chunk_row = np.repeat(np.arange(B * V), nch)
    chunk_begin = crow[chunk_row] + (np.arange(len(chunk_row)) - chunk_ptr[chunk_row]) * chunk
    return tuple(a.astype(np.int32) for a in (crow, entries, chunk_ptr, chunk_begin, chunk_row))


def _geometry_topology(vi: th.Tensor):
    """int32 vi [F,3] / [B,F,3] -> (contiguous tensor, batch stride in elements, B)"""
    assert vi.dtype == th.int32
    c = vi.contiguous()
    if c.ndim == 2 or c.shape[0] == 1:
        return c, 0, 1
    return c, c.shape[1] * 3, c.shape[0]


@_on_tensor_device
def geometry_face_forward(v, vi, vt=None, vti=None, outputs=("normals", "areas", "edges"), stream=None):
    """v [N,V,3], int32 vi [F,3] / [N,F,3]; with vt [N,T,2] and int32 vti [F,3] also "dpdt", "dpdt_u", "v012".
    Returns {name: tensor} for the requested outputs."""
    v = v.contiguous()
    N, V = v.shape[0], v.shape[1]
    vi_c, vi_sN, _ = _geometry_topology(vi)
    F = vi_c.shape[-2]
    shapes = {"normals": (N, F, 3), "areas": (N, F, 1), "edges": (N, F, 3, 3), "dpdt": (N, F, 2, 3),
              "dpdt_u": (N, F, 3), "v012": (N, F, 3, 3)}
    out = {k: _out(*shapes[k], dtype=v.dtype, device=v.device) for k in outputs}
    vt_c = None if vt is None else vt.contiguous()
    vti_c = None if vti is None else vti.contiguous()
    T = 0 if vt_c is None else vt_c.shape[1]
    _check(
        lib().drtk_amd_geometry_face_forward(
            ctypes.c_int(_dt(v)), _p(v), _i(V * 3), _p(vi_c), _i(vi_sN), _p(vt_c), _i(T * 2), _p(vti_c), _i(N), _i(V),
            _i(T), _i(F), *(_p(out.get(k)) for k in ("normals", "areas", "edges", "dpdt", "dpdt_u", "v012")),
            _stream(v, stream)),
        "geometry_face_forward")
    return out


@_on_tensor_device
def geometry_face_backward(v, vi, vt=None, vti=None, grad_vert=None, vert_sums=None, grad_normals=None,
                           grad_areas=None, grad_edges=None, grad_dpdt=None, grad_v012=None, stream=None):
    """Per-corner gradient rows of the face pass: positions [N,F,3,3] and (with vt) UVs [N,F,3,2] (None otherwise)."""
    v = v.contiguous()
    N, V = v.shape[0], v.shape[1]
    vi_c, vi_sN, _ = _geometry_topology(vi)
    F = vi_c.shape[-2]
    vt_c = None if vt is None else vt.contiguous()
    vti_c = None if vti is None else vti.contiguous()
    T = 0 if vt_c is None else vt_c.shape[1]
    pos = _out(N, F, 3, 3, dtype=v.dtype, device=v.device)
    uv = None if vt_c is None else _out(N, F, 3, 2, dtype=v.dtype, device=v.device)
    c = [None if g is None else g.contiguous() for g in (grad_vert, vert_sums, grad_normals, grad_areas, grad_edges,
                                                          grad_dpdt, grad_v012)]
    _check(
        lib().drtk_amd_geometry_face_backward(
            ctypes.c_int(_dt(v)), _p(v), _i(V * 3), _p(vi_c), _i(vi_sN), _p(vt_c), _i(T * 2), _p(vti_c), _i(N), _i(V),
            _i(T), _i(F), *(_p(g) for g in c), _p(pos), _p(uv), _stream(v, stream)),
        "geometry_face_backward")
    return pos, uv


@_on_tensor_device
def geometry_face_gather(grad_vert, vi, num_faces=None, vert_sums=None, stream=None):
    """[N,F,A] = sum over each face's corners of grad_vert [N,V,A] (through F.normalize's backward with vert_sums)."""
    g = grad_vert.contiguous()
    N, V, A = g.shape
    vi_c, vi_sN, _ = _geometry_topology(vi)
    F = vi_c.shape[-2]
    out = _out(N, F, A, dtype=g.dtype, device=g.device)
    s = None if vert_sums is None else vert_sums.contiguous()
    _check(lib().drtk_amd_geometry_face_gather(ctypes.c_int(_dt(g)), _p(g), _p(s), _p(vi_c), _i(vi_sN), _i(N), _i(V),
                                               _i(F), _i(A), _p(out), _stream(g, stream)),
           "geometry_face_gather")
    return out


@_on_tensor_device
def geometry_vertex_gather(src, incidence, num_vertices, per_corner=False, normalize=False, stream=None):
    """src [N,F,A] (per_corner False) or [N,F,3,A]; incidence = vertex_incidence_numpy(...) as device tensors (or
    numpy arrays, copied here).  Returns out [N,V,A] and, with normalize, the sums [N,V,3] (else None)."""
    src = src.contiguous()
    N, F, A = src.shape[0], src.shape[1], src.shape[-1]
    inc = [th.as_tensor(a, dtype=th.int32, device=src.device).contiguous() for a in incidence]
    crow, entries, chunk_ptr, chunk_begin, chunk_row = inc
    V = int(num_vertices)
    B = (crow.numel() - 1) // V if V else 1
    C = chunk_row.numel()
    out = _out(N, V, A, dtype=src.dtype, device=src.device)
    sums = _out(N, V, 3, dtype=src.dtype, device=src.device) if normalize else None
    need = ctypes.c_size_t(0)
    _check(lib().drtk_amd_geometry_vertex_gather_workspace_bytes(ctypes.c_int(_dt(src)), _i(N), _i(B), _i(C), _i(A),
                                                                 ctypes.byref(need)), "geometry_vertex_gather")
    ws = _out(max(need.value, 1), dtype=th.uint8, device=src.device)
    _check(
        lib().drtk_amd_geometry_vertex_gather(
            ctypes.c_int(_dt(src)), _p(src), _i(F * A * (3 if per_corner else 1)), ctypes.c_int(int(bool(per_corner))),
            _i(A), _p(crow), _p(entries), _p(chunk_ptr if C else None), _p(chunk_begin if C else None),
            _p(chunk_row if C else None), _i(C), _i(B), _i(N), _i(V), _i(F), ctypes.c_int(int(bool(normalize))), _p(out),
            _p(sums), _p(ws), ctypes.c_size_t(need.value), _stream(src, stream)),
        "geometry_vertex_gather")
    return out, sums


@_on_tensor_device
def geometry_cot_weights(v, vi, stream=None):
    """Cotangent weights [N,F,3] of v [N,V,3] over int32 vi [F,3] / [N,F,3]: cot(angle at corner k) / 2, the weight of the
    edge opposite corner k; 0 for a face whose |c| > 0 is false."""
    v = v.contiguous()
    N, V = v.shape[0], v.shape[1]
    vi_c, vi_sN, _ = _geometry_topology(vi)
    F = vi_c.shape[-2]
    w = _out(N, F, 3, dtype=v.dtype, device=v.device)
    _check(lib().drtk_amd_geometry_cot_weights(ctypes.c_int(_dt(v)), _p(v), _i(V * 3), _p(vi_c), _i(vi_sN), _i(N), _i(V),
                                               _i(F), _p(w), _stream(v, stream)), "geometry_cot_weights")
    return w


@_on_tensor_device
def geometry_cot_weights_backward(v, vi, grad_weights, stream=None):
    """Per-corner rows [N,F,3,3] of grad_v from grad_weights [N,F,3]; reduce with geometry_vertex_gather(per_corner=True)."""
    v = v.contiguous()
    N, V = v.shape[0], v.shape[1]
    vi_c, vi_sN, _ = _geometry_topology(vi)
    F = vi_c.shape[-2]
    g = grad_weights.contiguous()
    assert g.shape == (N, F, 3) and g.dtype == v.dtype
    pos = _out(N, F, 3, 3, dtype=v.dtype, device=v.device)
    _check(lib().drtk_amd_geometry_cot_weights_backward(ctypes.c_int(_dt(v)), _p(v), _i(V * 3), _p(vi_c), _i(vi_sN), _i(N),
                                                        _i(V), _i(F), _p(g), _p(pos), _stream(v, stream)),
           "geometry_cot_weights_backward")
    return pos


def _laplacian_weights(weights, x, F):
    """weights None / [F,3] / [1,F,3] / [N,F,3] -> (contiguous tensor or None, view stride in elements, B)"""
    if weights is None:
        return None, 0, 1
    w = weights.contiguous()
    assert w.dtype == x.dtype and w.shape[-2:] == (F, 3)
    if w.ndim == 2 or w.shape[0] == 1:
        return w, 0, 1
    assert w.shape[0] == x.shape[0]
    return w, F * 3, w.shape[0]


@_on_tensor_device
def geometry_laplacian(x, vi, incidence, weights=None, stream=None):
    """out [N,V,C] = sum_j w_ij (x_j - x_i) of x [N,V,C] over int32 vi [F,3] / [N,F,3] and its incidence
    (vertex_incidence_numpy(vi, V), device tensors or numpy arrays); weights [F,3] / [1,F,3] / [N,F,3], or None: every
    face edge weighs 1/2."""
    x = x.contiguous()
    N, V, C = x.shape
    vi_c, vi_sN, B = _geometry_topology(vi)
    F = vi_c.shape[-2]
    inc = [th.as_tensor(a, dtype=th.int32, device=x.device).contiguous() for a in incidence]
    crow, entries, chunk_ptr, chunk_begin, chunk_row = inc
    assert crow.numel() == B * V + 1
    nch = chunk_row.numel()
    w, w_sN, _ = _laplacian_weights(weights, x, F)
    out = _out(N, V, C, dtype=x.dtype, device=x.device)
    need = ctypes.c_size_t(0)
    _check(lib().drtk_amd_geometry_laplacian_workspace_bytes(ctypes.c_int(_dt(x)), _i(N), _i(B), _i(nch), _i(C),
                                                             ctypes.byref(need)), "geometry_laplacian")
    ws = _out(max(need.value, 1), dtype=th.uint8, device=x.device)
    _check(
        lib().drtk_amd_geometry_laplacian(
            ctypes.c_int(_dt(x)), _p(x), _i(C), _p(vi_c), _i(vi_sN), _p(w), _i(w_sN), _p(crow), _p(entries),
            _p(chunk_ptr if nch else None), _p(chunk_begin if nch else None), _p(chunk_row if nch else None), _i(nch),
            _i(B), _i(N), _i(V), _i(F), _p(out), _p(ws), ctypes.c_size_t(need.value), _stream(x, stream)),
        "geometry_laplacian")
    return out


@_on_tensor_device
def geometry_laplacian_grad_weights(grad_out, x, vi, shared_weights=False, stream=None):
    """grad_weights [N,F,3] (shared_weights: [1,F,3], summed over the views in ascending order) of geometry_laplacian."""
    x = x.contiguous()
    g = grad_out.contiguous()
    assert g.shape == x.shape and g.dtype == x.dtype
    N, V, C = x.shape
    vi_c, vi_sN, _ = _geometry_topology(vi)
    F = vi_c.shape[-2]
    wB = 1 if shared_weights else N
    gw = _out(wB, F, 3, dtype=x.dtype, device=x.device)
    _check(lib().drtk_amd_geometry_laplacian_grad_weights(ctypes.c_int(_dt(x)), _p(g), _p(x), _i(C), _p(vi_c), _i(vi_sN),
                                                          _i(N), _i(V), _i(F), _i(wB), _p(gw), _stream(x, stream)),
           "geometry_laplacian_grad_weights")
    return gw


SKIN_CHUNK = 512  # DRTK_SKIN_CHUNK of include/drtk_amd.h
SKIN_MAX_SLOTS = 8  # DRTK_SKIN_MAX_SLOTS


def joint_incidence_numpy(joint_idx, num_joints: int, chunk: int = SKIN_CHUNK):
    """The joint incidence drtk_amd_skin_backward takes (include/drtk_amd.h, "Linear blend skinning"), built with numpy from
    joint_idx [V,K] (-1: empty slot): (crow [J+1], entries, chunk_ptr [J+1], chunk_begin [C], chunk_joint [C]), int32.
    Every row is cut into chunks of `chunk` entries."""
    import numpy as np

    t = np.asarray(joint_idx, dtype=np.int64).reshape(-1)
    J = int(num_joints)
    if t.size and (t.min() < -1 or t.max() >= J):
        raise ValueError(f"joint_idx contains a joint index outside [-1, {J})")
    keys = np.where(t < 0, J, t)
    perm = np.argsort(keys, kind="stable")
    crow = np.searchsorted(keys[perm], np.arange(J + 1), side="left").astype(np.int64)
    nch = (np.diff(crow) + chunk - 1) // chunk
    chunk_ptr = np.concatenate([[0], np.cumsum(nch)]).astype(np.int64)
    chunk_joint = np.repeat(np.arange(J), nch)
    chunk_begin = crow[chunk_joint] + (np.arange(len(chunk_joint)) - chunk_ptr[chunk_joint]) * chunk
    return tuple(a.astype(np.int32) for a in (crow, perm, chunk_ptr, chunk_begin, chunk_joint))


def _skin_args(v, joint_idx, joint_weights, transforms):
    """-> (v contiguous, v_sN, idx, w, transforms read in place or copied, t_sN, t_sJ, N, V, J, K)"""
    assert joint_idx.dtype == th.int32 and joint_idx.dim() == 2
    assert transforms.dim() == 4 and transforms.shape[2] in (3, 4) and transforms.shape[3] == 4
    assert joint_weights.shape == joint_idx.shape and joint_weights.dtype == v.dtype == transforms.dtype
    N, J = transforms.shape[0], transforms.shape[1]
    v = (v[None] if v.dim() == 2 else v).contiguous()
    V, K = joint_idx.shape
    assert v.shape[1:] == (V, 3) and v.shape[0] in (1, N)
    t = transforms
    s = t.stride()
    if not (s[3] == 1 and s[2] == 4 and (J <= 1 or s[1] >= 12) and (N <= 1 or s[0] == 0 or s[0] >= (J - 1) * (s[1] if J > 1 else 0) + 12)):
        t = t.contiguous()
    t_sJ = t.stride(1) if J > 1 else 12
    t_sN = t.stride(0) if N > 1 else 0
    return v, (0 if v.shape[0] == 1 else 3 * V), joint_idx.contiguous(), joint_weights.contiguous(), t, t_sN, t_sJ, N, V, J, K


@_on_tensor_device
def skin_forward(v, joint_idx, joint_weights, transforms, stream=None):
    """out [N,V,3] of v [N,V,3] / [1,V,3] / [V,3], int32 joint_idx [V,K] (entries in [-1, J), NOT checked here),
    joint_weights [V,K] and transforms [N,J,3,4] / [N,J,4,4] (a [..., :3, :] view is read in place)."""
    v, v_sN, idx, w, t, t_sN, t_sJ, N, V, J, K = _skin_args(v, joint_idx, joint_weights, transforms)
    out = _out(N, V, 3, dtype=v.dtype, device=v.device)
    _check(lib().drtk_amd_skin_forward(ctypes.c_int(_dt(v)), _p(v), _i(v_sN), _p(idx), _p(w), _p(t), _i(t_sN), _i(t_sJ),
                                       _i(N), _i(V), _i(J), _i(K), _p(out), _stream(v, stream)), "skin_forward")
    return out


def skin_backward_workspace_bytes(dtype, N, num_chunks) -> int:
    out = ctypes.c_size_t(0)
    code = DRTK_F32 if dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_skin_backward_workspace_bytes(ctypes.c_int(code), _i(N), _i(num_chunks), ctypes.byref(out)),
           "skin_backward")
    return out.value


@_on_tensor_device
def skin_backward(grad_out, v, joint_idx, joint_weights, transforms, incidence=None, grads=("v", "weights", "transforms"),
                  sum_views=None, stream=None):
    """(grad_v, grad_weights, grad_transforms) of skin_forward, None for what `grads` does not name.  `incidence` =
    joint_incidence_numpy(joint_idx, J) (device tensors, or numpy arrays copied here), needed for "transforms".
    grad_v is [1,V,3] (the views' rows added, n ascending) where v was given as one row, else [N,V,3]; `sum_views`
    overrides that.  grad_transforms has the shape of `transforms`."""
    v, v_sN, idx, w, t, t_sN, t_sJ, N, V, J, K = _skin_args(v, joint_idx, joint_weights, transforms)
    g = grad_out.contiguous()
    assert g.shape == (N, V, 3) and g.dtype == v.dtype
    if sum_views is None:
        sum_views = v.shape[0] == 1
    gv_B = 1 if sum_views else N
    gv = _out(gv_B, V, 3, dtype=v.dtype, device=v.device) if "v" in grads else None
    gw = _out(V, K, dtype=v.dtype, device=v.device) if "weights" in grads else None
    gt = ws = None
    rows = transforms.shape[2]
    inc = [None] * 5
    nch = need = 0
    if "transforms" in grads:
        inc = [th.as_tensor(a, dtype=th.int32, device=v.device).contiguous() for a in incidence]
        assert inc[0].numel() == J + 1 and inc[2].numel() == J + 1
        nch = inc[4].numel()
        gt = _out(N, J, rows, 4, dtype=v.dtype, device=v.device)
        need = skin_backward_workspace_bytes(v.dtype, N, nch)
        ws = _out(max(need, 1), dtype=th.uint8, device=v.device)
        assert ws.data_ptr() % 8 == 0
    _check(
        lib().drtk_amd_skin_backward(
            ctypes.c_int(_dt(v)), _p(g), _p(v), _i(v_sN), _p(idx), _p(w), _p(t), _i(t_sN), _i(t_sJ), *(_p(a) for a in inc),
            _i(nch), _i(N), _i(V), _i(J), _i(K), _i(gv_B), _p(gv), _p(gw), _i(rows), _p(gt), _p(ws), ctypes.c_size_t(need),
            _stream(v, stream)),
        "skin_backward")
    return gv, gw, gt


FK_MAX_JOINTS = 320  # DRTK_FK_MAX_JOINTS of include/drtk_amd.h


def kinematic_schedule_numpy(parents):
    """The schedule drtk_amd_kinematics_* take (include/drtk_amd.h, "Forward kinematics"), built with numpy from `parents`
    [J] (-1: a root, else 0 <= parents[j] < j): (parents, order [J], level_start [D+1], child_crow [J+1], child_entries),
    int32.  `order` lists the joints by (depth, index); a joint's children are ascending."""
    import numpy as np

    p = np.asarray(parents)
    if p.ndim != 1 or p.dtype.kind not in "iu":
        raise ValueError("parents: expected a one-dimensional integer array")
    p = p.astype(np.int64)
    J = p.size
    if J and not ((p >= -1) & (p < np.arange(J))).all():
        raise ValueError("parents: expected parents[j] == -1 (a root) or 0 <= parents[j] < j")
    depth = np.zeros(J, dtype=np.int64)
    for j in range(J):
        depth[j] = 0 if p[j] < 0 else depth[p[j]] + 1
    order = np.argsort(depth, kind="stable")
    D = int(depth.max()) + 1 if J else 0
    level_start = np.searchsorted(depth[order], np.arange(D + 1), side="left")
    kids = np.nonzero(p >= 0)[0]
    child_entries = kids[np.argsort(p[kids], kind="stable")]
    child_crow = np.searchsorted(p[child_entries], np.arange(J + 1), side="left")
    return tuple(a.astype(np.int32) for a in (p, order, level_start, child_crow, child_entries))


def _kinematics_args(rotations, joints, translation, schedule):
    """-> (rot_is_matrix, strides array, joints contiguous, c_sN, translation, schedule tensors on the device, N, J, D)"""
    assert rotations.dim() in (3, 4) and rotations.shape[2:] in ((3,), (3, 3)), rotations.shape
    N, J = rotations.shape[0], rotations.shape[1]
    mat = rotations.dim() == 4
    st = list(rotations.stride()) + ([0] if not mat else [])
    strides = (ctypes.c_int64 * 4)(*st)
    assert joints.dtype == rotations.dtype and joints.shape in ((J, 3), (1, J, 3), (N, J, 3)), joints.shape
    c = joints.reshape(-1, J, 3).contiguous()
    c_sN = 0 if c.shape[0] == 1 else 3 * J  # (one view: one row either way)
    if translation is not None:
        assert translation.shape == (N, 3) and translation.dtype == rotations.dtype
        translation = translation.contiguous()
    sch = [th.as_tensor(a, dtype=th.int32, device=rotations.device).contiguous() for a in schedule]
    assert sch[0].numel() == J and sch[1].numel() == J and sch[3].numel() == J + 1
    D = sch[2].numel() - 1
    return int(mat), strides, c, c_sN, translation, sch, N, J, D


@_on_tensor_device
def kinematics_forward(rotations, joints, schedule, translation=None, stream=None):
    """(transforms [N,J,3,4], posed_joints [N,J,3]) of rotations [N,J,3] / [N,J,3,3] (read through their strides), joints
    [J,3] / [1,J,3] (shared) or [N,J,3], `schedule` = kinematic_schedule_numpy(parents) and translation [N,3] or None."""
    mat, strides, c, c_sN, tr, sch, N, J, D = _kinematics_args(rotations, joints, translation, schedule)
    out_t = _out(N, J, 3, 4, dtype=rotations.dtype, device=rotations.device)
    out_p = _out(N, J, 3, dtype=rotations.dtype, device=rotations.device)
    _check(lib().drtk_amd_kinematics_forward(ctypes.c_int(_dt(rotations)), _p(rotations), ctypes.c_int(mat), strides, _p(c), _i(c_sN),
                                             _p(tr), _p(sch[0]), _p(sch[1]), _p(sch[2]), _i(D), _i(N), _i(J), _p(out_t), _p(out_p),
                                             _stream(rotations, stream)), "kinematics_forward")
    return out_t, out_p


def kinematics_backward_workspace_bytes(dtype, N, J, grad_joints_B) -> int:
    out = ctypes.c_size_t(0)
    code = DRTK_F32 if dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_kinematics_backward_workspace_bytes(ctypes.c_int(code), _i(N), _i(J), _i(grad_joints_B), ctypes.byref(out)),
           "kinematics_backward")
    return out.value


@_on_tensor_device
def kinematics_backward(grad_transforms, grad_posed, rotations, joints, schedule, translation=None,
                        grads=("rotations", "joints", "translation"), stream=None):
    """(grad_rotations, grad_joints, grad_translation) of kinematics_forward, None for what `grads` does not name (and
    grad_translation without a translation).  Either of grad_transforms / grad_posed may be None (zero).  grad_joints is
    [1,J,3] (the views' rows added, n ascending, in double) where the joints were given as one row, else [N,J,3]."""
    mat, strides, c, c_sN, tr, sch, N, J, D = _kinematics_args(rotations, joints, translation, schedule)
    dt, dev = rotations.dtype, rotations.device
    gA = None if grad_transforms is None else grad_transforms.contiguous()
    gP = None if grad_posed is None else grad_posed.contiguous()
    assert gA is None or (gA.shape == (N, J, 3, 4) and gA.dtype == dt)
    assert gP is None or (gP.shape == (N, J, 3) and gP.dtype == dt)
    gr = _out(*rotations.shape, dtype=dt, device=dev) if "rotations" in grads else None
    gc_B = 1 if c_sN == 0 else N
    gc = _out(gc_B, J, 3, dtype=dt, device=dev) if "joints" in grads else None
    gt = _out(N, 3, dtype=dt, device=dev) if "translation" in grads and tr is not None else None
    need = kinematics_backward_workspace_bytes(dt, N, J, gc_B if gc is not None else 0)
    ws = _out(max(need, 1), dtype=th.uint8, device=dev)
    assert ws.data_ptr() % 8 == 0
    _check(
        lib().drtk_amd_kinematics_backward(
            ctypes.c_int(_dt(rotations)), _p(gA), _p(gP), _p(rotations), ctypes.c_int(mat), strides, _p(c), _i(c_sN), _p(tr),
            _p(sch[0]), _p(sch[1]), _p(sch[2]), _i(D), _p(sch[3]), _p(sch[4]), _i(N), _i(J), _p(gr), _i(gc_B), _p(gc), _p(gt),
            _p(ws), ctypes.c_size_t(need), _stream(rotations, stream)),
        "kinematics_backward")
    return gr, gc, gt


# DRTK_NEAREST_* of include/drtk_amd.h
NEAREST_R = 4
NEAREST_QUERIES = 1024
NEAREST_TILE = 1024
NEAREST_SPLIT_BLOCKS = 512
NEAREST_CHUNK = 256


def nearest_split(N, P, M) -> Tuple[int, int]:
    """(S, L) of the launch rule of drtk_amd_nearest_forward (include/drtk_amd.h): S ranges of L targets."""
    cd = lambda a, b: -(-a // b)  # noqa: E731
    B = N * cd(P, NEAREST_QUERIES)
    if B <= 0 or B >= NEAREST_SPLIT_BLOCKS or M <= NEAREST_TILE:
        return 1, M
    S0 = min(cd(NEAREST_SPLIT_BLOCKS, B), cd(M, NEAREST_TILE))
    L = cd(cd(M, S0), NEAREST_TILE) * NEAREST_TILE
    return cd(M, L), L


def _points(t):
    """-> (tensor read in place or copied, sN, sP, B, count) of points [B,count,3] / [count,3], B = 1 or N"""
    assert t.dim() in (2, 3) and t.shape[-1] == 3
    t = t[None] if t.dim() == 2 else t
    if t.shape[0] > 1 and t.stride(0) == 0:
        t = t[:1]
    B, count = t.shape[0], t.shape[1]
    s = t.stride()
    if not (s[2] == 1 and (count <= 1 or s[1] >= 3) and (B <= 1 or s[0] >= (count - 1) * (s[1] if count > 1 else 0) + 3)):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else 0), (t.stride(1) if count > 1 else 3), B, count


def _nearest_args(p, q):
    assert p.dtype == q.dtype and p.device == q.device
    N = max((p.shape[0] if p.dim() == 3 else 1), (q.shape[0] if q.dim() == 3 else 1))
    p, p_sN, p_sP, pB, P = _points(p)
    q, q_sN, q_sM, qB, M = _points(q)
    assert pB in (1, N) and qB in (1, N)
    return p, p_sN, p_sP, q, q_sN, q_sM, N, P, M


def nearest_forward_workspace_bytes(dtype, N, P, M) -> int:
    out = ctypes.c_size_t(0)
    code = DRTK_F32 if dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_nearest_forward_workspace_bytes(ctypes.c_int(code), _i(N), _i(P), _i(M), ctypes.byref(out)),
           "nearest_forward")
    return out.value


def nearest_backward_workspace_bytes(dtype, N, P, M, need_grad_q=True) -> int:
    out = ctypes.c_size_t(0)
    code = DRTK_F32 if dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_nearest_backward_workspace_bytes(ctypes.c_int(code), _i(N), _i(P), _i(M),
                                                           ctypes.c_int(int(need_grad_q)), ctypes.byref(out)), "nearest_backward")
    return out.value


@_on_tensor_device
def nearest_forward(p, q, stream=None):
    """(dist2 [N,P], idx int32 [N,P]) of p [N,P,3] / [1,P,3] / [P,3] and q likewise (N the larger batch); a `[..., :3]`
    view of a wider tensor is read in place."""
    p, p_sN, p_sP, q, q_sN, q_sM, N, P, M = _nearest_args(p, q)
    dist2 = _out(N, P, dtype=p.dtype, device=p.device)
    idx = _out(N, P, dtype=th.int32, device=p.device)
    need = nearest_forward_workspace_bytes(p.dtype, N, P, M)
    ws = _out(need, dtype=th.uint8, device=p.device) if need else None
    assert ws is None or ws.data_ptr() % 8 == 0
    _check(lib().drtk_amd_nearest_forward(ctypes.c_int(_dt(p)), _p(p), _i(p_sN), _i(p_sP), _p(q), _i(q_sN), _i(q_sM), _i(N),
                                          _i(P), _i(M), _p(dist2), _p(idx), _p(ws), ctypes.c_size_t(need), _stream(p, stream)),
           "nearest_forward")
    return dist2, idx


@_on_tensor_device
def nearest_backward(grad_dist2, p, q, idx, order=None, grads=("p", "q"), stream=None):
    """(grad_p, grad_q) of nearest_forward, None for what `grads` does not name; each has the batch of its input (1: the
    views added).  `order`: int32 [N,P], per view the STABLE ascending argsort of idx (needed for "q"; made here with
    torch's stable sort when not given)."""
    pB = p.shape[0] if p.dim() == 3 else 1
    qB = q.shape[0] if q.dim() == 3 else 1
    p, p_sN, p_sP, q, q_sN, q_sM, N, P, M = _nearest_args(p, q)
    g = grad_dist2.contiguous()
    idx = idx.contiguous()
    assert g.shape == (N, P) and g.dtype == p.dtype and idx.shape == (N, P) and idx.dtype == th.int32
    gp = _out(pB, P, 3, dtype=p.dtype, device=p.device) if "p" in grads else None
    gq = ws = None
    need = 0
    if "q" in grads:
        gq = _out(qB, M, 3, dtype=p.dtype, device=p.device)
        if order is None:
            order = th.sort(idx, dim=1, stable=True).indices
        order = order.to(th.int32).contiguous()
        assert order.shape == (N, P)
        need = nearest_backward_workspace_bytes(p.dtype, N, P, M)
        ws = _out(max(need, 1), dtype=th.uint8, device=p.device)
        assert ws.data_ptr() % 8 == 0
    _check(lib().drtk_amd_nearest_backward(ctypes.c_int(_dt(p)), _p(g), _p(p), _i(p_sN), _i(p_sP), _p(q), _i(q_sN), _i(q_sM),
                                           _p(idx), _p(order), _i(N), _i(P), _i(M), _i(pB), _p(gp), _i(qB), _p(gq), _p(ws),
                                           ctypes.c_size_t(need), _stream(p, stream)), "nearest_backward")
    return gp, gq


def edge_grad_backward_workspace_bytes(dtype, N, H, W) -> int:
    out = ctypes.c_size_t(0)
    code = DRTK_F32 if dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_edge_grad_backward_workspace_bytes(ctypes.c_int(code), _i(N), _i(H), _i(W), ctypes.byref(out)),
           "edge_grad_backward")
    return out.value


@_on_tensor_device
def edge_grad_backward(v_pix, img, index_img, vi, grad_output, max_dp_dr=1e4, stream=None, workspace=None):
    v_pix = v_pix.contiguous()
    img = img.contiguous()
    index_img = index_img.contiguous()
    grad_output = grad_output.contiguous()
    N, V, _ = v_pix.shape
    C, H, W = img.shape[1:]
    vi_c, vi_sN, F = _vi(vi, N)
    out = _out(N, 3, H, W, dtype=v_pix.dtype, device=v_pix.device)
    nbytes = edge_grad_backward_workspace_bytes(v_pix.dtype, N, H, W)
    ws = workspace if workspace is not None else _out(nbytes, dtype=th.uint8, device=v_pix.device)
    _check(
        lib().drtk_amd_edge_grad_backward(
            ctypes.c_int(_dt(v_pix)), _p(v_pix), _p(img), _p(index_img), _p(vi_c), _p(grad_output), _i(N), _i(V),
            _i(C), _i(F), _i(vi_sN), _i(H), _i(W), ctypes.c_double(max_dp_dr), _p(out), _p(ws),
            ctypes.c_size_t(ws.numel()), _stream(v_pix, stream)),
        "edge_grad_backward")
    return out


@_on_tensor_device
def edge_grad_backward_fused(v_pix, img, index_img, vi, bary_img, grad_output, max_dp_dr=1e4, stream=None):
    """grad_v_pix [N,V,3] = interpolate_backward(edge_grad_backward(...), v_pix, ...) in one call."""
    v_pix = v_pix.contiguous()
    img = img.contiguous()
    index_img = index_img.contiguous()
    bary_img = bary_img.contiguous()
    grad_output = grad_output.contiguous()
    N, V, _ = v_pix.shape
    C, H, W = img.shape[1:]
    vi_c, vi_sN, F = _vi(vi, N)
    out = _out(N, V, 3, dtype=v_pix.dtype, device=v_pix.device)
    nb = ctypes.c_size_t(0)
    code = DRTK_F32 if v_pix.dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_edge_grad_backward_fused_workspace_bytes(ctypes.c_int(code), _i(N), _i(H), _i(W), ctypes.byref(nb)),
           "edge_grad_backward_fused")
    ws = _out(nb.value, dtype=th.uint8, device=v_pix.device)
    _check(
        lib().drtk_amd_edge_grad_backward_fused(
            ctypes.c_int(_dt(v_pix)), _p(v_pix), _p(img), _p(index_img), _p(vi_c), _p(bary_img), _p(grad_output),
            _i(N), _i(V), _i(C), _i(F), _i(vi_sN), _i(H), _i(W), ctypes.c_double(max_dp_dr), _p(out), _p(ws),
            ctypes.c_size_t(ws.numel()), _stream(v_pix, stream)),
        "edge_grad_backward_fused")
    return out


def selftest_exact_div(dtype=th.float32, seed=1, count=1 << 28, device="cuda:0") -> int:
    """Number of (n, d) pairs for which the rasterizer's exact division differs from IEEE `/` (must be 0)."""
    out = th.zeros(1, dtype=th.int64, device=device)
    code = DRTK_F32 if dtype == th.float32 else DRTK_F64
    _check(lib().drtk_amd_selftest_exact_div(ctypes.c_int(code), ctypes.c_uint64(seed), _i(count), _p(out),
                                             _stream(out, None)), "selftest_exact_div")
    return int(out.item())


def kernel_timing_begin() -> None:
    """Open a per-kernel timing collection: until `kernel_timing_report()` every kernel the library launches (through
    this module or through the torch operators -- same library) is bracketed by HIP events on its launch stream."""
    _check(lib().drtk_amd_kernel_timing_begin(), "kernel_timing_begin")


def kernel_timing_report() -> dict:
    """Close the collection and return {launch-site kernel name: (launches, total_ms)} in order of first launch."""
    need = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(1 << 16)
    _check(lib().drtk_amd_kernel_timing_report(buf, ctypes.c_size_t(len(buf)), ctypes.byref(need)), "kernel_timing_report")
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms = line.rsplit("\t", 2)
        out[name.strip("()")] = (int(count), float(ms))
    return out
