"""`transform` -- the step before the hot path (drtk/transform.py:13-119, drtk/utils/projection.py:33-310,486-646).
Same signature as the reference.  On a HIP device, when neither the camera parameters nor the distortion inputs require
gradients, `transform` runs as ONE fused kernel each way: `drtk_amd_ext::transform_pinhole` (csrc/transform.hip) for the
undistorted pinhole model, `drtk_amd_ext::transform_distort` (csrc/transform_distort.hip) for the radial-tangential,
fisheye and fisheye62 (+ lookup table) models and per-view lists of them; otherwise the PyTorch formulation below is
used, which also provides the camera, coefficient and lookup-table gradients.

The distortion models run on the HIP device only: like every operator of this package they have no computing CPU path,
and `transform` with a non-pinhole `distortion_mode` on CPU tensors raises NotImplementedError.  With `fov=None` the
bound is estimated on the host from the coefficients (`estimate_*_fov`, numpy root finding as in the reference): that
reads `distortion_coeff` back, so it synchronises and cannot be captured into a HIP graph -- pass `fov` to capture."""
from typing import List, Optional, Tuple, Union

import numpy as np
import torch as th

DISTORTION_MODES = {None, "pinhole", "radial-tangential", "fisheye"}  # what a per-view list may hold (projection.py:13-18)
_FISHEYE62_MODES = {"fisheye62", "fisheye62_lut"}  # single-string modes only (projection.py:20)
_MODE_IDS = {None: 0, "pinhole": 0, "radial-tangential": 1, "fisheye": 2, "fisheye62": 3, "fisheye62_lut": 3}  # include/drtk_amd.h


def _invalid_mode(distortion_mode):
    return ValueError(f"Invalid distortion mode: {distortion_mode}. Valid options: {DISTORTION_MODES}.")


def _resolve_mode(distortion_mode, distortion_coeff):
    """The reference's mode handling (utils/projection.py:533-616): the mode as None (pinhole), one string, or a list of
    at least two distinct entries of DISTORTION_MODES."""
    if distortion_mode is not None:
        assert distortion_coeff is not None, "Missing distortion coefficients."
    if isinstance(distortion_mode, (list, tuple)):
        distinct = set(distortion_mode)
        if len(distinct) == 0:
            return None
        if len(distinct) == 1:
            distortion_mode = next(iter(distinct))
        else:
            if distinct <= {None, "pinhole"}:
                return None
            if not distinct <= DISTORTION_MODES:
                raise _invalid_mode(distortion_mode)
            return list(distortion_mode)
    if distortion_mode is None or distortion_mode == "pinhole":
        return None
    if not isinstance(distortion_mode, str) or distortion_mode not in _MODE_IDS:
        raise _invalid_mode(distortion_mode)
    return distortion_mode


def _check_coeff(mode, D: th.Tensor) -> None:
    modes = set(mode) if isinstance(mode, list) else {mode}
    assert D.dim() == 2, f"distortion_coeff must be [N, ncoef]: {D.shape}"
    if "radial-tangential" in modes:
        assert D.shape[1] in [4, 5, 8]
    if "fisheye" in modes:
        assert D.shape[1] >= 4, f"Fisheye model requires 4 distortion parameters: {D.shape}"
    if modes & _FISHEYE62_MODES:
        assert D.shape[1] == 8, f"Fisheye62 model requires 8 distortion parameters: {D.shape}"


# ---- field-of-view estimates (projection.py:312-482): host code, numpy root finding, not differentiable ----------------
def _first_positive_root(poly) -> Optional[float]:
    roots = np.roots(poly)
    real = roots.real[abs(roots.imag) < 1e-5]
    real = real[real > 0]
    return real.min() if len(real) else None


def _as_rows(D):
    return D.cpu().numpy() if th.is_tensor(D) else D


def _like_coeff(fov, D):
    fov = np.asarray(fov, dtype=np.float32)[..., None]  # float32 whatever the coefficients are, as the reference has it
    return th.from_numpy(fov).to(D) if th.is_tensor(D) else fov


def _odd_derivative(k, count):
    """Rows of d/dx (x + k[0] x^3 + k[1] x^5 + ...) with `count` coefficients, highest power first, in k's dtype."""
    zeros = np.zeros_like(k[:, 0])
    cols = []
    for j in reversed(range(count)):
        cols += [(2 * j + 3) * k[:, j], zeros]
    return np.stack(cols + [np.ones_like(k[:, 0])], axis=-1)


def estimate_rt_fov(D: Union[np.ndarray, th.Tensor]) -> th.Tensor:
    """`[N,1]`: the smallest positive radius at which r (1 + k1 r^2 + k2 r^4) stops growing, +inf if there is none.
    Reads the first two coefficients of `D [N, >=2]`."""
    rows = _odd_derivative(_as_rows(D), 2)
    roots = [_first_positive_root(p) for p in rows]
    return _like_coeff([np.inf if r is None else r for r in roots], D)


def _fisheye_fov(D, count):
    rows = _odd_derivative(_as_rows(D), count)
    roots = [_first_positive_root(p) for p in rows]
    return _like_coeff(np.tan([np.pi / 2 if r is None else min(r, np.pi / 2) for r in roots]), D)


def estimate_fisheye_fov(D: Union[np.ndarray, th.Tensor]) -> th.Tensor:
    """`[N,1]`: tan of the smallest positive angle (at most pi/2) at which the fisheye polynomial theta_d(theta) with
    the first four coefficients of `D` stops growing.  `transform` uses it for fisheye AND fisheye62, as the reference does."""
    return _fisheye_fov(D, 4)


def estimate_fisheye62_fov(D: Union[np.ndarray, th.Tensor]) -> th.Tensor:
    """As `estimate_fisheye_fov` with all six radial coefficients of the fisheye62 model (`D [N, >=6]`)."""
    assert _as_rows(D).shape[-1] >= 6, f"fisheye62 FOV requires at least 6 coefficients, got shape {_as_rows(D).shape}"
    return _fisheye_fov(D, 6)


def _resolve_fov(mode, D: th.Tensor, fov: Optional[th.Tensor]) -> th.Tensor:
    """`[N,1]` in D's dtype on D's device.  None: estimated on the host per view by its own mode (synchronises)."""
    N = D.shape[0]
    if fov is not None:
        return fov.to(D).reshape(N, 1)
    with th.no_grad():
        if isinstance(mode, list):
            out = th.full((N, 1), float("inf"), dtype=D.dtype)
            Dh = D.detach().cpu()
            for name, est in (("radial-tangential", estimate_rt_fov), ("fisheye", estimate_fisheye_fov)):
                rows = [i for i, m in enumerate(mode) if m == name]
                if rows:
                    out[rows] = est(Dh[rows])
            return out.to(D.device)
        return (estimate_rt_fov if mode == "radial-tangential" else estimate_fisheye_fov)(D.detach())


# ---- the PyTorch formulation -------------------------------------------------------------------------------------------
def _clamp_z(z: th.Tensor) -> th.Tensor:
    return th.where(z < 0, z.clamp(max=-1e-8), z.clamp(min=1e-8))


def _to_pixels(p: th.Tensor, focal: th.Tensor, princpt: th.Tensor) -> th.Tensor:
    # focal @ p per vertex, written as ONE [N,V,2]x[N,2,2] batched product: the reference's
    # per-vertex `focal[:, None] @ v_proj[..., None]` launches a degenerate N*V-batch GEMM that
    # takes milliseconds on ROCm.
    return th.bmm(p, focal.transpose(1, 2)) + princpt[:, None]


def project_pinhole(v_cam: th.Tensor, focal: th.Tensor, princpt: th.Tensor) -> th.Tensor:
    return _to_pixels(v_cam[:, :, 0:2] / _clamp_z(v_cam[:, :, 2:3]), focal, princpt)


def _project_rt(v_cam, focal, princpt, D, fov):
    """projection.py:87-135.  fov [N,1]."""
    p = v_cam[:, :, :2] / _clamp_z(v_cam[:, :, 2:3])
    r2 = (p * p).sum(-1).clamp(max=fov * fov)  # [N,V]
    pc = p.clamp(min=-fov[..., None], max=fov[..., None])  # the tangential terms see p clamped per component
    k1, k2, p1, p2 = (D[:, i:i + 1] for i in range(4))
    R = 1 + k1 * r2 + k2 * r2.pow(2)
    if D.shape[1] >= 5:  # a 4-coefficient call never forms r2^3 (fov = inf: it overflows on the camera plane)
        R = R + D[:, 4:5] * r2.pow(3)
    if D.shape[1] == 8:
        R = R / (1 + D[:, 5:6] * r2 + D[:, 6:7] * r2.pow(2) + D[:, 7:8] * r2.pow(3))
    x, y = pc[..., 0], pc[..., 1]
    tx = 2 * x * y * p1 + r2 * p2 + 2 * p2 * x * x
    ty = 2 * x * y * p2 + r2 * p1 + 2 * p1 * y * y
    return _to_pixels(p * R[..., None] + th.stack((tx, ty), dim=-1), focal, princpt)


def _fisheye_scaled(v_cam, D, fov, count):
    """(x/z, y/z) * theta_d(atan r) / r with r clamped to [1e-8, fov] and `count` radial coefficients."""
    p = v_cam[:, :, :2] / _clamp_z(v_cam[:, :, 2:3])
    r = (p * p).sum(-1).sqrt().clamp(max=fov, min=1e-8 * th.ones_like(fov))
    theta = th.atan(r)
    t2 = theta * theta
    poly, tp = 1, 1
    for k in range(count):
        tp = tp * t2
        poly = poly + D[:, k:k + 1] * tp
    return p * (theta * poly / r)[..., None]


def _project_fisheye(v_cam, focal, princpt, D, fov):
    """projection.py:165-183."""
    return _to_pixels(_fisheye_scaled(v_cam, D, fov, 4), focal, princpt)


def _project_fisheye62(v_cam, focal, princpt, D, fov, lut, lut_spacing):
    """projection.py:224-309."""
    q = _fisheye_scaled(v_cam, D, fov, 6).clamp(min=-fov[..., None], max=fov[..., None])
    x, y = q[..., 0], q[..., 1]
    p0, p1 = D[:, 6:7], D[:, 7:8]
    rr = x * x + y * y
    tx = (2 * x * x + rr) * p0 + (2 * x * y) * p1
    ty = (2 * x * y) * p0 + (2 * y * y + rr) * p1
    pix = _to_pixels(q + th.stack((tx, ty), dim=-1), focal, princpt)
    if lut is None:
        return pix
    assert lut_spacing is not None, "lookup table spacing must be provided along with vector field"
    # the reference normalises x by size(2) - 1 and y by size(3) - 1, while grid_sample reads x along size(3)
    size = th.tensor([lut.shape[2] - 1, lut.shape[3] - 1], dtype=pix.dtype).to(pix.device)
    pos = pix / lut_spacing[:, None, :] / size * 2.0 - 1.0
    off = th.nn.functional.grid_sample(lut, pos.unsqueeze(1), align_corners=True)[:, :, 0].transpose(1, 2)
    outside = ((pos < -1.0) | (pos > 1.0)).any(-1, keepdim=True)
    return pix + th.where(outside, th.zeros_like(off), off)


_index_cache = {}


def _rows_of(mode_list, names, device) -> th.Tensor:
    key = (tuple(mode_list), names, str(device))
    if key not in _index_cache:
        _index_cache[key] = th.tensor([i for i, m in enumerate(mode_list) if m in names], dtype=th.long).to(device)
    return _index_cache[key]


def _transform_torch(v, campos, camrot, focal, princpt, mode, D, fov, lut, lut_spacing, cull) -> Tuple[th.Tensor, th.Tensor]:
    """The package's PyTorch formulation of `project_points` (projection.py:486-646) on any device: `mode` as
    `_resolve_mode` returns it, `fov [N,1]` resolved, `cull`: the caller passed a fov (fisheye62 only)."""
    # camrot @ (v - campos) per vertex as one [N,V,3]x[N,3,3] batched product (see _to_pixels)
    v_cam = th.bmm(v - campos[:, None], camrot.transpose(1, 2))
    if mode is None:
        xy = project_pinhole(v_cam, focal, princpt)
    elif mode == "radial-tangential":
        xy = _project_rt(v_cam, focal, princpt, D, fov)
    elif mode == "fisheye":
        xy = _project_fisheye(v_cam, focal, princpt, D, fov)
    elif isinstance(mode, str):
        xy = _project_fisheye62(v_cam, focal, princpt, D, fov, lut, lut_spacing)
    else:
        xy = th.empty_like(v_cam[..., :2])
        for names, fn in (((None, "pinhole"), None), (("radial-tangential",), _project_rt), (("fisheye",), _project_fisheye)):
            idx = _rows_of(mode, names, v.device)
            if idx.numel() == 0:
                continue
            sub = (v_cam[idx], focal[idx], princpt[idx])
            xy = xy.index_put((idx,), project_pinhole(*sub) if fn is None else fn(*sub, D[idx], fov[idx]))
    z = v_cam[:, :, 2:3]
    if cull:  # projection.py:623-642 (fisheye62 with a fov given by the caller)
        r_raw = (v_cam[:, :, :2] / _clamp_z(z)).pow(2).sum(-1, keepdim=True).sqrt()
        z = th.where(r_raw > fov.view(-1, 1, 1), th.full_like(z, -1.0), z)
    return th.cat((xy, z), dim=-1), v_cam


# ---- dispatch ------------------------------------------------------------------------------------------------------------
_mode_tensor_cache = {}


def _mode_tensor(mode_list, device) -> th.Tensor:
    """int32 [N] mode ids on `device`, cached per (modes, device): a second call -- and a graph capture after a
    warm-up call -- copies nothing."""
    key = (tuple(mode_list), str(device))
    if key not in _mode_tensor_cache:
        _mode_tensor_cache[key] = th.tensor([_MODE_IDS[m] for m in mode_list], dtype=th.int32).to(device)
    return _mode_tensor_cache[key]


def _cameras(campos, camrot, focal, princpt, K, Rt):
    if not ((camrot is not None and campos is not None) ^ (Rt is not None)):
        raise ValueError("You must provide exactly one of Rt or (campos, camrot).")
    if not ((focal is not None and princpt is not None) ^ (K is not None)):
        raise ValueError("You must provide exactly one of K or (focal, princpt).")
    if campos is None:
        camrot = Rt[:, :3, :3]
        campos = -(camrot.transpose(-2, -1) @ Rt[:, :3, 3:4])[..., 0]
    if focal is None:
        focal = K[:, :2, :2]
        princpt = K[:, :2, 2]
    return campos, camrot, focal, princpt


def _distortion_inputs(mode, D, fov, lut, lut_spacing):
    """Checks of the coefficient table and the resolved `(fov [N,1], lut, lut_spacing, cull)` of a non-pinhole `mode`."""
    _check_coeff(mode, D)
    cull = fov is not None and isinstance(mode, str) and mode in _FISHEYE62_MODES  # an estimated fov does not cull
    fov = _resolve_fov(mode, D, fov)
    if not (isinstance(mode, str) and mode in _FISHEYE62_MODES):
        lut = lut_spacing = None  # only fisheye62 reads the table (projection.py:560-569)
    elif lut is not None:
        assert lut_spacing is not None, "lookup table spacing must be provided along with vector field"
    return fov, lut, lut_spacing, cull


def _transform_torch_route(v, campos, camrot, focal, princpt, distortion_mode=None, distortion_coeff=None, fov=None,
                           lut_vector_field=None, lut_spacing=None) -> Tuple[th.Tensor, th.Tensor]:
    """`project_points` of the reference in this package's PyTorch formulation, on any device (the tests evaluate it on
    the CPU against the reference's fixtures; `transform` takes it on the HIP device when a camera parameter, the
    coefficients or the lookup table require a gradient)."""
    mode = _resolve_mode(distortion_mode, distortion_coeff)
    if mode is None:
        return _transform_torch(v, campos, camrot, focal, princpt, None, None, None, None, None, False)
    return _transform_torch(v, campos, camrot, focal, princpt, mode, distortion_coeff,
                            *_distortion_inputs(mode, distortion_coeff, fov, lut_vector_field, lut_spacing))


def _transform_distorted(v, cams, mode, D, fov, lut, lut_spacing, need_v_cam):
    """A non-pinhole `mode` (as `_resolve_mode` returns it): the fused operator on a HIP device when only `v` may require a
    gradient, the PyTorch formulation otherwise."""
    if not (v.is_cuda and v.dtype in (th.float32, th.float64)):
        raise NotImplementedError(
            f"drtk_amd.transform implements the pinhole camera only on CPU tensors; distortion_mode={mode!r} "
            "(radial-tangential / fisheye / fisheye62 of drtk.utils.projection) runs on the HIP device (float32 or "
            "float64 tensors), like every operator of this package -- there is no computing CPU path")
    fov, lut, lut_spacing, cull = _distortion_inputs(mode, D, fov, lut, lut_spacing)
    params = (*cams, D, fov, lut, lut_spacing)
    if th.is_grad_enabled() and any(t is not None and t.requires_grad for t in params):
        return _transform_torch(v, *cams, mode, D, fov, lut, lut_spacing, cull)
    from drtk_amd.utils import load_torch_ops

    load_torch_ops("drtk.rasterize_ext")
    if v.shape[0] != 1 and v.stride(0) == 0:
        v = v[:1]  # expanded world-space vertices: keep them shared, the kernel broadcasts
    per_view = isinstance(mode, list)
    if D.shape[1] not in (4, 5, 8):
        D = D[:, :4]  # fisheye alone reads four coefficients of however many there are
    return th.ops.drtk_amd_ext.transform_distort(
        v, *cams, 0 if per_view else _MODE_IDS[mode], _mode_tensor(mode, v.device) if per_view else None, D, fov, cull,
        lut, lut_spacing, need_v_cam)


def transform_with_v_cam(
    v: th.Tensor,
    campos: Optional[th.Tensor] = None,
    camrot: Optional[th.Tensor] = None,
    focal: Optional[th.Tensor] = None,
    princpt: Optional[th.Tensor] = None,
    K: Optional[th.Tensor] = None,
    Rt: Optional[th.Tensor] = None,
    distortion_mode: Optional[Union[List[str], str]] = None,
    distortion_coeff: Optional[th.Tensor] = None,
    fov: Optional[th.Tensor] = None,
    lut_vector_field: Optional[th.Tensor] = None,
    lut_spacing: Optional[th.Tensor] = None,
) -> Tuple[th.Tensor, th.Tensor]:
    """`(v_pix, v_cam)` -- `transform` and the camera-space vertices.  Signature of drtk/transform.py:66-79; the
    distortion modes as in `transform`, `lut_vector_field [N,2,H_lut,W_lut]` / `lut_spacing [N,2]` for fisheye62."""
    cams = _cameras(campos, camrot, focal, princpt, K, Rt)
    mode = _resolve_mode(distortion_mode, distortion_coeff)
    if mode is not None:
        return _transform_distorted(v, cams, mode, distortion_coeff, fov, lut_vector_field, lut_spacing, True)
    campos, camrot, focal, princpt = cams
    # camrot @ (v - campos) per vertex as one [N,V,3]x[N,3,3] batched product (see project_pinhole)
    v_cam = th.bmm(v - campos[:, None], camrot.transpose(1, 2))
    v_pix = project_pinhole(v_cam, focal, princpt)
    return th.cat((v_pix, v_cam[:, :, 2:3]), dim=-1), v_cam


def transform(
    v: th.Tensor,
    campos: Optional[th.Tensor] = None,
    camrot: Optional[th.Tensor] = None,
    focal: Optional[th.Tensor] = None,
    princpt: Optional[th.Tensor] = None,
    K: Optional[th.Tensor] = None,
    Rt: Optional[th.Tensor] = None,
    distortion_mode: Optional[Union[List[str], str]] = None,
    distortion_coeff: Optional[th.Tensor] = None,
    fov: Optional[th.Tensor] = None,
) -> th.Tensor:
    """World space `[N,V,3]` (or one shared `[1,V,3]`) -> `(x_pix, y_pix, z_cam)`;
    `v_cam = camrot @ (v - campos)`.  Signature of drtk/transform.py:13-24.

    `distortion_mode`: None / "pinhole", "radial-tangential" (`distortion_coeff [N,4|5|8]`), "fisheye" (`[N,4]`),
    "fisheye62" / "fisheye62_lut" (`[N,8]`), or a per-view list of the first three.  The distortion models need HIP
    tensors.  `fov [N,1]`: the largest normalised radius; None estimates it on the host from the coefficients, which
    synchronises -- pass `fov` to capture the call into a HIP graph.  With fisheye62 and a `fov` given, vertices
    beyond it get z = -1 so that the rasterizer culls their triangles."""
    if v.is_cuda and v.dtype in (th.float32, th.float64):
        cams = _cameras(campos, camrot, focal, princpt, K, Rt)
        mode = _resolve_mode(distortion_mode, distortion_coeff)
        if mode is not None:
            return _transform_distorted(v, cams, mode, distortion_coeff, fov, None, None, False)[0]
        if not (th.is_grad_enabled() and any(c.requires_grad for c in cams)):
            from drtk_amd.utils import load_torch_ops

            load_torch_ops("drtk.rasterize_ext")
            if v.shape[0] != 1 and v.stride(0) == 0:
                v = v[:1]  # expanded world-space vertices: keep them shared, the kernel broadcasts
            return th.ops.drtk_amd_ext.transform_pinhole(v, *cams)
        return transform_with_v_cam(v, *cams)[0]
    return transform_with_v_cam(v, campos, camrot, focal, princpt, K, Rt, distortion_mode, distortion_coeff, fov)[0]
