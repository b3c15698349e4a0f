"""The distortion camera models of `transform` without a GPU: the package's PyTorch formulation on the CPU against the
reference's fixtures (tests/golden/transform_distort_*.npz), the field-of-view estimators, the reference's validation,
and the argument checks of the C ABI (decided on the host, before any launch)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transform_distort_oracle as O  # noqa: E402

# the project's float64 bar for transform (test_gpu_parity.py: test_transform_pinhole_matches_pytorch_formulation)
RTOL64 = 1e-12


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= rtol * scale, f"{what}: {err:.3e} > {rtol:g} * {scale:.3e}"


@pytest.mark.parametrize("name", O.CASE_NAMES)
def test_pytorch_formulation_matches_the_reference_fixture(name):
    """float64 on the CPU: v_pix, v_cam within 1e-12 max|ref|, every VJP (v, cameras, coefficients) within 10 times that."""
    from drtk_amd.transform import _transform_torch_route

    data = O.load(name)
    v, cams, kw = O.case_kwargs(name, data, th.float64)
    leaves = dict(cams, v=v, D=kw["distortion_coeff"])
    for t in leaves.values():
        t.requires_grad_(True)
    v_pix, v_cam = _transform_torch_route(v, cams["campos"], cams["camrot"], cams["focal"], cams["princpt"], **kw)
    assert v_pix.shape == v_cam.shape == (O.N, O.V, 3)
    _close(v_pix.detach(), data["v_pix_f64"], RTOL64, "v_pix")
    _close(v_cam.detach(), data["v_cam_f64"], RTOL64, "v_cam")
    assert np.array_equal(v_pix.detach().numpy()[..., 2] == -1, data["v_pix_f64"][..., 2] == -1), "culled set"
    ((v_pix * th.from_numpy(data["g_pix"])).sum() + (v_cam * th.from_numpy(data["g_cam"])).sum()).backward()
    for k, t in leaves.items():
        _close(t.grad, data[f"grad_{k}_f64"], 10 * RTOL64, f"grad {k}")


def test_fixtures_hold_the_inputs_the_oracle_module_makes_and_what_it_promises():
    """The committed inputs are make_inputs() (so the generator can be rerun), both sides of every fov are populated, the
    lookup table moves most vertices, and the cull is exercised."""
    made, stored = O.make_inputs(), O._npz("inputs")
    for k, a in made.items():
        assert np.array_equal(a, stored[k]), k
    d = O.load("fisheye62_lut")
    p = d["v_cam_f64"][..., :2] / np.where(np.abs(d["v_cam_f64"][..., 2:]) < 1e-8, 1e-8, d["v_cam_f64"][..., 2:])
    beyond = (np.sqrt((p * p).sum(-1)) > d["fov"]).mean(1)
    assert (beyond > 0.05).all() and (beyond < 0.7).all(), beyond
    assert np.array_equal(d["v_pix_f64"][..., 2] == -1, np.sqrt((p * p).sum(-1)) > d["fov"])
    moved = np.abs(d["v_pix_f64"] - O.load("fisheye62")["v_pix_f64"]).max(-1) > 0
    assert moved.sum() > O.N * O.V // 2 and (~moved).sum() > 20, moved.sum()
    assert not (O.load("fisheye62_nofov")["v_pix_f64"][..., 2] == -1).any()  # an estimated fov does not cull
    assert abs(float(O.load("rt_nofov")["fov_estimated"][0, 0]) - 1.14) < 0.01
    assert abs(float(O.load("fisheye_nofov")["fov_estimated"][0, 0]) - 1.205) < 0.01


@pytest.mark.parametrize("tag,dtype", [("f64", np.float64), ("f32", np.float32)])
def test_fov_estimators_equal_the_reference_exactly(tag, dtype):
    """Same derivative polynomials, numpy.roots in the coefficients' dtype, smallest positive real root, float32."""
    import drtk.utils
    import drtk.utils.projection as P
    import importlib

    T = importlib.import_module("drtk_amd.transform")  # (the package attribute of that name is the function)
    rec = O._npz("estimators")
    rows = rec["rows"].astype(dtype)
    for fn in ("estimate_rt_fov", "estimate_fisheye_fov", "estimate_fisheye62_fov"):
        assert getattr(P, fn) is getattr(T, fn) and getattr(drtk.utils, fn) is getattr(T, fn)
        got = getattr(T, fn)(th.from_numpy(rows))
        assert got.dtype == th.from_numpy(rows).dtype and got.shape == (len(rows), 1)
        assert np.array_equal(got.numpy(), rec[f"{fn}_{tag}"]), (fn, got.ravel(), rec[f"{fn}_{tag}"].ravel())
        assert np.array_equal(getattr(T, fn)(rows), rec[f"{fn}_{tag}"].astype(np.float32))  # numpy in: float32 numpy out
    assert np.isinf(rec["estimate_rt_fov_f64"]).any() and np.isfinite(rec["estimate_rt_fov_f64"]).any()


def test_validation_mirrors_the_reference():
    import drtk.utils.projection as P
    from drtk_amd.transform import _transform_torch_route, transform, transform_with_v_cam

    assert P.DISTORTION_MODES == {None, "pinhole", "radial-tangential", "fisheye"}
    d = O.load("fisheye")
    v, cams, _ = O.case_kwargs("fisheye", d, th.float64)
    c = (cams["campos"], cams["camrot"], cams["focal"], cams["princpt"])
    D8 = th.zeros(3, 8, dtype=th.float64)
    for fn in (transform, transform_with_v_cam, _transform_torch_route, P.project_points):
        with pytest.raises(AssertionError, match="Missing distortion coefficients"):
            fn(v, *c, distortion_mode="fisheye")
        for bad in ("fish-eye", ["pinhole", "fisheye62", "fisheye"], ["fisheye62_lut", "pinhole", "pinhole"], 7):
            with pytest.raises(ValueError, match=re.escape(f"Invalid distortion mode: {bad}. Valid options:")):
                fn(v, *c, distortion_mode=bad, distortion_coeff=D8)
    # the checks of the coefficient table
    with pytest.raises(AssertionError):
        _transform_torch_route(v, *c, distortion_mode="radial-tangential", distortion_coeff=th.zeros(3, 6, dtype=th.float64))
    with pytest.raises(AssertionError, match="Fisheye62 model requires 8 distortion parameters"):
        _transform_torch_route(v, *c, distortion_mode="fisheye62", distortion_coeff=th.zeros(3, 4, dtype=th.float64))
    with pytest.raises(AssertionError, match="spacing must be provided"):
        _transform_torch_route(v, *c, distortion_mode="fisheye62", distortion_coeff=D8, lut_vector_field=th.zeros(3, 2, 4, 4, dtype=th.float64))
    # a list of one distinct mode is that mode (fisheye62 included); a list of pinhole spellings is the pinhole camera
    D = th.from_numpy(O.load("fisheye62")["D"])
    one = _transform_torch_route(v, *c, distortion_mode="fisheye62", distortion_coeff=D)[0]
    assert th.equal(_transform_torch_route(v, *c, distortion_mode=["fisheye62"] * 3, distortion_coeff=D)[0], one)
    assert th.equal(_transform_torch_route(v, *c, distortion_mode=["pinhole", None, "pinhole"], distortion_coeff=D)[0], transform(v, *c))
    assert th.equal(_transform_torch_route(v, *c, distortion_mode=[], distortion_coeff=D)[0], transform(v, *c))


def test_cpu_tensors_still_get_the_pinhole_camera_only():
    """No computing CPU path: the public functions raise on CPU tensors and say where the models run."""
    import drtk.utils.projection as P
    from drtk_amd.transform import transform, transform_with_v_cam

    d = O.load("mixed")
    for name in ("rt8", "fisheye", "fisheye62_lut", "mixed"):
        v, cams, kw = O.case_kwargs(name, dict(d, D=O.load(name)["D"]), th.float32)
        c = (cams["campos"], cams["camrot"], cams["focal"], cams["princpt"])
        calls = [lambda: transform_with_v_cam(v, *c, **kw), lambda: P.project_points(v, *c, **kw),
                 lambda: transform(v, *c, **{k: a for k, a in kw.items() if not k.startswith("lut")})]
        for call in calls:
            with pytest.raises(NotImplementedError, match="pinhole camera only") as e:
                call()
            assert "HIP device" in str(e.value)


def test_new_entry_points_are_declared_exported_and_bound():
    from drtk_amd import capi

    with open(os.path.join(ROOT, "include", "drtk_amd.h")) as f:
        header = f.read()
    for sym in ("drtk_amd_transform_distort", "drtk_amd_transform_distort_backward"):
        assert re.search(rf"\bint {sym}\(", header), sym
        assert sym in capi.EXPORTS
        assert getattr(capi.lib(), sym).restype is ctypes.c_int


def _call_c_abi(backward=False, **over):
    """One call of the C ABI with made-up non-null pointers: every case below is rejected before anything is read."""
    from drtk_amd import capi

    N, V = 2, 5
    a = dict(dtype=capi.DRTK_F32, v=0x1000, v_sN=3 * V, campos=0x1000, camrot=0x1000, focal=0x1000, princpt=0x1000, mode_all=2,
             mode_per_view=0, coeff=0x1000, ncoef=4, fov=0x1000, cull=0, lut=0, lut_spacing=0, Hl=0, Wl=0, N=N, V=V,
             out=0x1000, out2=0, g_pix=0x1000, g_cam=0)
    a.update(over)
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    head = [i(a["dtype"]), p(a["v"]), i64(a["v_sN"]), p(a["campos"]), p(a["camrot"]), p(a["focal"]), p(a["princpt"]),
            i(a["mode_all"]), p(a["mode_per_view"]), p(a["coeff"]), i(a["ncoef"]), p(a["fov"]), i(a["cull"]), p(a["lut"]),
            p(a["lut_spacing"]), i64(a["Hl"]), i64(a["Wl"])]
    if backward:
        return capi.lib().drtk_amd_transform_distort_backward(*head, p(a["g_pix"]), p(a["g_cam"]), i64(a["N"]), i64(a["V"]), p(a["out"]), p(0))
    return capi.lib().drtk_amd_transform_distort(*head, i64(a["N"]), i64(a["V"]), p(a["out"]), p(a["out2"]), p(0))


@pytest.mark.parametrize("backward", [False, True])
def test_c_abi_rejects_bad_arguments_without_a_gpu(backward):
    INVALID = -1  # DRTK_ERR_INVALID_ARGUMENT
    from drtk_amd import capi

    assert b"invalid" in capi.lib().drtk_amd_status_string(INVALID).lower()
    bad = [dict(mode_all=4), dict(mode_all=-1), dict(ncoef=3), dict(ncoef=6), dict(ncoef=0), dict(v_sN=1), dict(v_sN=14),
           dict(dtype=2), dict(N=-1), dict(V=-1), dict(mode_all=3, ncoef=4), dict(lut=0x1000, Hl=3, Wl=3), dict(lut=0x1000, lut_spacing=0x1000, Hl=0, Wl=3),
           dict(out=0)]
    bad += [{k: 0} for k in ("v", "campos", "camrot", "focal", "princpt", "coeff", "fov")]
    if backward:
        bad.append(dict(g_pix=0, g_cam=0))
    for over in bad:
        assert _call_c_abi(backward, **over) == INVALID, over
    # nothing to do is not an error, whatever the pointers
    assert _call_c_abi(backward, N=0, v=0, out=0, g_pix=0) == 0
    assert _call_c_abi(backward, V=0, v_sN=0, v=0, out=0, g_pix=0) == 0
