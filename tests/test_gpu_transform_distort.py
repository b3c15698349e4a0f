"""GPU (-m gpu): the distortion camera models of `transform` -- radial-tangential, fisheye, fisheye62 (+ lookup table),
per-view mode lists -- as ONE fused kernel each way (csrc/transform_distort.hip), against fixtures recorded from the
reference's own `project_points` (tests/gen_golden_transform_distort.py, cases in tests/transform_distort_oracle.py).

Bounds (nothing hand-picked):
  float64   1e-12 * max|ref| for outputs, 10 times that for gradients -- the project's float64 bar for transform;
  float32   assert_within_f64_distance (tests/f64_distance.py) with its defaults: max(1e-5 max|ref64|, 3 |ref32 - ref64|),
            ref32 the reference's own float32 evaluation, read from the fixture;
  the culled set (v_pix.z == -1) equals the fixture's exactly."""
import numpy as np
import pytest
import torch as th

import transform_distort_oracle as O
from f64_distance import assert_within_f64_distance

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [th.float32, th.float64]
IDS = ["f32", "f64"]


def check(got, data, key, dtype, what):
    ref64 = th.from_numpy(data[key + "_f64"])
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    if dtype == th.float64:
        err, scale = float((got - ref64).abs().max()), float(ref64.abs().max())
        bound = (1e-11 if key.startswith("grad") else 1e-12) * scale
        assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    else:
        assert_within_f64_distance(got, th.from_numpy(data[key + "_f32"]), ref64, what)


def cam_tuple(cams):
    return cams["campos"], cams["camrot"], cams["focal"], cams["princpt"]


_FIXTURES = {}


def fixture(name):
    if name not in _FIXTURES:
        _FIXTURES[name] = O.load(name)
    return _FIXTURES[name]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", O.CASE_NAMES)
def test_python_api_matches_the_reference_fixture(name, dtype):
    from drtk_amd.transform import transform, transform_with_v_cam

    data = fixture(name)
    v, cams, kw = O.case_kwargs(name, data, dtype, DEV)
    v.requires_grad_(True)
    v_pix, v_cam = transform_with_v_cam(v, *cam_tuple(cams), **kw)
    g_pix, g_cam = (th.from_numpy(data[k]).to(dtype).to(DEV) for k in ("g_pix", "g_cam"))
    ((v_pix * g_pix).sum() + (v_cam * g_cam).sum()).backward()
    check(v_pix, data, "v_pix", dtype, f"{name} v_pix")
    check(v_cam, data, "v_cam", dtype, f"{name} v_cam")
    check(v.grad, data, "grad_v", dtype, f"{name} grad v")
    assert np.array_equal(v_pix.detach().cpu().numpy()[..., 2] == -1, data["v_pix_f64"][..., 2] == -1), "culled set"
    if "lut_vector_field" not in kw:  # `transform` has no lookup-table arguments (drtk/transform.py:13-24)
        assert th.equal(transform(v.detach(), *cam_tuple(cams), **kw), v_pix.detach())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", O.CASE_NAMES)
def test_c_abi_matches_the_reference_fixture(name, dtype):
    from drtk_amd import capi
    from drtk_amd.transform import _MODE_IDS, _resolve_fov

    data = fixture(name)
    mode, _, fov_given, _ = O.CASES[name]
    v, cams, kw = O.case_kwargs(name, data, dtype, DEV)
    per_view = isinstance(mode, list)
    fov = _resolve_fov(list(mode) if per_view else mode, kw["distortion_coeff"], kw.get("fov"))
    args = dict(coeff=kw["distortion_coeff"], fov=fov, mode=0 if per_view else _MODE_IDS[mode],
                mode_per_view=th.tensor([_MODE_IDS[m] for m in mode], dtype=th.int32, device=DEV) if per_view else None,
                cull_outside_fov=fov_given and not per_view and _MODE_IDS[mode] == 3, lut=kw.get("lut_vector_field"),
                lut_spacing=kw.get("lut_spacing"))
    v_pix, v_cam = capi.transform_distort(v, *cam_tuple(cams), **args)
    g_pix, g_cam = (th.from_numpy(data[k]).to(dtype).to(DEV) for k in ("g_pix", "g_cam"))
    grad_v = capi.transform_distort_backward(g_pix, g_cam, v, *cam_tuple(cams), **args)
    check(v_pix, data, "v_pix", dtype, f"{name} v_pix")
    check(v_cam, data, "v_cam", dtype, f"{name} v_cam")
    check(grad_v, data, "grad_v", dtype, f"{name} grad v")
    assert np.array_equal(v_pix.cpu().numpy()[..., 2] == -1, data["v_pix_f64"][..., 2] == -1), "culled set"
    # either upstream gradient alone: the two add up (to rounding: the sums associate differently)
    only_pix = capi.transform_distort_backward(g_pix, None, v, *cam_tuple(cams), **args)
    only_cam = capi.transform_distort_backward(None, g_cam, v, *cam_tuple(cams), **args)
    scale = float(grad_v.abs().max())
    assert float((only_pix + only_cam - grad_v).abs().max()) <= (1e-5 if dtype == th.float32 else 1e-13) * scale
    assert th.equal(capi.transform_distort(v, *cam_tuple(cams), want_v_cam=False, **args)[0], v_pix)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["rt8_shared", "fisheye62_lut_shared"])
def test_expanded_vertices_take_the_shared_path_bitwise(name, dtype):
    from drtk_amd.transform import transform_with_v_cam

    data = fixture(name)
    v, cams, kw = O.case_kwargs(name, data, dtype, DEV)
    g_pix = th.from_numpy(data["g_pix"]).to(dtype).to(DEV)
    outs = []
    for expand in (False, True):
        leaf = v.clone().requires_grad_(True)
        v_pix, v_cam = transform_with_v_cam(leaf.expand(O.N, -1, -1) if expand else leaf, *cam_tuple(cams), **kw)
        (v_pix * g_pix).sum().backward()
        assert leaf.grad.shape == (1, O.V, 3)
        outs.append((v_pix.detach(), v_cam.detach(), leaf.grad))
    for a, b in zip(*outs):
        assert th.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["rt8", "fisheye", "fisheye62_lut", "mixed", "rt_nofov"])
def test_pytorch_route_on_the_device_serves_camera_and_coefficient_gradients(name, dtype):
    """`camrot.requires_grad_()` sends the call through the PyTorch formulation: its output agrees with the fused route
    within the same bound, its camera and coefficient gradients match the fixture (float32: rtol 1e-4 of the tensor, as
    test_refpy_fixtures.py has it for the pinhole camera)."""
    from drtk_amd.transform import transform_with_v_cam

    data = fixture(name)
    v, cams, kw = O.case_kwargs(name, data, dtype, DEV)
    fused = transform_with_v_cam(v, *cam_tuple(cams), **kw)[0]
    leaves = dict(cams, v=v, D=kw["distortion_coeff"])
    for t in leaves.values():
        t.requires_grad_(True)
    v_pix, v_cam = transform_with_v_cam(v, *cam_tuple(cams), **kw)
    assert v_pix.grad_fn is not None and "TransformDistort" not in type(v_pix.grad_fn).__name__
    check(v_pix, data, "v_pix", dtype, f"{name} v_pix (PyTorch route)")
    check(fused, data, "v_pix", dtype, f"{name} v_pix (fused route)")
    g_pix, g_cam = (th.from_numpy(data[k]).to(dtype).to(DEV) for k in ("g_pix", "g_cam"))
    ((v_pix * g_pix).sum() + (v_cam * g_cam).sum()).backward()
    check(v.grad, data, "grad_v", dtype, f"{name} grad v (PyTorch route)")
    for k in ("campos", "camrot", "focal", "princpt", "D"):
        ref = th.from_numpy(data[f"grad_{k}_f64"])
        err = float((leaves[k].grad.cpu().double() - ref).abs().max())
        rtol = 1e-4 if dtype == th.float32 else 1e-11
        assert err <= rtol * float(ref.abs().max()), f"{name} grad {k}: {err:.3e} > {rtol:g} * {float(ref.abs().max()):.3e}"


def test_graph_capture_with_fov_given_replays_bitwise():
    """fisheye and the mixed list, fov given: after one warm-up call (which builds the cached per-view mode tensor) the
    calls capture into a HIP graph, and the replay -- on new vertices -- equals the eager result bit for bit."""
    import importlib

    from drtk_amd import capi
    T = importlib.import_module("drtk_amd.transform")

    data = fixture("mixed")
    v, cams, kw_mixed = O.case_kwargs("mixed", data, th.float32, DEV)
    _, _, kw_fish = O.case_kwargs("fisheye", fixture("fisheye"), th.float32, DEV)
    g = th.from_numpy(data["g_pix"]).float().to(DEV)
    c = cam_tuple(cams)
    modes = T._mode_tensor(kw_mixed["distortion_mode"], v.device)
    assert T._mode_tensor(list(kw_mixed["distortion_mode"]), v.device) is modes  # cached per (modes, device)

    def step():
        a = T.transform(v, *c, **kw_fish)
        b, b_cam = T.transform_with_v_cam(v, *c, **kw_mixed)
        gb = capi.transform_distort_backward(g, None, v, *c, kw_mixed["distortion_coeff"], kw_mixed["fov"], mode_per_view=modes)
        return a, b, b_cam, gb

    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side), th.no_grad():
        step()
    th.cuda.current_stream().wait_stream(side)
    th.cuda.synchronize()
    graph = th.cuda.CUDAGraph()
    with th.cuda.graph(graph), th.no_grad():
        out = step()
    for shift in (0.0, 0.01):
        v.copy_(th.from_numpy(data["v"]).float().to(DEV) + shift)
        graph.replay()
        th.cuda.synchronize()
        got = [t.clone() for t in out]
        with th.no_grad():
            eager = step()
        for a, b in zip(got, eager):
            assert th.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_more_views_than_one_launch_takes(dtype):
    """N = 65 537 views of V = 2 vertices (the view is blockIdx.y: two slices), fisheye, against the PyTorch route on the device."""
    from drtk_amd.transform import _transform_torch_route, transform_with_v_cam

    N, V = 65537, 2
    rng = np.random.RandomState(7)
    z = rng.uniform(0.5, 2.0, (N, V, 1))
    v64 = th.from_numpy(np.concatenate([0.6 * rng.randn(N, V, 2) * z, z], -1))
    campos = th.from_numpy(0.05 * rng.randn(N, 3))
    camrot = th.eye(3, dtype=th.float64).repeat(N, 1, 1)
    focal = th.tensor([[500.0, 1.5], [0.0, 480.0]], dtype=th.float64).repeat(N, 1, 1) * th.from_numpy(rng.uniform(0.9, 1.1, (N, 1, 1)))
    princpt = th.tensor([320.0, 240.0], dtype=th.float64).repeat(N, 1)
    D = th.tensor(O.FISHEYE, dtype=th.float64).repeat(N, 1) * th.from_numpy(rng.uniform(0.5, 1.5, (N, 1)))
    fov = th.from_numpy(rng.uniform(0.6, 1.4, (N, 1)))
    g = th.from_numpy(rng.uniform(-1, 1, (N, V, 3)))
    # a vertex within 1e-3 of its fov would let float32 clamp where float64 does not: move those inside
    p = v64[..., :2] / v64[..., 2:]
    near = ((p.norm(dim=-1) / fov - 1).abs() < 1e-3)
    v64[..., :2] = th.where(near[..., None], 0.5 * v64[..., :2], v64[..., :2])

    def run(fn, dt, grad_cam):
        t = [x.to(dt).to(DEV) for x in (v64, campos, camrot, focal, princpt, D, fov, g)]
        t[0].requires_grad_(True)
        t[2].requires_grad_(grad_cam)
        out = fn(t[0], *t[1:5], distortion_mode="fisheye", distortion_coeff=t[5], fov=t[6])[0]
        (out * t[7]).sum().backward()
        return out.detach().cpu(), t[0].grad.cpu()

    got = run(transform_with_v_cam, dtype, False)
    ref64 = run(_transform_torch_route, th.float64, True)
    if dtype == th.float64:
        for a, b, tol, what in zip(got, ref64, (1e-12, 1e-11), ("v_pix", "grad v")):
            assert float((a - b).abs().max()) <= tol * float(b.abs().max()), what
    else:
        ref32 = run(_transform_torch_route, th.float32, True)
        for a, b32, b64, what in zip(got, ref32, ref64, ("v_pix", "grad v")):
            assert_within_f64_distance(a, b32, b64, what)
    # the last view lies in the second slice: it is the same as that view alone
    t = [x[-1:].to(dtype).to(DEV) for x in (v64, campos, camrot, focal, princpt, D, fov)]
    alone = transform_with_v_cam(t[0], *t[1:5], distortion_mode="fisheye", distortion_coeff=t[5], fov=t[6])[0]
    assert th.equal(alone.cpu(), got[0][-1:])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", ["radial-tangential", "fisheye", "fisheye62"])
def test_degenerate_vertices_stay_finite(mode, dtype):
    """A vertex with z = 0 exactly (camera plane), one on the optical axis (where the reference's sqrt has a NaN gradient:
    the documented deviation) and an ordinary one; radial-tangential with fov = inf and 4 coefficients, where r2^3
    overflows in float32 on the camera plane and must not be formed.  Outputs and gradients are finite."""
    from drtk_amd.transform import transform_with_v_cam

    v = th.tensor([[[0.05, 0.02, 0.0], [0.0, 0.0, 1.5], [0.3, -0.2, 1.0], [0.0, 0.0, 0.0]]], dtype=dtype, device=DEV).requires_grad_(True)
    cams = (th.zeros(1, 3), th.eye(3)[None], th.tensor([[[500.0, 1.5], [0.0, 480.0]]]), th.tensor([[320.0, 240.0]]))
    cams = tuple(c.to(dtype).to(DEV) for c in cams)
    kw = {"radial-tangential": dict(distortion_coeff=th.tensor([O.RT[:4]]), fov=th.tensor([[float("inf")]])),
          "fisheye": dict(distortion_coeff=th.tensor([O.FISHEYE]), fov=th.tensor([[0.9]])),
          "fisheye62": dict(distortion_coeff=th.tensor([O.FISHEYE62]), fov=th.tensor([[0.9]]), lut_vector_field=th.ones(1, 2, 9, 13),
                            lut_spacing=th.tensor([O.LUT_SPACING]))}[mode]
    kw = {k: t.to(dtype).to(DEV) for k, t in kw.items()}
    v_pix, v_cam = transform_with_v_cam(v, *cams, distortion_mode=mode, **kw)
    (v_pix.sum() + v_cam.sum()).backward()
    assert bool(th.isfinite(v_pix).all()) and bool(th.isfinite(v_cam).all()), v_pix
    assert bool(th.isfinite(v.grad).all()), v.grad
    # on the axis the projection is the principal point, and its gradient that of the pinhole camera (scale 1)
    assert th.allclose(v_pix[0, 1, :2].cpu().double(), th.tensor([320.0, 240.0], dtype=th.float64) + (1.0 if mode == "fisheye62" else 0.0), atol=1e-4, rtol=0)
    if mode != "fisheye62":
        expect = th.tensor([500.0 / 1.5 + 1.0, (1.5 + 480.0) / 1.5 + 1.0, 2.0], dtype=th.float64)
        assert th.allclose(v.grad[0, 1].cpu().double(), expect, rtol=1e-5 if dtype == th.float32 else 1e-12, atol=0)


def test_end_to_end_fisheye_step_at_48x64():
    """transform -> rasterize -> render -> interpolate -> loss.backward() with one fisheye view: the gradient that reaches
    the world-space vertices through the fused kernel against the PyTorch route, within the float32 rule (oracle_f64: the
    PyTorch route in float64; rasterize runs once, on the fused v_pix, and all three share its index image)."""
    import drtk_amd
    from drtk_amd import synthetic as S
    from drtk_amd.transform import _transform_torch_route, transform

    H, W = 48, 64
    v0, vi = S.uv_sphere(10, 12, dtype=th.float64)
    cams64 = S.ring_cameras(1, W, H, dtype=th.float64)
    D64, fov64 = th.tensor([O.FISHEYE], dtype=th.float64), th.tensor([[0.9]], dtype=th.float64)
    gen = th.Generator().manual_seed(3)
    attr64 = th.rand(1, v0.shape[0], 4, generator=gen, dtype=th.float64)
    w64 = th.rand(1, 4, H, W, generator=gen, dtype=th.float64) * 2 - 1
    vi = vi.to(DEV)
    index_img = None

    def run(route, dt):
        nonlocal index_img
        v = v0[None].to(dt).to(DEV).requires_grad_(True)
        cams = tuple(c.to(dt).to(DEV) for c in cams64)
        kw = dict(distortion_mode="fisheye", distortion_coeff=D64.to(dt).to(DEV), fov=fov64.to(dt).to(DEV))
        v_pix = transform(v, *cams, **kw) if route == "fused" else _transform_torch_route(v, *cams, **kw)[0]
        if index_img is None:
            index_img = drtk_amd.rasterize(v_pix.detach(), vi, H, W)
            assert int((index_img >= 0).sum()) > H * W // 20
        depth_img, bary_img = drtk_amd.render(v_pix, vi, index_img)
        img = drtk_amd.interpolate(attr64.to(dt).to(DEV), vi, index_img, bary_img)
        ((img * w64.to(dt).to(DEV)).sum() + depth_img.sum()).backward()
        return v.grad.cpu()

    got = run("fused", th.float32)
    assert_within_f64_distance(got, run("torch", th.float32), run("torch", th.float64), "grad v through the step")
