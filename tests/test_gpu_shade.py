"""GPU: drtk_amd.shade on the HIP route (csrc/shade.hip through the drtk_amd_ext operator and through the C ABI) -- the output
and every gradient against the independent oracle (tests/shade_oracle.py, evaluated on the device) on its structural
cases, input layouts read in place, NaN where nothing may be read, the conventions at the non-smooth points, which
gradients and kernels a backward produces, bitwise reproducibility, graph capture, autocast, more views than one launch
takes, the tutorial's step end to end, and the C ABI between sentinel elements (tests/guarded_shade.py in a child process).

float64 is held to 1e-12 * max(1, max|oracle|); float32 to tests/f64_distance.py's bound with its defaults (k = 3,
rel = 1e-5), the oracle in float32 and float64 on the same float32 inputs, and for the parameter gradients the magnitude that
was accumulated into them."""
import functools
import os
import subprocess
import sys

import pytest
import torch as th
from conftest import ROOT

import shade_oracle as O
from f64_distance import assert_within_f64_distance

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOATS = ("normal_img", "pos_img", "albedo", "background", "light_dir", "ambient", "specular", "shininess")


@functools.lru_cache(maxsize=None)
def inputs(name):
    return O.case(name)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype):
    """The oracle on the device, once per case and precision, shared by every test (and never modified)."""
    inp, grad_out = inputs(name)
    return {k: v.detach().cpu() for k, v in O.reference(inp, grad_out, dtype, DEV).items()}


def to_device(inp, dtype):
    return {k: (v.to(DEV, dtype) if v.is_floating_point() else v.to(DEV)) if th.is_tensor(v) else v for k, v in inp.items()}


def run_hip(inp, grad_out, dtype, api="ops", need=FLOATS):
    """{"out", "grad_<name>"} of the package (`ops`: drtk_amd.shade and autograd) or of the ctypes binding (`capi`), on the CPU."""
    import drtk_amd
    from drtk_amd import capi

    a = to_device(inp, dtype)
    g = grad_out.to(DEV, dtype)
    res = {}
    if api == "ops":
        for k in need:
            if a[k] is not None:
                a[k].requires_grad_(True)
        out = drtk_amd.shade(**a)
        out.backward(g)
        res = {"grad_" + k: a[k].grad for k in need if a[k] is not None}
        res["out"] = out.detach()
    else:
        res = {"grad_" + k: v for k, v in capi.shade_backward(g, **a, want=need).items()}
        res["out"] = capi.shade_forward(**a)
    return {k: v.cpu() for k, v in res.items()}


def check(got, r64, r32, dtype, what):
    """Every output and gradient the oracle has: float64 to 1e-12, float32 within the float64-distance bound."""
    for k, want in r64.items():
        if k.startswith("mag_"):
            continue
        name = k[5:] if k.startswith("grad_") else k
        if k.startswith("grad_") and name in ("pos_img", "shininess") and "grad_specular" not in r64:
            continue
        assert k in got, (what, k)
        a = got[k]
        assert a.dtype == dtype and a.shape == want.shape, (what, k, a.shape, want.shape)
        err = float((a.double() - want).abs().max())
        print(f"{what} {k} {dtype}: |hip - f64| = {err:.3e}, max|f64| = {float(want.abs().max()):.3e}")
        if dtype == th.float64:
            assert err <= 1e-12 * max(1.0, float(want.abs().max())), (what, k, err)
        else:
            assert_within_f64_distance(a, r32[k], want, f"{what} {k}", acc_magnitude=r64.get("mag_" + name))


def check_case(name, dtype, api):
    inp, grad_out = inputs(name)
    got = run_hip(inp, grad_out, dtype, api)
    check(got, oracle(name, th.float64), oracle(name, th.float32) if dtype == th.float32 else None, dtype, f"{name} {api}")
    return got


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("name", list(O.CASES))
def test_output_and_every_gradient_match_the_oracle(name, dtype):
    check_case(name, dtype, "ops")


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("name", list(O.CASES))
def test_c_abi_matches_the_oracle_and_the_operator_bit_for_bit(name, dtype):
    a, b = check_case(name, dtype, "capi"), run_hip(*inputs(name), dtype, "ops")
    assert set(a) == set(b)
    for k in a:
        assert th.equal(a[k], b[k]), (name, k)


# ---- layouts -----------------------------------------------------------------------------------------------------------------

def _layout_base(dtype):
    inp, grad_out = inputs("n2_c3")  # 41 x 25, two views
    return to_device(inp, dtype), grad_out.to(DEV, dtype)


def _with_grads(a, names):
    out = dict(a)
    for k in names:
        out[k] = a[k].detach().clone().requires_grad_(True)
    return out


LAYOUTS = ["channel_slices", "view_slice", "expanded_background", "w_strided", "offset_one_element", "cropped_columns"]


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_are_read_in_place_and_give_the_contiguous_result(layout, dtype):
    """Each layout against the same values in contiguous tensors: bitwise equal (the kernel does the same arithmetic on the
    same numbers), the gradient arriving in the base tensor; and the contiguous result against the oracle."""
    import drtk_amd

    a, g = _layout_base(dtype)
    N, _, H, W = a["normal_img"].shape
    a["albedo"] = (th.rand(N, 3, H, W, dtype=th.float64, generator=th.Generator().manual_seed(3)) + 0.05).float().to(DEV, dtype)
    names = ("normal_img", "pos_img", "albedo", "background")
    ref = _with_grads(a, names)
    alt = dict(a)
    bases = {}

    if layout == "channel_slices":  # one [N, 9, H, W] tensor, as interpolate returns it
        attr = th.cat([a["normal_img"], a["pos_img"], a["albedo"]], 1).requires_grad_(True)
        alt.update(normal_img=attr[:, 0:3], pos_img=attr[:, 3:6], albedo=attr[:, 6:9])
        alt["background"] = a["background"].clone().requires_grad_(True)
    elif layout == "view_slice":
        for k in names:
            big = th.full((N + 2, *a[k].shape[1:]), float("nan"), dtype=dtype, device=DEV)
            big[1:N + 1] = a[k]
            big.requires_grad_(True)
            bases[k], alt[k] = big, big[1:N + 1]
        idx = th.full((N + 2, H, W), 7, dtype=th.int32, device=DEV)
        idx[1:N + 1] = a["index_img"]
        alt["index_img"] = idx[1:N + 1]
    elif layout == "expanded_background":
        one = a["background"][:1].clone().requires_grad_(True)
        bases["background"], alt["background"] = one, one.expand(N, -1, -1, -1)
        ref["background"] = one.detach().expand(N, -1, -1, -1).contiguous().requires_grad_(True)
        for k in names[:3]:
            alt[k] = a[k].clone().requires_grad_(True)
    elif layout == "w_strided":  # copied once
        for k in names:
            big = th.full((*a[k].shape[:3], 2 * W), float("nan"), dtype=dtype, device=DEV)
            big[..., ::2] = a[k]
            big.requires_grad_(True)
            bases[k], alt[k] = big, big[..., ::2]
    elif layout == "offset_one_element":  # element alignment only
        for k in names:
            flat = th.zeros(a[k].numel() + 1, dtype=dtype, device=DEV)
            flat[1:] = a[k].flatten()
            flat.requires_grad_(True)
            bases[k], alt[k] = flat, flat[1:].view(a[k].shape)
        idx = th.zeros(N * H * W + 1, dtype=th.int32, device=DEV)
        idx[1:] = a["index_img"].flatten()
        alt["index_img"] = idx[1:].view(N, H, W)
    else:  # rows W + 3 apart: a lane's pixels may span two rows
        for k in names:
            big = th.full((*a[k].shape[:3], W + 3), float("nan"), dtype=dtype, device=DEV)
            big[..., 2:W + 2] = a[k]
            big.requires_grad_(True)
            bases[k], alt[k] = big, big[..., 2:W + 2]
        idx = th.full((N, H, W + 3), -1, dtype=th.int32, device=DEV)
        idx[..., 1:W + 1] = a["index_img"]
        alt["index_img"] = idx[..., 1:W + 1]
    for k in names:
        assert layout not in ("w_strided", "cropped_columns") or not alt[k].is_contiguous(), k
    want = drtk_amd.shade(**ref)
    want.backward(g)
    got = drtk_amd.shade(**alt)
    got.backward(g)
    assert th.equal(got, want)
    for k in names:
        if layout == "channel_slices" and k != "background":
            lo = {"normal_img": 0, "pos_img": 3, "albedo": 6}[k]
            mine = attr.grad[:, lo:lo + 3]
        elif k in bases:
            base_grad = bases[k].grad
            if layout == "view_slice":
                mine = base_grad[1:N + 1]
                assert th.equal(base_grad[0], th.zeros_like(base_grad[0]))
            elif layout == "w_strided":
                mine = base_grad[..., ::2]
            elif layout == "offset_one_element":
                mine = base_grad[1:].view(a[k].shape)
            elif layout == "cropped_columns":
                mine = base_grad[..., 2:W + 2]
            else:  # the one shared background: the sum over the views
                assert th.allclose(base_grad[0], ref[k].grad.sum(0), rtol=1e-6 if dtype == th.float32 else 1e-14, atol=1e-7 if dtype == th.float32 else 1e-15)
                continue
        else:
            mine = alt[k].grad
        assert th.equal(mine, ref[k].grad), (layout, k)
    inp = {k: (v.detach().cpu().double() if th.is_tensor(v) and v.is_floating_point() else v.cpu() if th.is_tensor(v) else v)
           for k, v in ref.items()}
    r64 = O.reference(inp, g.cpu().double(), th.float64, DEV)
    r32 = O.reference(inp, g.cpu().double(), th.float32, DEV) if dtype == th.float32 else None
    res = {"out": want.detach().cpu(), **{"grad_" + k: ref[k].grad.cpu() for k in names}}
    cpu = lambda r: None if r is None else {k: v.cpu() for k, v in r.items() if k == "out" or k[5:] in names}  # noqa: E731
    check(res, cpu(r64), cpu(r32), dtype, layout)


# ---- what must not be read, and the non-smooth points ------------------------------------------------------------------------

@pytest.mark.parametrize("api", ["ops", "capi"])
@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_nan_where_nothing_may_be_read_changes_no_bit(dtype, api):
    inp, grad_out = inputs("n1_c1")  # an albedo image, index, specular, background, gamma
    assert inp["albedo"].ndim == 4
    clean = run_hip(inp, grad_out, dtype, api)
    fg = (inp["index_img"] != -1)[:, None]
    bad = dict(inp)
    for k in ("normal_img", "pos_img", "albedo"):
        bad[k] = th.where(fg, inp[k], th.full_like(inp[k], float("nan")))
    bad["background"] = th.where(fg, th.full_like(inp["background"], float("nan")), inp["background"])
    poisoned = run_hip(bad, grad_out, dtype, api)
    assert set(clean) == set(poisoned) and len(clean) == 9
    for k in clean:
        assert bool(th.isfinite(poisoned[k]).all()), k
        assert th.equal(clean[k], poisoned[k]), k


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_conventions_negative_value_under_gamma_and_a_zero_normal(dtype):
    import drtk_amd

    inp, grad_out = inputs("opt_i1s1b1g1")
    a = to_device(inp, dtype)
    g = grad_out.to(DEV, dtype)
    # a negative albedo shades to a negative value: the gamma step gives 0 and passes exactly 0 (PyTorch's pow(clamp) gives NaN)
    neg = dict(a, specular=None, pos_img=None, shininess=None, albedo=-a["albedo"].abs())
    leaves = _with_grads(neg, ("normal_img", "albedo", "background", "light_dir", "ambient"))
    out = drtk_amd.shade(**leaves)
    out.backward(g)
    fg = (a["index_img"] != -1)[:, None].expand_as(out)
    assert th.equal(out[fg], th.zeros_like(out[fg])) and bool((out[~fg] > 0).all())
    for k in ("normal_img", "albedo", "light_dir", "ambient"):
        assert th.equal(leaves[k].grad, th.zeros_like(leaves[k].grad)), k
    gb = leaves["background"].grad
    assert bool(th.isfinite(gb).all()) and th.equal(gb[fg], th.zeros_like(gb[fg])) and float(gb[~fg].abs().min()) > 0
    # a zero normal: unit(0) = 0, so the pixel is albedo * ambient, and the normal gets no gradient
    zero = dict(a, gamma=None)
    zero["normal_img"] = a["normal_img"].clone()
    zero["normal_img"][:, :, ::2, ::3] = 0
    zero["specular"] = th.zeros_like(a["specular"])
    leaves = _with_grads(zero, ("normal_img", "pos_img", "albedo", "ambient", "light_dir"))
    out = drtk_amd.shade(**leaves)
    out.backward(g)
    assert bool(th.isfinite(out).all())
    flat = leaves["albedo"].detach() * leaves["ambient"].detach()[:, :, None, None]
    at = th.zeros(out.shape, dtype=th.bool, device=DEV)
    at[:, :, ::2, ::3] = True
    at &= fg
    assert bool(at.any()) and th.equal(out[at], flat[at])
    gn = leaves["normal_img"].grad
    at3 = at[:, :1].expand_as(gn)
    assert th.equal(gn[at3], th.zeros_like(gn[at3]))
    for k in ("normal_img", "pos_img", "albedo", "ambient", "light_dir"):
        assert bool(th.isfinite(leaves[k].grad).all()), k


# ---- which gradients, which kernels --------------------------------------------------------------------------------------------

def _launches(a, g, need):
    import drtk_amd
    from drtk_amd import capi

    leaves = _with_grads(a, need)
    th.cuda.synchronize()
    capi.kernel_timing_begin()
    out = drtk_amd.shade(**leaves)
    if out.requires_grad:
        out.backward(g)
    th.cuda.synchronize()
    rep = capi.kernel_timing_report()
    count = lambda name: sum(n for k, (n, _) in rep.items() if k.strip("()").split("<")[0] == name)  # noqa: E731
    return leaves, tuple(count(k) for k in ("shade_forward_kernel", "shade_backward_kernel", "shade_finalize_kernel"))


def test_only_requested_gradients_and_no_finalize_without_a_parameter_gradient():
    inp, grad_out = inputs("n3_c3")  # light and ambient per view, albedo, specular and shininess shared
    a, g = to_device(inp, th.float32), grad_out.to(DEV)
    every = tuple(k for k in FLOATS if a[k] is not None)
    full, n = _launches(a, g, every)
    assert n == (1, 1, 2)  # the views' rows, then the views' sums for the shared parameters
    for need, want in (((), (1, 0, 0)), (("normal_img",), (1, 1, 0)), (("pos_img", "background"), (1, 1, 0)),
                       (("light_dir", "ambient"), (1, 1, 1)), (("shininess",), (1, 1, 2)), (("normal_img", "albedo"), (1, 1, 2))):
        leaves, n = _launches(a, g, need)
        assert n == want, (need, n)
        for k in every:
            if k in need:  # the same bits, whatever else was asked for
                assert th.equal(leaves[k].grad, full[k].grad), (need, k)
            else:
                assert leaves[k].grad is None, (need, k)
    one = {k: (v[:1] if th.is_tensor(v) and (v.ndim >= 3 or (v.ndim == 2 and v.shape[0] == 3)) else v) for k, v in a.items()}
    assert _launches(one, g[:1], every)[1] == (1, 1, 1)  # one view: its sums are the shared parameters' gradients


def test_errors_on_the_device_and_double_backward():
    import drtk_amd

    inp, grad_out = inputs("n2_c3")
    a = to_device(inp, th.float32)
    with pytest.raises(ValueError, match="specular needs"):
        drtk_amd.shade(**dict(a, pos_img=None))
    with pytest.raises(ValueError, match="int32"):
        drtk_amd.shade(**dict(a, index_img=a["index_img"].long()))
    with pytest.raises(RuntimeError, match="type of normal_img"):
        drtk_amd.shade(**dict(a, background=a["background"].double()))
    with pytest.raises(RuntimeError, match="same device"):
        drtk_amd.shade(**dict(a, ambient=a["ambient"].cpu()))
    leaves = _with_grads(a, ("normal_img",))
    out = drtk_amd.shade(**leaves)
    with pytest.raises(RuntimeError, match="double backward"):
        th.autograd.grad(out.sum(), leaves["normal_img"], create_graph=True)
    (gn,) = th.autograd.grad(drtk_amd.shade(**leaves).sum(), leaves["normal_img"])  # a plain backward still works
    assert bool(th.isfinite(gn).all())


def test_no_views_and_no_pixels():
    import drtk_amd

    for N, H, W in ((0, 4, 5), (2, 0, 5)):
        n = th.zeros(N, 3, H, W, device=DEV, requires_grad=True)
        amb = th.rand(3, device=DEV, requires_grad=True)
        out = drtk_amd.shade(n, th.ones(3, device=DEV), th.rand(3, device=DEV), amb)
        assert out.shape == (N, 3, H, W)
        out.sum().backward()
        assert n.grad.shape == n.shape and th.equal(amb.grad, th.zeros(3, device=DEV))


# ---- reproducibility, capture, autocast, many views ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rows_2S+1_f32", "per_view_all", "n3_c4"])
def test_two_runs_are_bitwise_equal(name):
    a = run_hip(*inputs(name), th.float32)
    b = run_hip(*inputs(name), th.float32)
    assert set(a) == set(b)
    for k in a:
        assert th.equal(a[k], b[k]), (name, k)


def test_graph_capture_replays_to_the_same_bits():
    import drtk_amd

    inp, grad_out = inputs("n3_c3")
    a, g = to_device(inp, th.float32), grad_out.to(DEV)
    names = tuple(k for k in FLOATS if a[k] is not None)
    leaves = _with_grads(a, names)

    def step():
        out = drtk_amd.shade(**leaves)
        loss = (out * g).sum()
        loss.backward()
        return out

    want = step().detach().clone()
    want_grads = {k: leaves[k].grad.clone() for k in names}
    cap = drtk_amd.capture_step(step, [leaves[k] for k in names])
    for _ in range(2):
        for k in names:
            leaves[k].grad = None
        cap()
        th.cuda.synchronize()
        assert th.equal(cap.outputs, want)
        for k in names:
            assert th.equal(leaves[k].grad, want_grads[k]), k


def test_autocast_half_inputs_give_a_float32_result():
    import drtk_amd

    inp, _ = inputs("n2_c3")
    a = to_device(inp, th.float32)
    half = {k: (v.half() if th.is_tensor(v) and v.is_floating_point() else v) for k, v in a.items()}
    with th.autocast("cuda", dtype=th.float16):
        out = drtk_amd.shade(**half)
    assert out.dtype == th.float32
    want = drtk_amd.shade(**{k: (v.float() if th.is_tensor(v) and v.is_floating_point() else v) for k, v in half.items()})
    assert th.equal(out, want)


def test_more_views_than_one_launch_takes():
    """N = 65 537 views of 1 x 2 pixels: two launches of the streaming kernels, and 65 537 rows of view sums for the shared
    parameters.  Against the oracle under the same bounds."""
    N = 65537
    g = th.Generator().manual_seed(11)
    f32 = lambda t: t.float().double()  # noqa: E731
    d = th.randn(N, 3, 1, 2, generator=g, dtype=th.float64)
    inp = dict(normal_img=f32(d / d.norm(dim=1, keepdim=True) * 0.7), light_dir=f32(th.tensor([0.2, -0.4, 0.9], dtype=th.float64)),
               albedo=f32(0.05 + th.rand(3, generator=g, dtype=th.float64)), ambient=f32(0.05 + th.rand(N, 3, generator=g, dtype=th.float64)),
               index_img=th.where(th.rand(N, 1, 2, generator=g) < 0.3, -1, 5).int(), pos_img=None, specular=None, shininess=None,
               background=f32(0.05 + th.rand(N, 3, 1, 2, generator=g, dtype=th.float64)), gamma=2.2)
    grad_out = f32(th.randn(N, 3, 1, 2, generator=g, dtype=th.float64))
    cat = O.categories(inp)
    keep = cat["ndl"].abs() >= O.MARGIN  # pixels nearer the kink become background
    inp["index_img"] = th.where(keep, inp["index_img"], th.full_like(inp["index_img"], -1))
    for dtype in (th.float32, th.float64):
        got = run_hip(inp, grad_out, dtype)
        r64 = {k: v.cpu() for k, v in O.reference(inp, grad_out, th.float64, DEV).items()}
        r32 = {k: v.cpu() for k, v in O.reference(inp, grad_out, th.float32, DEV).items()} if dtype == th.float32 else None
        check(got, r64, r32, dtype, "N65537")
        assert float(r64["grad_light_dir"].abs().max()) > 0 and float(r64["grad_ambient"][N - 100:].abs().max()) > 0


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _tutorial_step(dtype, index_img, use_shade):
    """transform -> render -> interpolate([normals, positions]) -> shading -> edge_grad_estimator -> loss on a lobed sphere,
    two views at 64 x 64; the shading is drtk_amd.shade or the tutorial's eager formulation.  (image, gradient to the vertices)"""
    import drtk_amd
    from drtk_amd.synthetic import ring_cameras, uv_sphere

    N, H, W = 2, 64, 64
    v0, vi = uv_sphere(12, 16, lobes=0.15, device=DEV, dtype=dtype)
    campos, camrot, focal, princpt = ring_cameras(N, W, H, device=DEV, dtype=dtype)
    v = v0[None].expand(N, -1, -1).contiguous().requires_grad_(True)
    v_pix, v_cam = drtk_amd.transform_with_v_cam(v, campos, camrot, focal, princpt)
    if index_img is None:
        index_img = drtk_amd.rasterize(v_pix, vi, H, W)
    _, bary_img = drtk_amd.render(v_pix, vi, index_img)
    attr = drtk_amd.interpolate(th.cat([drtk_amd.vert_normals(v_cam, vi), v_cam], -1), vi, index_img, bary_img)
    t = lambda *x: th.tensor(x, dtype=dtype, device=DEV)  # noqa: E731
    light, albedo, ambient, specular, gloss = t(0.3, 0.4, 0.85), t(0.8, 0.6, 0.5), t(0.2, 0.25, 0.3), t(0.5, 0.5, 0.6), t(0.4)
    gen = th.Generator().manual_seed(2)
    bg = (0.1 + 0.8 * th.rand(1, 3, H, W, generator=gen)).to(DEV, dtype).expand(N, -1, -1, -1)
    if use_shade:
        img = drtk_amd.shade(attr[:, 0:3], light, albedo, ambient, index_img, attr[:, 3:6], specular, (gloss * 40).view(1), bg, 2.2)
    else:
        row = lambda p: p.view(1, -1).expand(N, -1)  # noqa: E731
        img = O.tutorial_shade(attr[:, 0:3], row(light), row(albedo), row(ambient), index_img, attr[:, 3:6], row(specular), row(gloss), bg)
    img = drtk_amd.edge_grad_estimator(v_pix=v_pix, vi=vi, bary_img=bary_img, img=img, index_img=index_img)
    target = (0.5 + 0.4 * th.cos(th.arange(N * 3 * H * W, dtype=th.float64) * 0.11)).view(N, 3, H, W).to(DEV, dtype)
    ((img - target) ** 2).mean().backward()
    return img.detach().cpu(), v.grad.cpu(), index_img


def test_the_tutorials_step_end_to_end_against_the_eager_shading():
    img, grad, index_img = _tutorial_step(th.float32, None, True)
    assert 0.2 < float((index_img != -1).float().mean()) < 0.9
    e32 = _tutorial_step(th.float32, index_img, False)
    e64 = _tutorial_step(th.float64, index_img, False)
    s64 = _tutorial_step(th.float64, index_img, True)
    assert bool(th.isfinite(grad).all()) and float(grad.abs().max()) > 0
    for what, a, a64, b32, b64 in (("image", img, s64[0], e32[0], e64[0]), ("grad_v", grad, s64[1], e32[1], e64[1])):
        err = float((a64 - b64).abs().max())
        print(f"end to end {what}: float64 |shade - eager| = {err:.3e}, max = {float(b64.abs().max()):.3e}")
        assert err <= 1e-12 * max(1.0, float(b64.abs().max())), what
        assert_within_f64_distance(a, b32, b64, f"end to end {what}")


def test_c_abi_between_sentinels_in_a_child_process():
    env = dict(os.environ, DRTK_CAPI_GUARD="1", DRTK_CAPI_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_shade.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cases passed" in r.stdout
