"""GPU (-m gpu): `filter2d` -- fused separable up/down-sampling FIR filters -- through the C ABI and through the Python
functions under autograd, against the CPU oracle of tests/filter2d_oracle.py (which tests/test_filter2d_host.py holds to the
fixtures recorded from the reference's PyTorch model).

Bounds (nothing hand-picked):
  float32   assert_within_f64_distance (tests/f64_distance.py) with its defaults -- oracle_f32 the oracle on the float32
            inputs, oracle_f64 the same inputs cast up, acc_magnitude the largest magnitude the oracle accumulates into an
            element (the operator on |x|, |f|);
  float64   1e-12 * max|ref|;
  float16   per element 2^-11 |y_f64| for the rounding of the output itself, plus the float32 bound (the sums are float32);
            the oracle runs in float64 on the half-rounded inputs;
  tuned instantiation against the generic one: k 2^-24 sum|f| max|x| -- only the order of summation may differ."""
import pytest
import torch as th

import filter2d_oracle as O
from f64_distance import assert_within_f64_distance, f64_distance_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def hip(name, padding, dtype, api):
    """(out, grad_x or None) of the kernels as CPU tensors.  api: `python` (resample_filter under autograd) | `capi`."""
    x, f, gout, up, down = O.make_case(name)
    return hip_on(x.to(DEV, dtype), f.to(DEV), gout.to(DEV, dtype), up, down, padding, api, O.divisible(name))


def hip_on(x, f, gout, up, down, padding, api, divisible=True):
    """`hip` on any device tensors, x in the layout it comes in (shared with tests/fuzz_added_ops.py)."""
    import drtk_amd
    from drtk_amd import capi

    reflect = padding == "reflection"
    if api == "capi":
        out = capi.filter2d(x, f, up, down, reflect)
        grad = capi.filter2d(gout, f, down, up, reflect, backward=True) if divisible else None
    else:
        x, f = x.detach().requires_grad_(True), f.detach().requires_grad_(True)
        out = drtk_amd.resample_filter(x, f, up, down, padding)
        grad = None
        if divisible:
            out.backward(gout)
            assert f.grad is None  # the filter gets no gradient
            grad = x.grad
    return out.detach().cpu(), None if grad is None else grad.cpu()


@pytest.mark.parametrize("api", ["capi", "python"])
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,padding", O.CASE_PADDINGS)
def test_cases_against_the_oracle(name, padding, dtype, api):
    x, f, gout, up, down = O.make_case(name)
    e = O.expected(name, padding)
    out, grad = hip(name, padding, dtype, api)
    assert out.dtype == dtype and out.shape == e["out64"].shape == gout.shape
    assert O.divisible(name) and grad.dtype == dtype and grad.shape == x.shape
    if dtype == th.float32:
        a = assert_within_f64_distance(out, e["out32"], e["out64"], f"{name} {padding} out", acc_magnitude=float(e["out_mag"].max()))
        b = assert_within_f64_distance(grad, e["grad32"], e["grad64"], f"{name} {padding} grad_x", acc_magnitude=float(e["grad_mag"].max()))
        print(f"{name} {padding} {api}: |out - f64| = {a[0]:.3e} (oracle f32 {a[1]:.3e}), |grad - f64| = {b[0]:.3e} (oracle f32 {b[1]:.3e})")
    else:
        a = float((out - e["out64"]).abs().max())
        b = float((grad - e["grad64"]).abs().max())
        print(f"{name} {padding} {api} f64: |out - ref| = {a:.3e}, |grad - ref| = {b:.3e}")
        assert a <= 1e-12 * float(e["out64"].abs().max())
        assert b <= 1e-12 * float(e["grad64"].abs().max())


@pytest.mark.parametrize("name", ["up2", "down2", "filt5"])
@pytest.mark.parametrize("padding", O.BOTH)
def test_half_is_storage_only(name, padding):
    import drtk_amd

    x, f, gout, up, down = O.make_case(name)
    xh, gh = x.half(), gout.half()
    reflect = padding == "reflection"
    xd = xh.to(DEV).requires_grad_(True)
    out = drtk_amd.resample_filter(xd, f.to(DEV), up, down, padding)
    out.backward(gh.to(DEV))
    assert out.dtype == th.float16 and xd.grad.dtype == th.float16 and xd.grad.shape == x.shape
    for got, inp, args, what in ((out.detach().cpu(), xh, (up, down, reflect, False), "out"), (xd.grad.cpu(), gh, (down, up, reflect, True), "grad_x")):
        ref64 = O.apply(inp.double(), f, *args)
        ref32 = O.apply(inp.float(), f, *args)
        mag = O.apply(inp.double(), f, *args, absolute=True)
        assert got.shape == ref64.shape
        f32_bound, _ = f64_distance_bound(ref32, ref64, acc_magnitude=float(mag.max()))
        excess = (got.double() - ref64).abs() - (2.0 ** -11 * ref64.abs() + f32_bound)
        print(f"{name} {padding} half {what}: worst |y - f64| - bound = {float(excess.max()):.3e}")
        assert bool(th.isfinite(got).all()) and float(excess.max()) <= 0


def test_named_operators_are_resample_filter_with_their_kernel_bit_for_bit():
    import drtk_amd

    g = th.Generator().manual_seed(11)
    x = (th.rand(2, 3, 26, 34, generator=g) * 2 - 1).to(DEV)
    for filter_type in drtk_amd.FilterType:
        for padding in O.BOTH:
            opt = drtk_amd.FilterOptions(6, filter_type, 0.5)
            for m in (2, 4):
                f = drtk_amd.make_resampling_kernel(opt, m, 1.0, float(m), device=x.device)
                assert f.device == x.device and f.shape == (6 * m,)
                assert th.equal(drtk_amd.upsample(x, opt, m, padding), drtk_amd.resample_filter(x, f, m, 1, padding))
                f = drtk_amd.make_resampling_kernel(opt, m, 1.0, 1.0, device=x.device)
                assert th.equal(drtk_amd.downsample(x, opt, m, padding), drtk_amd.resample_filter(x, f, 1, m, padding))
            f = drtk_amd.make_resampling_kernel(opt, 1, 2.0, 1.0, device=x.device)
            assert th.equal(drtk_amd.low_pass_filter(x, opt, 2.0, padding), drtk_amd.resample_filter(x, f, 1, 1, padding))
            assert th.equal(drtk_amd.filter(x, f, padding), drtk_amd.resample_filter(x, f, 1, 1, padding))
    # the device filter is the CPU filter, and cached
    opt = drtk_amd.FilterOptions()
    f = drtk_amd.make_resampling_kernel(opt, 2, 1.0, 2.0, device=x.device)
    assert drtk_amd.make_resampling_kernel(opt, 2, 1.0, 2.0, device=x.device) is f
    assert th.equal(f.cpu(), drtk_amd.make_resampling_kernel(opt, 2, 1.0, 2.0))


@pytest.mark.parametrize("name", ["up2", "down4", "filt65", "generic_3_2_12"])
def test_two_calls_give_bitwise_equal_results(name):
    from drtk_amd import capi

    x, f, gout, up, down = O.make_case(name)
    x, f = x.to(DEV), f.to(DEV)
    for reflect in (False, True):
        assert th.equal(capi.filter2d(x, f, up, down, reflect), capi.filter2d(x, f, up, down, reflect))


@pytest.mark.parametrize("dtype", [th.float32, th.float64, th.float16], ids=["f32", "f64", "f16"])
@pytest.mark.parametrize("name", O.TUNED)
def test_tuned_and_generic_instantiations_agree(name, dtype):
    from drtk_amd import capi

    x, f, gout, up, down = O.make_case(name)
    k = f.shape[0]
    for padding in O.CASES[name][4]:
        reflect = padding == "reflection"
        for inp, (u, d, bwd) in ((x, (up, down, False)), (gout, (down, up, True))):
            inp = inp.to(DEV, dtype)
            tuned = capi.filter2d(inp, f.to(DEV), u, d, reflect, bwd)
            generic = capi.filter2d(inp, f.to(DEV), u, d, reflect, bwd, force_generic=True)
            assert tuned.shape == generic.shape and bool(th.isfinite(tuned).all())
            bound = k * 2.0 ** -24 * float(f.abs().sum()) * float(inp.abs().max())
            if dtype == th.float16:
                bound += 2.0 ** -11 * float(generic.abs().max())  # the two roundings of the output may fall on either side
            assert float((tuned.double() - generic.double()).abs().max()) <= bound, (name, padding, bwd)


def check_family(up, down, k, dtype, padding):
    """The forward (up, down, k) and its gradient call (down, up, k, backward) on O.family_case through the C ABI against the
    oracle under the bounds of this file's docstring -- the oracle runs on what the image type holds (the inputs rounded to
    float16 for a half image) --, and, where (up, down, k) is a tuned family, the tuned instantiation against the generic
    one.  Shared with tests/guarded_added_ops.py.  -> {"out" | "grad_x": (worst error, its bound)} against the oracle."""
    x, f, gout = O.family_case(up, down, k)
    return check_inputs(x, f, gout, up, down, dtype, padding, O.family_expected(up, down, k, padding, dtype == th.float16))


def check_inputs(x, f, gout, up, down, dtype, padding, e):
    """check_family on any float32 CPU tensors x, f, grad_out with `e` the oracle's results on them, in the form of
    O.family_expected (shared with tests/fuzz_added_ops.py)."""
    from drtk_amd import capi

    k = f.shape[0]
    half = dtype == th.float16
    reflect = padding == "reflection"
    fd = f.to(DEV)
    figures = {}
    for what, inp, (u, d, bwd), tag in (("out", x, (up, down, False), "out"), ("grad_x", gout, (down, up, True), "grad")):
        inp = inp.to(DEV, dtype)
        tuned = capi.filter2d(inp, fd, u, d, reflect, bwd)
        got = tuned.cpu()
        ref32, ref64, mag = e[tag + "32"], e[tag + "64"], e[tag + "_mag"]
        name = f"({up}, {down}, {k}) {padding} {str(dtype).split('.')[-1]} {what}"
        assert got.dtype == dtype and got.shape == ref64.shape and got.shape == (gout if what == "out" else x).shape, name
        assert bool(th.isfinite(got).all()), name
        if dtype == th.float32:
            bound, _ = f64_distance_bound(ref32, ref64, acc_magnitude=float(mag.max()))
            err, own = assert_within_f64_distance(got, ref32, ref64, name, acc_magnitude=float(mag.max()))
            print(f"{name}: |kernel - f64| = {err:.3e} (oracle f32 {own:.3e}), bound {bound:.3e}")
        elif dtype == th.float64:
            err, bound = float((got - ref64).abs().max()), 1e-12 * float(ref64.abs().max())
            print(f"{name}: |kernel - ref| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
        else:
            f32_bound, _ = f64_distance_bound(ref32, ref64, acc_magnitude=float(mag.max()))
            excess = (got.double() - ref64).abs() - (2.0 ** -11 * ref64.abs() + f32_bound)
            err, bound = float((got.double() - ref64).abs().max()), float((2.0 ** -11 * ref64.abs() + f32_bound).max())
            print(f"{name}: worst |y - f64| - bound = {float(excess.max()):.3e} (|y - f64| = {err:.3e})")
            assert float(excess.max()) <= 0, f"{name}: an element is {float(excess.max()):.3e} beyond its bound"
        figures[what] = (err, bound)
        if (u, d, k) in O.FAMILIES:
            generic = capi.filter2d(inp, fd, u, d, reflect, bwd, force_generic=True)
            assert tuned.shape == generic.shape and bool(th.isfinite(generic).all()), name
            bound = k * 2.0 ** -24 * float(f.abs().sum()) * float(inp.abs().max())
            if half:
                bound += 2.0 ** -11 * float(generic.abs().max())  # the two roundings of the output may fall on either side
            err = float((tuned.double() - generic.double()).abs().max())
            assert err <= bound, f"{name}: tuned against generic {err:.3e} > {bound:.3e}"
    return figures


@pytest.mark.parametrize("padding", O.BOTH)
@pytest.mark.parametrize("dtype", [th.float32, th.float64, th.float16], ids=["f32", "f64", "f16"])
@pytest.mark.parametrize("up,down,k", O.FAMILIES)
def test_every_tuned_family_against_the_oracle(up, down, k, dtype, padding):
    """Every compiled (up, down, k) in every storage type with either setting of the `backward` flag (the gradient call of
    (up, down, k) is the family (down, up, k)), under both paddings, on an output of O.FAMILY_OUT: two tiles and a ragged
    last tile per axis at every tile shape the planner may choose (tests/test_filter2d_host.py asserts that, and that
    FAMILIES is the tuned set of the source)."""
    check_family(up, down, k, dtype, padding)


def test_non_contiguous_x_and_grad_out():
    import drtk_amd

    x, f, gout, up, down = O.make_case("down2")
    x, f, gout = x.to(DEV), f.to(DEV), gout.to(DEV)
    wide = th.cat([x, x.flip(3)], 3)
    xs = wide[..., : x.shape[3]]
    tall = th.cat([gout, -gout], 2)
    gs = tall[:, :, : gout.shape[2]]
    assert not xs.is_contiguous() and not gs.is_contiguous()
    a = x.clone().requires_grad_(True)
    ya = drtk_amd.resample_filter(a, f, up, down)
    ya.backward(gout)
    b = xs.detach().requires_grad_(True)
    yb = drtk_amd.resample_filter(b, f, up, down)
    yb.backward(gs)
    assert th.equal(ya, yb) and th.equal(a.grad, b.grad)
    # a permuted (channels-last) image and gradient too
    c = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).detach().requires_grad_(True)
    yc = drtk_amd.resample_filter(c, f, up, down)
    yc.backward(gout.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert th.equal(ya, yc) and th.equal(a.grad, c.grad)


def test_no_graph_without_requires_grad_and_no_gradient_for_f():
    import drtk_amd

    x, f, gout, up, down = O.make_case("up2")
    x, f = x.to(DEV), f.to(DEV)
    opt = drtk_amd.FilterOptions()
    for y in (drtk_amd.resample_filter(x, f, up, down), drtk_amd.upsample(x, opt), drtk_amd.downsample(x, opt), drtk_amd.low_pass_filter(x, opt)):
        assert not y.requires_grad and y.grad_fn is None
    fr = f.clone().requires_grad_(True)
    y = drtk_amd.resample_filter(x, fr, up, down)
    assert y.requires_grad  # an input asks for a gradient ...
    assert th.autograd.grad(y.sum(), fr, allow_unused=True)[0] is None  # ... and gets an undefined one


def test_double_backward():
    """d/d(grad_out) of (grad_x . r).sum() is the forward operator applied to r: the backward goes through the operator."""
    import drtk_amd

    x, f, gout, up, down = O.make_case("up2")
    g = th.Generator().manual_seed(3)
    r = th.rand(x.shape, generator=g, dtype=th.float64) * 2 - 1
    xd = x.double().to(DEV).requires_grad_(True)
    go = gout.double().to(DEV).requires_grad_(True)
    y = drtk_amd.resample_filter(xd, f.to(DEV), up, down, "zeros")
    (gx,) = th.autograd.grad(y, xd, go, create_graph=True)
    (gg,) = th.autograd.grad((gx * r.to(DEV)).sum(), go)
    want = O.apply(r, f, up, down, False)
    assert gg.shape == want.shape
    assert float((gg.cpu() - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_backward_of_a_decimation_that_does_not_divide_the_image_raises():
    import drtk_amd

    x = th.rand(1, 2, 13, 17, device=DEV, requires_grad=True)
    y = drtk_amd.downsample(x, drtk_amd.FilterOptions(), 2)  # the forward is unaffected
    assert y.shape == (1, 2, O.output_size(13, 12, 1, 2), O.output_size(17, 12, 1, 2)) == (1, 2, 6, 8)
    with pytest.raises(RuntimeError, match=r"input of 13x17 comes out 12x16 .*multiples of down"):
        y.sum().backward()


def test_reflection_on_an_image_smaller_than_the_halo_raises_before_any_launch():
    import drtk_amd
    from drtk_amd import capi

    x = th.rand(1, 1, 3, 40, device=DEV)
    with pytest.raises(RuntimeError, match="reflection padding of"):
        drtk_amd.resample_filter(x, th.ones(9, device=DEV), 1, 1, "reflection")
    with pytest.raises(capi.DrtkAmdError, match="invalid argument"):
        capi.filter2d(x, th.ones(9, device=DEV), 1, 1, True)
    assert drtk_amd.resample_filter(x, th.ones(9, device=DEV), 1, 1, "zeros").shape == x.shape
    with pytest.raises(RuntimeError, match="f must reside on the same device as x"):
        drtk_amd.resample_filter(x, th.ones(3))


@pytest.mark.parametrize("dtype", [th.float32, th.float64, th.float16], ids=["f32", "f64", "f16"])
def test_every_output_element_is_written(dtype):
    """The binding pre-fills what it allocates with NaN (DRTK_CAPI_POISON, tests/conftest.py): ragged last tiles in both
    axes, images narrower than a tile, tiles of every width the planner chooses."""
    from drtk_amd import capi

    for (up, down, k), (H, W) in (((1, 1, 5), (33, 65)), ((1, 1, 65), (40, 70)), ((2, 1, 12), (17, 33)), ((1, 2, 12), (70, 134)),
                                  ((1, 8, 48), (88, 136)), ((8, 1, 32), (9, 9)), ((3, 2, 12), (23, 47)), ((1, 1, 1), (1, 1))):
        x = th.ones(1, 3, H, W, device=DEV, dtype=dtype)
        f = th.full((k,), 1.0 / k, device=DEV)
        y = capi.filter2d(x, f, up, down, False)
        assert y.shape[2:] == (O.output_size(H, k, up, down), O.output_size(W, k, up, down))
        assert bool(th.isfinite(y).all()), (up, down, k)


def test_graph_capture_and_replay_with_other_work_between_replays():
    import drtk_amd

    g = th.Generator().manual_seed(5)
    x0 = (th.rand(2, 2, 19, 41, generator=g) * 2 - 1).to(DEV)
    x = x0.clone()
    opt = drtk_amd.FilterOptions()

    def step():
        up = drtk_amd.upsample(x, opt, 2)
        return up, drtk_amd.downsample(up, opt, 2)

    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        step()  # the warm-up: the two filters are made (one host-to-device copy each) before the capture
    th.cuda.current_stream().wait_stream(side)
    th.cuda.synchronize()
    graph = th.cuda.CUDAGraph()
    with th.cuda.graph(graph):
        out = step()
    for k, scale in enumerate((1.0, -0.5)):
        x.copy_(x0 * scale)  # an unrelated eager kernel between the replays
        graph.replay()
        th.cuda.synchronize()
        got = [t.clone() for t in out]
        want = step()
        th.cuda.synchronize()
        assert got[0].shape == (2, 2, 38, 82) and got[1].shape == x.shape
        for a, b in zip(got, want):
            assert th.equal(a, b), f"replay {k} differs from the eager result"
        _ = float((got[1] * 2).sum())
