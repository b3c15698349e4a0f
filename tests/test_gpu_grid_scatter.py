"""GPU (-m gpu): `grid_scatter` -- the splatting counterpart of grid_sample -- through the C ABI, the torch operator under
autograd and the Python API, against the CPU oracles of tests/grid_scatter_oracle.py: the adjoint of
torch.nn.functional.grid_sample wherever it is the statement of what the kernel computes, the float64 restatement of the
reference kernel's coordinate rule for bicubic border / reflection outside [0, size - 1], and the recorded outputs of the
reference's own PyTorch model (tests/golden/grid_scatter_*.npz).

Bounds (tests/f64_distance.py, nothing hand-picked):
  float32   max norm: assert_within_f64_distance with its defaults (oracle_f32 = torch CPU on the float32 inputs,
            oracle_f64 = the same inputs cast up); per element: elementwise_excess with the accumulated magnitudes A of
            the oracle module and ULPS below -- at most 4 x what the float32 CPU oracle itself uses of u * A over the cases
            of this file (the kernel sums the same terms in another, partly tree-shaped order);
  float64   1e-12 * max|ref|;
  grad_grid pixels at which the float32 and float64 evaluations of the coordinate pick another floor cell or clip /
            reflect branch (grid_scatter_oracle.flip_pixels, from the grid alone) are left out -- never more than 1e-4
            of a case's pixels, more is a failure."""
import itertools
import os

import numpy as np
import pytest
import torch as th
from conftest import GOLDEN

import grid_scatter_oracle as O
from f64_distance import assert_within_f64_distance, elementwise_excess

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("out", "grad_input", "grad_grid")
# Per element, two allowances (elementwise_excess: |kernel - f64| <= max(3 |oracle_f32 - f64|, ulps * u * magnitude)):
#   "A"    the accumulated magnitudes alone.  ulps = 4 x the largest |oracle_f32 - f64| / (u A) of the float32 CPU oracle
#          itself over the float32 cases of this file (a CPU-only quantity; the last test of a run prints it): MEASURED_A.  That maximum is set by elements
#          fed through weights near zero, whose error is absolute in the weight (grid_scatter_oracle.coordinate_sensitivity):
#          it is millions to billions of u A (one more case moved it from 2.9e8 to 5.6e11), and the allowance that
#          follows from it says little;
#   "A+S"  the accumulated magnitudes plus the coordinate sensitivity S, the scale two correct float32 evaluations of an
#          element differ by.  ulps = 4 x the same measurement against u (A + S): MEASURED_AS.  This is the check with teeth.
MEASURED_A = {"out": 5.63e11, "grad_input": 1.93e7, "grad_grid": 1.55e7}
MEASURED_AS = {"out": 1.93, "grad_input": 2.83, "grad_grid": 3.51}
ULPS = {"A": {k: 4 * v for k, v in MEASURED_A.items()}, "A+S": {k: 4 * v for k, v in MEASURED_AS.items()}}
OWN = {kind: {k: 0.0 for k in NAMES} for kind in ULPS}  # the float32 oracle's own use of each, collected while the tests run
FIXTURES = sorted(f[len("grid_scatter_"):-4] for f in os.listdir(GOLDEN) if f.startswith("grid_scatter_") and f.endswith(".npz"))


def oracle(inp, grid, gout, oh, ow, mode, pad, al):
    """(out, grad_input, grad_grid) of the CPU oracle in the dtype of the arguments: the adjoint of grid_sample where the
    two coordinate rules coincide for this grid, the restatement of the reference kernel's rule where they do not."""
    if O.rules_coincide(grid, oh, ow, mode, pad, al):
        return (O.scatter(inp, grid, oh, ow, mode, pad, al),) + O.scatter_backward(gout, inp, grid, mode, pad, al)
    return O.restate(inp, grid, oh, ow, mode, pad, al, gout)


def hip(inp, grid, gout, oh, ow, mode, pad, al, api="python", needs=(True, True), counts=None, as_uv_image=False):
    """The kernels' (out, grad_input, grad_grid) as CPU tensors (None where not asked for).  api: `python`
    (drtk_amd.grid_scatter under autograd) | `capi` (the ctypes binding of the C ABI).  as_uv_image: the grid handed over
    as a channel-first [N,2,H,W] image seen through permute(0, 2, 3, 1)."""
    import drtk_amd
    from drtk_amd import capi

    x, g, go = inp.to(DEV), grid.to(DEV), gout.to(DEV)
    if as_uv_image:
        g = g.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
        assert not g.is_contiguous()
    if api == "capi":
        out = capi.grid_scatter_2d(x, g, oh, ow, O.PADDING_ENUM[pad], O.MODE_ENUM[mode], al, route_counts=counts)
        gi, gg = capi.grid_scatter_2d_backward(go, x, g, O.PADDING_ENUM[pad], O.MODE_ENUM[mode], al, needs[0], needs[1])
    else:
        assert counts is None
        x, g = x.requires_grad_(needs[0]), g.requires_grad_(needs[1])
        out = drtk_amd.grid_scatter(x, g, oh, ow, mode, pad, al)
        assert out.requires_grad == (needs[0] or needs[1])
        if out.requires_grad:
            out.backward(go)
        gi, gg = x.grad, g.grad
        assert (gi is not None) == needs[0] and (gg is not None) == needs[1]
    if gg is not None and as_uv_image:
        assert gg.stride() == g.stride(), "grad_grid is laid out like the grid it belongs to"
    th.cuda.synchronize()
    return tuple(None if t is None else t.detach().cpu() for t in (out, gi, gg))


def compare(got, inp, grid, gout, oh, ow, mode, pad, al, what, want=None):
    """got = (out, grad_input, grad_grid) (None: not compared) against the oracle under the bounds of the docstring.
    want: recorded reference outputs to use as the oracle in the dtype of the inputs (fixtures)."""
    assert got[0].shape == (inp.shape[0], inp.shape[1], oh, ow) and got[0].dtype == inp.dtype
    if inp.dtype == th.float64:
        ref = want if want is not None else oracle(inp, grid, gout, oh, ow, mode, pad, al)
        for name, g, r in zip(NAMES, got, ref):
            if g is not None:
                err, tol = float((g - r).abs().max()), 1e-12 * float(r.abs().max())
                assert err <= tol, f"{what}: {name}: {err:.3e} > {tol:.3e}"
        return
    o32 = want if want is not None else oracle(inp, grid, gout, oh, ow, mode, pad, al)
    o64 = oracle(inp.double(), grid.double(), gout.double(), oh, ow, mode, pad, al)
    A = O.magnitudes(inp, grid, oh, ow, mode, pad, al, gout)
    S = O.coordinate_sensitivity(inp, grid, oh, ow, mode, pad, al, gout)
    flagged = O.flip_pixels(grid, oh, ow, pad, al)
    assert int(flagged.sum()) <= O.FLIP_CAP * flagged.numel(), f"{what}: {int(flagged.sum())} of {flagged.numel()} pixels flip their cell between float32 and float64"
    for name, g, a, b, m, sens in zip(NAMES, got, o32, o64, A, S):
        if g is None:
            continue
        if name == "grad_grid" and bool(flagged.any()):
            keep = ~flagged[..., None].expand_as(g)
            g, a, b, m, sens = (th.where(keep, t.double(), th.zeros((), dtype=th.float64)) for t in (g, a, b, m, sens))
        err, own_err = assert_within_f64_distance(g, a, b, f"{what}: {name}")
        print(f"{what}: {name}: |kernel - f64| {err:.3e}, |oracle_f32 - f64| {own_err:.3e}")
        for kind, mags in (("A", m), ("A+S", m + sens)):
            ulps = ULPS[kind][name]
            excess, worst, own = elementwise_excess(g, a, b, mags, ulps)
            OWN[kind][name] = max(OWN[kind][name], own * ulps)
            print(f"    per element against u {kind}: {excess:.3f} of the bound (the float32 oracle alone uses {own * ulps:.3g} u {kind})")
            assert excess <= 1.0, (f"{what}: {name}: element {worst} is {excess:.2f} x its bound max(3 |oracle_f32 - f64|, {ulps:.3g} u ({kind})) "
                                   f"(kernel {float(g.flatten()[worst]):.9e}, f64 {float(b.flatten()[worst]):.9e}, {kind} {float(mags.flatten()[worst]):.3e})")


def route_counts():
    return th.zeros(2, dtype=th.int32, device=DEV)


def tiles(N, H, W):
    return N * ((H + 15) // 16) * ((W + 15) // 16)


# ---------------------------------------------------------------------------------------------------------------------
# recorded outputs of the reference's PyTorch model
# ---------------------------------------------------------------------------------------------------------------------
def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, "grid_scatter_" + name + ".npz"))
    t = lambda k: th.from_numpy(np.ascontiguousarray(z[k]))  # noqa: E731
    mode = {0: "bilinear", 2: "bicubic"}[int(z["in_mode"])]
    pad = O.PADDINGS[int(z["in_padding"])]
    args = (t("in_input"), t("in_grid"), t("in_grad_out"), int(z["in_oh"]), int(z["in_ow"]), mode, pad, bool(int(z["in_align"])))
    return args, (t("out_out"), t("out_grad_input"), t("out_grad_grid"))


@pytest.mark.parametrize("api", ["capi", "python"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_of_the_reference_model(name, api):
    assert len(FIXTURES) >= 6
    args, want = load_fixture(name)
    compare(hip(*args, api=api), *args, f"{name} ({api})", want=want)


# ---------------------------------------------------------------------------------------------------------------------
# every mode x padding x align_corners, float32 and float64, C in {1, 3, 4, 7}
# ---------------------------------------------------------------------------------------------------------------------
SWEEP = list(itertools.product(O.MODES, O.PADDINGS, (False, True), (th.float32, th.float64)))
SWEEP_C = (1, 3, 4, 7)


def sweep_case(mode, pad, al, dtype, C):
    """Sizes that are no multiple of the tile; the small output fits one window (every tile windowed), the larger one under
    a uniformly random grid does not (every tile direct).  Seeds are fixed: no pixel of these grids flips its cell."""
    oh, ow = ((30, 45), (61, 83), (30, 45), (61, 83))[SWEEP_C.index(C)]
    seed = 1000 + 97 * SWEEP.index((mode, pad, al, dtype)) + C
    inp, grid, gout = O.make_case(seed, 2, C, 37, 53, oh, ow, dtype=dtype, kind="uniform", extent=1.2)
    return inp, grid, gout, oh, ow, mode, pad, al


@pytest.mark.parametrize("mode,pad,al,dtype", SWEEP, ids=lambda v: str(v).replace("torch.", ""))
def test_mode_sweep_forward_and_both_gradients_and_each_gradient_alone(mode, pad, al, dtype):
    for C in SWEEP_C:
        args = sweep_case(mode, pad, al, dtype, C)
        what = f"{mode} {pad} align_corners={al} {dtype} C={C}"
        both = hip(*args)
        compare(both, *args, what)
        # each gradient alone: the backward is a gather, bit-identical whatever else is computed; neither: no graph
        only_input = hip(*args, needs=(True, False))
        only_grid = hip(*args, needs=(False, True))
        assert only_input[2] is None and th.equal(only_input[1], both[1]), what
        assert only_grid[1] is None and th.equal(only_grid[2], both[2]), what
        compare(only_input, *args, what + " (input gradient alone)")
        none = hip(*args, needs=(False, False))
        assert none[1] is None and none[2] is None
        compare(none, *args, what + " (no gradient)")
        if C == 3:
            compare(hip(*args, api="capi"), *args, what + " (C ABI)")


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_adjoint_identity_against_the_device_grid_sample(mode, dtype):
    """<scatter(x, g), y> = <x, grid_sample(y, g)> with torch's own grid_sample on the device"""
    import drtk_amd

    for pad, al in itertools.product(O.PADDINGS, (False, True)):
        extent = 1.2 if (mode == "bilinear" or pad == "zeros") else 0.93  # (where the two coordinate rules coincide)
        x, g, y = (t.to(DEV) for t in O.make_case(7, 2, 5, 70, 90, 64, 100, dtype=dtype, kind="uniform", extent=extent))
        assert O.rules_coincide(g.cpu(), 64, 100, mode, pad, al)
        lhs = (drtk_amd.grid_scatter(x, g, 64, 100, mode, pad, al).double() * y.double()).sum()
        s = th.nn.functional.grid_sample(y, g, mode=mode, padding_mode=pad, align_corners=al)
        rhs = (x.double() * s.double()).sum()
        scale = float((x.double().abs() * th.nn.functional.grid_sample(y.abs(), g, mode="bilinear", padding_mode=pad, align_corners=al).double().abs()).sum())
        u = 2.0 ** -24 if dtype == th.float32 else 2.0 ** -53
        # Both sides are the same sum of N*H*W*C*taps products x * w * y, grouped by texel (left) or by pixel (right) in the
        # element type and then added up in double.  A group has at most a few dozen terms here (<= 16 taps per pixel; the
        # uniform grid puts ~4 (bilinear) / ~16 (bicubic) contributions on a texel), each term carries <= 4 roundings of its
        # factors: worst case < 64 u of the sum of the absolute products (`scale`, with the bicubic weights' absolute sum
        # (1.27)^2 < 4 times the bilinear weights' it is computed from).
        assert abs(float(lhs - rhs)) <= 64 * u * max(scale, 1.0) * (4 if mode == "bicubic" else 1), (mode, pad, al, float(lhs), float(rhs))


# ---------------------------------------------------------------------------------------------------------------------
# kernel routes, proven by the route counters of the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", O.MODES)
def test_routes_smooth_warp_is_windowed_and_random_grid_is_direct(mode):
    N, C, H, W = 2, 3, 150, 203
    args = O.make_case(31, N, C, H, W, 144, 200, kind="warp", extent=0.97) + (144, 200, mode, "border", False)
    counts = route_counts()
    compare(hip(*args, api="capi", counts=counts), *args, f"smooth warp {mode}")
    assert counts.tolist() == [tiles(N, H, W), 0], counts.tolist()

    args = O.make_case(32, N, C, H, W, 256, 256, kind="uniform", extent=1.1) + (256, 256, mode, "border", False)
    counts = route_counts()
    compare(hip(*args, api="capi", counts=counts), *args, f"random grid {mode}")
    assert counts.tolist() == [0, tiles(N, H, W)], counts.tolist()


def identity_grid(N, H, W, scale=1.0):
    ys = (th.arange(H, dtype=th.float64) * 2 + 1) / H - 1
    xs = (th.arange(W, dtype=th.float64) * 2 + 1) / W - 1
    yy, xx = th.meshgrid(ys, xs, indexing="ij")
    return (th.stack([xx, yy], -1) * scale)[None].expand(N, -1, -1, -1).contiguous()


@pytest.mark.parametrize("mode", O.MODES)
def test_routes_minification_magnification_and_everything_on_one_texel(mode):
    g = th.Generator().manual_seed(5)
    # 16 x minification: 256^2 pixels onto 16^2 texels -- every tile touches a handful of texels: windowed
    # (the irrational scale keeps the pixels off the texel boundaries, where the cell would be a matter of rounding)
    N, C, H, W, oh, ow = 1, 4, 256, 256, 16, 16
    inp, gout = th.rand(N, C, H, W, generator=g) * 2 - 1, th.rand(N, C, oh, ow, generator=g) * 2 - 1
    args = (inp, identity_grid(N, H, W, 0.98765).float(), gout, oh, ow, mode, "zeros", False)
    counts = route_counts()
    compare(hip(*args, api="capi", counts=counts), *args, f"16x minification {mode}")
    assert counts.tolist() == [tiles(N, H, W), 0], counts.tolist()
    # 16 x magnification: a tile of 16 x 16 pixels spans 256 x 256 texels: direct
    N, C, H, W, oh, ow = 1, 3, 40, 40, 640, 640
    inp, gout = th.rand(N, C, H, W, generator=g) * 2 - 1, th.rand(N, C, oh, ow, generator=g) * 2 - 1
    args = (inp, identity_grid(N, H, W, 0.98765).float(), gout, oh, ow, mode, "zeros", False)
    counts = route_counts()
    compare(hip(*args, api="capi", counts=counts), *args, f"16x magnification {mode}")
    assert counts.tolist() == [0, tiles(N, H, W)], counts.tolist()
    # every pixel aimed at one texel (between four): windowed, one atomic per texel, channel and tile
    N, C, H, W, oh, ow = 2, 3, 100, 90, 31, 47
    inp, gout = th.rand(N, C, H, W, generator=g) * 2 - 1, th.rand(N, C, oh, ow, generator=g) * 2 - 1
    grid = th.tensor([0.137, -0.291]).expand(N, H, W, 2).contiguous()
    args = (inp, grid, gout, oh, ow, mode, "border", False)
    counts = route_counts()
    got = hip(*args, api="capi", counts=counts)
    compare(got, *args, f"all to one texel {mode}")
    assert counts.tolist() == [tiles(N, H, W), 0], counts.tolist()
    assert int((got[0] != 0).sum()) == N * C * (4 if mode == "bilinear" else 16)


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("pad", O.PADDINGS)
def test_a_grid_entirely_outside(mode, pad):
    g = th.Generator().manual_seed(6)
    N, C, H, W, oh, ow = 2, 3, 45, 70, 24, 40
    inp, gout = th.rand(N, C, H, W, generator=g) * 2 - 1, th.rand(N, C, oh, ow, generator=g) * 2 - 1
    grid = 2.5 + th.rand(N, H, W, 2, generator=g)  # [2.5, 3.5]: more than a texture width beyond the border
    args = (inp, grid, gout, oh, ow, mode, pad, False)
    counts = route_counts()
    got = hip(*args, api="capi", counts=counts)
    compare(got, *args, f"outside {mode} {pad}")
    if pad == "zeros":  # nothing lands: no route at all, the output is the zero fill
        assert counts.tolist() == [0, 0] and int((got[0] != 0).sum()) == 0 and int((got[1] != 0).sum()) == 0 and int((got[2] != 0).sum()) == 0
    else:
        assert counts.tolist() == [tiles(N, H, W), 0], counts.tolist()
    if pad == "border":  # everything on the last texel, the grid gradient clipped away
        total, A = inp.double().sum((2, 3)), inp.double().abs().sum((2, 3))
        assert bool(((got[0][:, :, -1, -1].double() - total).abs() <= ULPS["A+S"]["out"] * 2.0 ** -24 * A).all())
        assert int((got[0][:, :, :-1, :-1] != 0).sum()) == 0
        assert int((got[2] != 0).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# bicubic under border / reflection outside [0, size - 1]: the reference kernel's rule, not grid_sample's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["border", "reflection"])
@pytest.mark.parametrize("al", [False, True])
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_bicubic_outside_the_range_follows_the_reference_kernels_centre_rule(pad, al, dtype):
    for C, (oh, ow) in ((2, (30, 45)), (3, (61, 83))):
        args = O.make_case(77 + C, 2, C, 37, 53, oh, ow, dtype=dtype, kind="uniform", extent=1.7) + (oh, ow, "bicubic", pad, al)
        if not (pad == "reflection" and al):  # (there the two rules happen to agree everywhere)
            assert not O.rules_coincide(args[1], oh, ow, "bicubic", pad, al)
        compare(hip(*args), *args, f"bicubic {pad} align_corners={al} {dtype} beyond the border")
        compare(hip(*args, api="capi"), *args, f"bicubic {pad} align_corners={al} {dtype} beyond the border (C ABI)")


@pytest.mark.parametrize("pad", ["border", "reflection"])
def test_bicubic_hand_derived_answers_at_the_border(pad):
    """align_corners=False, unnormalised x = -0.5 (grid x = -1): the centre is clipped (border) or reflected and clipped
    (reflection) to 0 BEFORE floor and fraction, so t = 0, the cubic weights are (0, 1, 0, 0) and the whole value lands
    on texel 0; grid_sample's rule (floor(-0.5) = -1, t = 0.5) would spread it.  y: unnormalised 5 exactly -> row 5."""
    import drtk_amd

    oh, ow = 16, 12
    inp = th.tensor([[[[2.0, -3.0]], [[0.5, 7.0]]]], device=DEV)  # [1,2,1,2]
    grid = th.tensor([[[[-1.0, 11.0 / oh - 1.0], [-1.0, 11.0 / oh - 1.0]]]], device=DEV)
    out = drtk_amd.grid_scatter(inp, grid, oh, ow, "bicubic", pad, False).cpu()
    want = th.zeros(1, 2, oh, ow)
    want[0, :, 5, 0] = th.tensor([-1.0, 7.5])
    assert th.equal(out, want), out.nonzero()
    # ... and the restatement says the same
    assert th.equal(O.restate(inp.cpu().double(), grid.cpu().double(), oh, ow, "bicubic", pad, False).float(), want)
    # x beyond the far border: unnormalised W - 0.5 (grid x = +1) -> texel W - 1
    grid[..., 0] = 1.0
    out = drtk_amd.grid_scatter(inp, grid, oh, ow, "bicubic", pad, False).cpu()
    want = th.zeros(1, 2, oh, ow)
    want[0, :, 5, ow - 1] = th.tensor([-1.0, 7.5])
    assert th.equal(out, want), out.nonzero()


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_channel_first_uv_image_is_read_in_place_and_noncontiguous_input(mode, dtype):
    import drtk_amd

    args = O.make_case(41, 2, 3, 50, 61, 48, 64, dtype=dtype, kind="warp", extent=0.95) + (48, 64, mode, "border", False)
    for api in ("capi", "python"):
        plain = hip(*args, api=api)
        image = hip(*args, api=api, as_uv_image=True)
        compare(image, *args, f"{mode} channel-first uv image ({api})")
        compare(plain, *args, f"{mode} contiguous grid ({api})")
        assert th.equal(plain[1], image[1]) and th.equal(plain[2], image[2]), "the backward is a gather: the same bits through either layout"
    # the operator does not copy the permuted image: what it hands to the C ABI is the tensor itself (capi._grid_layout rule)
    from drtk_amd import capi

    g = args[1].to(DEV).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    passed, layout = capi._grid_layout(g)
    assert passed.data_ptr() == g.data_ptr() and list(layout) == [2 * 50 * 61, 1, 50 * 61]
    # non-contiguous input: channels-last memory, and a strided slice of a wider image
    inp = args[0].to(DEV)
    x1 = inp.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wide = th.zeros(2, 3, 50, 122, dtype=dtype, device=DEV)
    wide[..., ::2] = inp
    x2 = wide[..., ::2]
    assert not x1.is_contiguous() and not x2.is_contiguous()
    for x in (x1, x2):
        x = x.requires_grad_(True)
        gr = args[1].to(DEV).requires_grad_(True)
        out = drtk_amd.grid_scatter(x, gr, 48, 64, mode, "border", False)
        out.backward(args[2].to(DEV))
        compare((out.detach().cpu(), x.grad.cpu(), gr.grad.cpu()), *args, f"{mode} non-contiguous input")


def test_half_precision_under_autocast_is_cast_to_float32_and_empty_batches_give_zeros():
    import drtk_amd

    inp, grid, gout = O.make_case(43, 1, 2, 20, 30, 16, 24)
    with th.autocast("cuda", dtype=th.float16):
        out = drtk_amd.grid_scatter(inp.to(DEV).half(), grid.to(DEV).half(), 16, 24)
    assert out.dtype == th.float32
    want = drtk_amd.grid_scatter(inp.to(DEV).half().float(), grid.to(DEV).half().float(), 16, 24)
    assert float((out - want).abs().max()) <= 1e-5 * float(want.abs().max())
    for shape in ((0, 3, 8, 8), (2, 3, 0, 8), (2, 0, 8, 8)):
        x = th.zeros(shape, device=DEV)
        g = th.zeros(shape[0], shape[2], shape[3], 2, device=DEV)
        out = drtk_amd.grid_scatter(x, g, 5, 7)
        assert out.shape == (shape[0], shape[1], 5, 7) and int((out != 0).sum()) == 0
    with pytest.raises(RuntimeError, match="positive"):
        drtk_amd.grid_scatter(th.zeros(1, 1, 4, 4, device=DEV), th.zeros(1, 4, 4, 2, device=DEV), 0, 7)
    with pytest.raises(RuntimeError, match="batch size, height and width"):
        drtk_amd.grid_scatter(th.zeros(1, 1, 4, 4, device=DEV), th.zeros(1, 4, 5, 2, device=DEV), 4, 4)


def test_more_views_than_one_launch_takes():
    """the view is blockIdx.y (65 535 at most): a larger batch runs as consecutive slices inside the entry points"""
    N = 65535 + 70
    for mode in O.MODES:
        args = O.make_case(61, N, 2, 3, 5, 4, 6, kind="uniform", extent=1.1) + (4, 6, mode, "zeros", False)
        counts = route_counts()
        compare(hip(*args, api="capi", counts=counts), *args, f"{N} views {mode}")
        assert counts[1].item() == 0 and 0.9 * N < counts[0].item() <= N
        compare(hip(*args), *args, f"{N} views {mode} (operator)")


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline: rasterize -> render -> interpolate(uv) -> grid_scatter into the atlas
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", O.MODES)
def test_pipeline_projects_camera_views_into_the_atlas_of_the_spheres_scene(mode):
    import drtk_amd
    from drtk_amd import synthetic as S

    N, H, W, nl, no, T = 3, 192, 256, 24, 28, 128
    v_pix, vi = S.sphere_views(N, nl, no, H, W, device=DEV)
    vt, vti = S.uv_sphere_atlas(nl, no, device=DEV)
    index_img = drtk_amd.rasterize(v_pix, vi, H, W)
    _, bary_img = drtk_amd.render(v_pix, vi, index_img)
    uv_img = drtk_amd.interpolate(vt[None].expand(N, -1, -1).contiguous(), vti, index_img, bary_img)  # [N,2,H,W]
    mask = (index_img != -1)[:, None]
    assert 0.2 < float(mask.float().mean()) < 0.9
    g = th.Generator().manual_seed(9)
    colour = th.where(mask, th.rand(N, 3, H, W, generator=g).to(DEV), 0.0)  # the background is masked by a zero input

    def atlas(background):
        grid = th.where(mask, uv_img * 2 - 1, background).permute(0, 2, 3, 1)  # the channel-first image, in place
        assert not grid.is_contiguous()
        return drtk_amd.grid_scatter(colour, grid, T, T, mode, "border", False), grid

    a_nan, _ = atlas(float("nan"))
    a_far, grid = atlas(5.0)
    assert bool(th.isfinite(a_nan).all())
    assert float(a_far.abs().sum()) > 0.5 * float(colour.sum())
    gout = th.zeros(N, 3, T, T)
    args = (colour.cpu(), grid.cpu().contiguous(), gout, T, T, mode, "border", False)
    compare((a_far.cpu(), None, None), *args, f"atlas {mode}, background at 5.0")
    compare((a_nan.cpu(), None, None), *args, f"atlas {mode}, background at NaN")


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay_matches_eager():
    import drtk_amd
    from drtk_amd import capi

    cases = [O.make_case(51, 2, 4, 120, 130, 128, 128, kind="warp", extent=0.97), O.make_case(52, 2, 4, 120, 130, 128, 128, kind="uniform")]
    x, g, go = (t.to(DEV).clone() for t in cases[0])

    def step():
        a = drtk_amd.grid_scatter(x, g, 128, 128, "bilinear", "border", False)  # windowed / direct by the data of the replay
        b = capi.grid_scatter_2d(x, g, 128, 128, 0, 2, True)
        gi, gg = capi.grid_scatter_2d_backward(go, x, g, 0, 2, True)
        return dict(a=a, b=b, gi=gi, gg=gg)

    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(2):
            step()
    th.cuda.current_stream().wait_stream(side)
    th.cuda.synchronize()
    graph = th.cuda.CUDAGraph()
    with th.cuda.graph(graph):
        out = step()
    for k, case in enumerate(cases + cases[:1]):
        for dst, src in zip((x, g, go), case):
            dst.copy_(src)
        graph.replay()
        th.cuda.synchronize()
        got = {n: t.detach().cpu().clone() for n, t in out.items()}
        compare((got["a"], None, None), *case, 128, 128, "bilinear", "border", False, f"replay {k}: operator")
        compare((got["b"], got["gi"], got["gg"]), *case, 128, 128, "bicubic", "zeros", True, f"replay {k}: C ABI")


def test_zz_report_what_the_float32_oracle_itself_uses_of_the_elementwise_allowances():
    for kind in ULPS:
        print(f"float32 CPU oracle, largest |oracle_f32 - f64| / (u {kind}) seen in this run:", {k: float(f"{v:.3g}") for k, v in OWN[kind].items()},
              "allowed:", {k: float(f"{v:.3g}") for k, v in ULPS[kind].items()})
