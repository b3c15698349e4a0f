"""GPU (-m gpu): `composite_layers` -- fused front-to-back compositing of K layers -- through the C ABI, the torch operator
and the Python API.

The oracle is the definition, the loop `img += (T * a) * color; T *= 1 - a` written below: run in the op's dtype on the
device for the forward (bit for bit: the library is compiled without FMA contraction), in float64 on the CPU for the
gradients.  The gradient bounds are a-priori rounding bounds (roundings per term and per sum), with u = 2^-24 (2^-53 for
float64), M = max(|color|, |background|) and |g| <= G = 3:
    img (2K+4) u M;  T (K+1) u;  grad_color (K+3) u G;  grad_background (K+2) u G;  grad_alpha (2K+C+6) u (C M G + G)."""
import functools

import pytest
import torch as th

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 3.0
KS, CS = (1, 2, 3, 5, 8), (1, 3, 4, 7, 16)


def loop(color, alpha, index=None, background=None):
    """The definition.  color [N,K,C,H,W], alpha [N,K,H,W]."""
    N, K, C, H, W = color.shape
    img, T = color.new_zeros(N, C, H, W), color.new_ones(N, 1, H, W)
    for k in range(K):
        a = alpha[:, k:k + 1]
        if index is not None:
            a = a * (index[:, k:k + 1] != -1)
        img = img + (T * a) * color[:, k]
        T = T * (1 - a)
    if background is not None:
        img = img + T * background
    return img, T


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(K, C, dtype, holes=False, N=2, H=37, W=29):
    """Inputs on the CPU in `dtype` (never modified), and the float64 oracle: outputs and gradients of
    (img * g_img).sum() + (T * g_T).sum()."""
    g = th.Generator().manual_seed(1000 * K + 10 * C + int(holes))
    p = Problem()
    p.color = (th.rand(N, K, C, H, W, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    alpha = th.rand(N, K, H, W, generator=g, dtype=th.float64)
    r = th.rand(N, K, H, W, generator=g)
    alpha[r < 0.15], alpha[r > 0.85] = 0.0, 1.0
    p.alpha = alpha.to(dtype)
    p.bg = (th.rand(N, C, H, W, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    count = th.randint(0, K + 1, (N, 1, H, W), generator=g)  # valid layers per pixel, -1 entries trailing
    tri = th.randint(0, 1000, (N, K, H, W), generator=g)
    index = th.where(th.arange(K)[None, :, None, None] < count, tri, -1)
    if holes:  # a -1 between valid layers
        index = th.where(th.rand(N, K, H, W, generator=g) < 0.25, -1, index)
    p.index = index.int()
    p.g_img = ((th.rand(N, C, H, W, generator=g, dtype=th.float64) * 2 - 1) * G).to(dtype)
    p.g_T = ((th.rand(N, 1, H, W, generator=g, dtype=th.float64) * 2 - 1) * G).to(dtype)
    c64, a64, b64 = f64(p.color), f64(p.alpha), f64(p.bg)
    img, T = loop(c64, a64, p.index, b64)
    ((img * p.g_img.double()).sum() + (T * p.g_T.double()).sum()).backward()
    p.img, p.T, p.gc, p.ga, p.gb = img.detach(), T.detach(), c64.grad, a64.grad, b64.grad
    p.M = max(float(p.color.abs().max()), float(p.bg.abs().max()))
    return p


def bounds(K, C, dtype, M):
    u = 2.0 ** -24 if dtype == th.float32 else 2.0 ** -53
    return dict(img=(2 * K + 4) * u * M, T=(K + 1) * u, gc=(K + 3) * u * G, gb=(K + 2) * u * G, ga=(2 * K + C + 6) * u * (C * M * G + G))


def f64(t):
    """a float64 leaf of its own (`.double()` of a float64 tensor is the tensor itself)"""
    return t.to(th.float64, copy=True).requires_grad_(True)


def dev(*ts):
    return [t.to(DEV) for t in ts]


def run_autograd(fn, color, alpha, index, bg, g_img, g_T):
    """(img, T, grad_color, grad_alpha, grad_background) of a route that goes through autograd.  The leaves share the
    memory of the arguments (placement and strides are part of what is tested); nothing is modified in place."""
    color, alpha, bg = (t.detach().requires_grad_(True) for t in (color, alpha, bg))
    img, T = fn(color, alpha, index, bg)
    ((img * g_img).sum() + (T * g_T).sum()).backward()
    return img.detach(), T.detach(), color.grad, alpha.grad, bg.grad


def run_capi(color, alpha, index, bg, g_img, g_T):
    from drtk_amd import capi

    img, T = capi.composite_layers(color, alpha, index, bg)
    gc, ga, gb = capi.composite_layers_backward(g_img, g_T, color, alpha, index, bg)
    return img, T, gc, ga, gb


def routes():
    import drtk_amd

    return {
        "python": functools.partial(run_autograd, drtk_amd.composite_layers),
        "torch.ops": functools.partial(run_autograd, th.ops.drtk_amd_ext.composite_layers),
        "capi": run_capi,
    }


def check_grid_point(K, C, dtype, holes, H=37, W=29, names=None, use_index=True, use_background=True):
    """problem(K, C, dtype, holes, H=H, W=W) through the routes `names` (all of them by default): the forward bit for bit
    the loop in the same dtype on the device, the five float64 bounds of `bounds`, exact zeros at skipped layers.  Without
    the index or without the background (the guarded driver, tests/guarded_added_ops.py) the float64 oracle is the loop
    without it, under the same bounds."""
    p = problem(K, C, dtype, holes, 2, H, W)
    args = dev(p.color, p.alpha, p.index, p.bg, p.g_img, p.g_T)
    ref = dict(img=p.img, T=p.T, gc=p.gc, ga=p.ga, gb=p.gb)
    if not (use_index and use_background):
        c64, a64, b64 = f64(p.color), f64(p.alpha), (f64(p.bg) if use_background else None)
        ri, rT = loop(c64, a64, p.index if use_index else None, b64)
        ((ri * p.g_img.double()).sum() + (rT * p.g_T.double()).sum()).backward()
        ref = dict(img=ri.detach(), T=rT.detach(), gc=c64.grad, ga=a64.grad, gb=None if b64 is None else b64.grad)
        args[2], args[3] = (args[2] if use_index else None), (args[3] if use_background else None)
    want_img, want_T = loop(*args[:4])  # the loop, same dtype, on the device
    bound = bounds(K, C, dtype, p.M)
    for name, route in routes().items():
        if names is not None and name not in names:
            continue
        img, T, gc, ga, gb = route(*args)
        what = f"K={K} C={C} {H}x{W} {dtype} holes={holes} index={use_index} background={use_background} {name}"
        assert img.dtype == dtype and img.shape == want_img.shape and T.shape == want_T.shape, what
        assert th.equal(img, want_img) and th.equal(T, want_T), f"{what}: forward differs from the loop in the same dtype"
        got = dict(img=img, T=T, gc=gc, ga=ga, gb=gb)
        for key, r in ref.items():
            if r is None:
                assert got[key] is None, (what, key)
                continue
            assert got[key].shape == r.shape, (what, key)
            err = float((got[key].double().cpu() - r).abs().max())
            print(f"{what} {key}: max |d| {err:.3e}, bound {bound[key]:.3e}")
            assert err <= bound[key], f"{what} {key}: {err:.3e} > {bound[key]:.3e}"
        if use_index:
            masked = (p.index == -1).to(DEV)
            assert not bool(ga[masked].any()) and not bool(gc[masked[:, :, None].expand_as(gc)].any()), f"{what}: gradient at a skipped layer"


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("K", KS)
def test_base_grid_forward_bits_and_gradient_bounds(K, C, dtype):
    for holes in (False, True):
        check_grid_point(K, C, dtype, holes)


# H x W whose pixel count leaves every remainder mod 4 -- the tail the P-pixel loads and stores of a lane end in (P = 4, or
# 2 where 4 K P values per lane are too many) --; 37 x 29 is also more than one workgroup at P = 4.
TAIL_SHAPES = ((37, 29), (6, 7), (5, 7), (8, 8))


@pytest.mark.parametrize("holes", [False, True], ids=["trailing", "holes"])
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("H,W", TAIL_SHAPES)
@pytest.mark.parametrize("K", range(1, 9))
def test_every_layer_count_and_every_pixel_tail(K, H, W, dtype, holes):
    """Every K the library instantiates (1 ... 8: K = 4 is the last at which the backward keeps four pixels per lane, 6 and
    7 the only ones whose `present` mask is neither full-width nor small) on every tail of the pixel vectors, C = 3, through
    every route: the checks of test_base_grid_forward_bits_and_gradient_bounds."""
    assert sorted(h * w % 4 for h, w in TAIL_SHAPES) == [0, 1, 2, 3] and 37 * 29 > 4 * 256
    check_grid_point(K, 3, dtype, holes, H, W)


def test_without_index_and_without_background():
    import drtk_amd

    for K, C, dtype in ((1, 3, th.float32), (3, 4, th.float32), (8, 1, th.float64)):
        p = problem(K, C, dtype)
        color, alpha, bg, g_img, g_T = dev(p.color, p.alpha, p.bg, p.g_img, p.g_T)
        for index, background in ((None, None), (None, bg), (p.index.to(DEV), None)):
            want = loop(color, alpha, index, background)
            c64, a64 = f64(p.color), f64(p.alpha)
            b64 = f64(p.bg) if background is not None else None
            ri, rT = loop(c64, a64, None if index is None else p.index, b64)
            ((ri * p.g_img.double()).sum() + (rT * p.g_T.double()).sum()).backward()
            c, a = color.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
            b = background.clone().requires_grad_(True) if background is not None else None
            img, T = drtk_amd.composite_layers(c, a, index, b)
            assert th.equal(img, want[0]) and th.equal(T, want[1])
            ((img * g_img).sum() + (T * g_T).sum()).backward()
            bound = bounds(K, C, dtype, p.M)
            assert float((c.grad.double().cpu() - c64.grad).abs().max()) <= bound["gc"]
            assert float((a.grad.double().cpu() - a64.grad).abs().max()) <= bound["ga"]
            if b is not None:
                assert float((b.grad.double().cpu() - b64.grad).abs().max()) <= bound["gb"]


def test_gradcheck_float64():
    import drtk_amd

    g = th.Generator().manual_seed(3)
    N, K, C, H, W = 1, 3, 2, 3, 3
    color = (th.rand(N, K, C, H, W, generator=g, dtype=th.float64) * 2 - 1).to(DEV).requires_grad_(True)
    alpha = (0.1 + 0.8 * th.rand(N, K, H, W, generator=g, dtype=th.float64)).to(DEV).requires_grad_(True)
    bg = (th.rand(N, C, H, W, generator=g, dtype=th.float64) * 2 - 1).to(DEV).requires_grad_(True)
    index = th.where(th.rand(N, K, H, W, generator=g) < 0.3, -1, 7).int().to(DEV)
    assert bool((index == -1).any()) and bool((index != -1).any())
    assert th.autograd.gradcheck(lambda c, a, b: drtk_amd.composite_layers(c, a, index, b), (color, alpha, bg))
    rgba = th.cat([color.detach(), alpha.detach()[:, :, None]], 2).requires_grad_(True)
    assert th.autograd.gradcheck(lambda x, b: drtk_amd.composite_layers(x, None, index, b), (rgba, bg))


def test_double_backward_raises():
    import drtk_amd

    p = problem(2, 3, th.float64)
    color, alpha = (t.to(DEV).requires_grad_(True) for t in (p.color, p.alpha))
    img, _ = drtk_amd.composite_layers(color, alpha)
    with pytest.raises(RuntimeError, match="double backward"):
        th.autograd.grad(img.sum(), color, create_graph=True)


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_forms_give_identical_bits(dtype):
    """split tensors, one rgba tensor, channel slices of it, a permuted input (planes not contiguous: copied once), a
    view-shared background, [N,K,1,H,W] alpha."""
    import drtk_amd

    K, C = 5, 3
    p = problem(K, C, dtype, True)
    color, alpha, index, bg, g_img, g_T = dev(p.color, p.alpha, p.index, p.bg, p.g_img, p.g_T)
    base = run_autograd(drtk_amd.composite_layers, color, alpha, index, bg, g_img, g_T)

    def same(got, what):
        for a, b, name in zip(got, base, ("img", "T", "grad_color", "grad_alpha", "grad_background")):
            assert a.shape == b.shape and th.equal(a, b), f"{what}: {name} differs"

    rgba0 = th.cat([color, alpha[:, :, None]], 2)
    # rgba
    rgba, b = rgba0.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    img, T = drtk_amd.composite_layers(rgba, index_img=index, background=b)
    ((img * g_img).sum() + (T * g_T).sum()).backward()
    assert rgba.grad.shape == rgba0.shape
    same((img.detach(), T.detach(), rgba.grad[:, :, :-1], rgba.grad[:, :, -1], b.grad), "rgba")
    # channel slices of rgba
    rgba, b = rgba0.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    img, T = drtk_amd.composite_layers(rgba[:, :, :-1], rgba[:, :, -1], index, b)
    ((img * g_img).sum() + (T * g_T).sum()).backward()
    same((img.detach(), T.detach(), rgba.grad[:, :, :-1], rgba.grad[:, :, -1], b.grad), "slices")
    # planes that are not contiguous
    color_t = color.transpose(3, 4).contiguous().transpose(3, 4)
    alpha_t = alpha.transpose(2, 3).contiguous().transpose(2, 3)
    index_t = index.transpose(2, 3).contiguous().transpose(2, 3)
    bg_t = bg.transpose(2, 3).contiguous().transpose(2, 3)
    assert not color_t.is_contiguous() and color_t.stride(-1) != 1
    same(run_autograd(drtk_amd.composite_layers, color_t, alpha_t, index_t, bg_t, g_img.transpose(2, 3).contiguous().transpose(2, 3), g_T), "permuted")
    # [N,K,1,H,W] alpha: the gradient has that shape
    a5 = alpha[:, :, None].clone().requires_grad_(True)
    img, T = drtk_amd.composite_layers(color, a5, index, bg)
    ((img * g_img).sum() + (T * g_T).sum()).backward()
    assert a5.grad.shape == a5.shape and th.equal(a5.grad[:, :, 0], base[3]) and th.equal(img, base[0])
    # one background for all views
    bg1 = bg[:1].clone().requires_grad_(True)
    shared = run_autograd(lambda c, a, i, b: drtk_amd.composite_layers(c, a, i, bg1.expand(bg.shape[0], -1, -1, -1)), color, alpha, index, bg, g_img, g_T)
    full = run_autograd(drtk_amd.composite_layers, color, alpha, index, bg[:1].expand_as(bg).contiguous(), g_img, g_T)
    for a, b in zip(shared[:4], full[:4]):
        assert th.equal(a, b)
    assert th.equal(bg1.grad, full[4].sum(0, keepdim=True))


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_element_alignment_only(dtype):
    """every tensor carved out of a larger buffer at an odd element offset"""
    K, C = 3, 4
    p = problem(K, C, dtype, True)
    args = dev(p.color, p.alpha, p.index, p.bg, p.g_img, p.g_T)

    def carve(t, offset):
        buf = th.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        view = buf[offset:offset + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        return view

    odd = [carve(t, o) for t, o in zip(args, (1, 3, 1, 3, 1, 3))]
    for name, route in routes().items():
        for a, b in zip(route(*odd), route(*args)):
            assert th.equal(a, b), name


def test_nan_at_skipped_layers_does_not_propagate():
    K, C = 5, 3
    p = problem(K, C, th.float32, True)
    color, alpha, index, bg, g_img, g_T = dev(p.color, p.alpha, p.index, p.bg, p.g_img, p.g_T)
    masked = index == -1
    assert bool(masked.any())
    color_nan, alpha_nan = color.clone(), alpha.clone()
    color_nan[masked[:, :, None].expand_as(color)] = float("nan")
    alpha_nan[masked] = float("nan")
    for name, route in routes().items():
        clean = route(color, alpha, index, bg, g_img, g_T)
        dirty = route(color_nan, alpha_nan, index, bg, g_img, g_T)
        for a, b in zip(dirty, clean):
            assert th.equal(a, b), name
        assert not bool(dirty[2][masked[:, :, None].expand_as(color)].any()) and not bool(dirty[3][masked].any()), name


def test_opaque_front_layer():
    """layers behind an opaque one get zero gradient; the opaque layer's own alpha gradient depends on them"""
    import drtk_amd

    K, C = 3, 3
    p = problem(K, C, th.float32)
    alpha = p.alpha.clone()
    alpha[:, 0] = 1.0
    alpha[:, 1:] = alpha[:, 1:].clamp(0.2, 0.8)
    c64, a64 = f64(p.color), f64(alpha)
    img, T = loop(c64, a64)
    ((img * p.g_img.double()).sum() + (T * p.g_T.double()).sum()).backward()
    color, alpha_d, g_img, g_T = dev(p.color, alpha, p.g_img, p.g_T)
    c, a = color.clone().requires_grad_(True), alpha_d.clone().requires_grad_(True)
    img, T = drtk_amd.composite_layers(c, a)
    ((img * g_img).sum() + (T * g_T).sum()).backward()
    assert not bool(T.any()) and th.equal(img, color[:, 0])
    assert not bool(c.grad[:, 1:].any()) and not bool(a.grad[:, 1:].any())
    bound = bounds(K, C, th.float32, p.M)
    assert float((a.grad.double().cpu() - a64.grad).abs().max()) <= bound["ga"]
    assert float((c.grad.double().cpu() - c64.grad).abs().max()) <= bound["gc"]
    # ... and it is not the gradient of a scene without the layers behind
    c2, a2 = color[:, :1].clone().requires_grad_(True), alpha_d[:, :1].clone().requires_grad_(True)
    img2, T2 = drtk_amd.composite_layers(c2, a2)
    ((img2 * g_img).sum() + (T2 * g_T).sum()).backward()
    assert float((a2.grad - a.grad[:, :1]).abs().max()) > 0.1


def test_gradient_subsets():
    import drtk_amd

    K, C = 3, 3
    p = problem(K, C, th.float32, True)
    color, alpha, index, bg, g_img, g_T = dev(p.color, p.alpha, p.index, p.bg, p.g_img, p.g_T)
    full = {}
    for uses in ("img", "T", "both"):
        c, a, b = (t.clone().requires_grad_(True) for t in (color, alpha, bg))
        img, T = drtk_amd.composite_layers(c, a, index, b)
        loss = {"img": lambda: (img * g_img).sum(), "T": lambda: (T * g_T).sum(), "both": lambda: (img * g_img).sum() + (T * g_T).sum()}[uses]()
        loss.backward()
        full[uses] = (c.grad, a.grad, b.grad)
    assert th.equal(full["both"][0], full["img"][0]) and not bool(full["T"][0].any()) and not bool(full["T"][2].any())
    assert float((full["img"][1] + full["T"][1] - full["both"][1]).abs().max()) <= 4 * bounds(K, C, th.float32, p.M)["ga"]
    for uses in ("img", "T", "both"):
        for which in range(3):
            ts = [t.clone() for t in (color, alpha, bg)]
            ts[which].requires_grad_(True)
            img, T = drtk_amd.composite_layers(ts[0], ts[1], index, ts[2])
            loss = {"img": lambda: (img * g_img).sum(), "T": lambda: (T * g_T).sum(), "both": lambda: (img * g_img).sum() + (T * g_T).sum()}[uses]()
            loss.backward()
            for i, t in enumerate(ts):
                if i == which:
                    assert th.equal(t.grad, full[uses][i]), (uses, which)
                else:
                    assert t.grad is None, (uses, which, i)
    # no input requires a gradient: no node
    img, T = drtk_amd.composite_layers(color, alpha, index, bg)
    assert not img.requires_grad and not T.requires_grad


def test_edge_sizes():
    import drtk_amd
    from drtk_amd import capi

    # N = 0
    img, T = drtk_amd.composite_layers(th.zeros(0, 2, 3, 4, 5, device=DEV), th.zeros(0, 2, 4, 5, device=DEV))
    assert img.shape == (0, 3, 4, 5) and T.shape == (0, 1, 4, 5)
    img, T = capi.composite_layers(th.zeros(0, 2, 3, 4, 5, device=DEV), th.zeros(0, 2, 4, 5, device=DEV))
    assert img.shape == (0, 3, 4, 5) and T.shape == (0, 1, 4, 5)
    g = th.Generator().manual_seed(5)
    # H * W = 1, and K = 1 without index or background
    for shape in ((3, 4, 2, 1, 1), (2, 1, 3, 5, 7)):
        N, K, C, H, W = shape
        color, alpha = th.rand(*shape, generator=g).to(DEV), th.rand(N, K, H, W, generator=g).to(DEV)
        g_img, g_T = th.rand(N, C, H, W, generator=g).to(DEV), th.rand(N, 1, H, W, generator=g).to(DEV)
        got = run_autograd(lambda c, a, i, b: drtk_amd.composite_layers(c, a), color, alpha, None, color[:, 0], g_img, g_T)
        want = run_autograd(lambda c, a, i, b: loop(c, a), color, alpha, None, color[:, 0], g_img, g_T)
        assert th.equal(got[0], want[0]) and th.equal(got[1], want[1])
        assert float((got[2] - want[2]).abs().max()) <= 1e-6 and float((got[3] - want[3]).abs().max()) <= 1e-5
    # more views than one launch takes
    N, K, C = 65537, 2, 1
    color, alpha = th.rand(N, K, C, 1, 1, generator=g).to(DEV), th.rand(N, K, 1, 1, generator=g).to(DEV)
    index = th.where(th.rand(N, K, 1, 1, generator=g) < 0.3, -1, 1).int().to(DEV)
    bg, g_img, g_T = th.rand(N, C, 1, 1, generator=g).to(DEV), th.rand(N, C, 1, 1, generator=g).to(DEV), th.rand(N, 1, 1, 1, generator=g).to(DEV)
    got = run_autograd(drtk_amd.composite_layers, color, alpha, index, bg, g_img, g_T)
    want = run_autograd(loop, color, alpha, index, bg, g_img, g_T)
    assert th.equal(got[0], want[0]) and th.equal(got[1], want[1])
    for a, b in zip(got[2:], want[2:]):
        assert float((a - b).abs().max()) <= 1e-5


def test_autocast_casts_half_to_float():
    import drtk_amd

    p = problem(3, 3, th.float32, True)
    color, alpha, index, bg = dev(p.color.half(), p.alpha.half(), p.index, p.bg.half())
    with th.autocast("cuda", dtype=th.float16):
        img, T = drtk_amd.composite_layers(color, alpha, index, bg)
    want = drtk_amd.composite_layers(color.float(), alpha.float(), index, bg.float())
    assert img.dtype == th.float32 and T.dtype == th.float32
    assert th.equal(img, want[0]) and th.equal(T, want[1])


def test_reproducible_and_every_output_element_written():
    import os

    from drtk_amd import capi

    assert os.environ.get("DRTK_CAPI_POISON") == "1" and capi._POISON  # outputs start as NaN: conftest.py
    for K, C, dtype in ((8, 7, th.float32), (5, 4, th.float64)):
        p = problem(K, C, dtype, True)
        args = dev(p.color, p.alpha, p.index, p.bg, p.g_img, p.g_T)
        first, second = run_capi(*args), run_capi(*args)
        for a, b in zip(first, second):
            assert not bool(th.isnan(a).any()) and th.equal(a, b)
        # rgba: one gradient tensor through two pointer sets, all of it written
        rgba = th.cat([args[0], args[1][:, :, None]], 2)
        gc, ga, gb = capi.composite_layers_backward(args[4], args[5], rgba, None, args[2], args[3])
        assert ga is None and not bool(th.isnan(gc).any())
        assert th.equal(gc[:, :, :-1], first[2]) and th.equal(gc[:, :, -1], first[3]) and th.equal(gb, first[4])
        # absent upstream gradients are zeros
        gc0, ga0, gb0 = capi.composite_layers_backward(None, None, *args[:4])
        assert not bool(gc0.any()) and not bool(ga0.any()) and not bool(gb0.any())


def test_graph_capture_of_forward_and_backward():
    import drtk_amd

    K, C = 3, 3
    p, q = problem(K, C, th.float32, True), problem(K, C, th.float32, False)
    color, alpha, bg = (t.to(DEV).requires_grad_(True) for t in (p.color, p.alpha, p.bg))
    index, g_img, g_T = dev(p.index.clone(), p.g_img, p.g_T)
    out = {}

    def step():
        out["img"], out["T"] = drtk_amd.composite_layers(color, alpha, index, bg)
        loss = (out["img"] * g_img).sum() + (out["T"] * g_T).sum()
        loss.backward()
        return loss

    captured = drtk_amd.capture_step(step, [color, alpha, bg])
    with th.no_grad():
        color.copy_(q.color), alpha.copy_(q.alpha), bg.copy_(q.bg), index.copy_(q.index)
    captured()
    th.cuda.synchronize()
    want = run_autograd(drtk_amd.composite_layers, *dev(q.color, q.alpha, q.index, q.bg, p.g_img, p.g_T))
    got = (out["img"], out["T"], color.grad, alpha.grad, bg.grad)
    for a, b in zip(got, want):
        assert th.equal(a, b)


def test_end_to_end_two_sheets():
    """rasterize_layers -> render -> interpolate -> composite_layers on the two-sheet scene of
    tests/test_gpu_rasterize_layers.py (96 x 128, K = 2): the loop's image bit for bit, its attribute gradients within
    that test's bar."""
    import drtk_amd

    H, W, C, K = 96, 128, 3, 2

    def sheet(x0, x1, y0, y1, z, nx, ny, tilt):
        x = th.linspace(x0, x1, nx + 1, dtype=th.float64)
        y = th.linspace(y0, y1, ny + 1, dtype=th.float64)
        yy, xx = th.meshgrid(y, x, indexing="ij")
        zz = z + tilt * (xx / W + 0.5 * yy / H)
        v = th.stack([xx, yy, zz], -1).reshape(1, -1, 3).float()
        j, i = th.meshgrid(th.arange(ny), th.arange(nx), indexing="ij")
        a = (j * (nx + 1) + i).reshape(-1)
        vi = th.cat([th.stack([a, a + nx + 1, a + nx + 2], -1), th.stack([a, a + nx + 2, a + 1], -1)]).int()
        return v.to(DEV), vi.to(DEV)

    vA, viA = sheet(3.3, 90.7, 5.2, 80.1, 2.0, 9, 7, 0.4)       # front, translucent (per-vertex alpha)
    vB, viB = sheet(40.6, 124.2, 20.4, 93.3, 4.0, 6, 8, -0.3)   # back
    VA, VB = vA.shape[1], vB.shape[1]
    g = th.Generator().manual_seed(11)
    attr0 = th.cat([
        th.cat([th.rand(1, VA, C, generator=g), 0.2 + 0.6 * th.rand(1, VA, 1, generator=g)], -1),
        th.cat([th.rand(1, VB, C, generator=g), 0.7 + 0.3 * th.rand(1, VB, 1, generator=g)], -1)], 1).to(DEV)
    weight = (th.rand(1, C, H, W, generator=g) * 2 - 1).to(DEV)
    bg = th.rand(1, C, H, W, generator=g).to(DEV)
    v, vi = th.cat([vA, vB], 1), th.cat([viA, viB + VA])
    index = drtk_amd.rasterize_layers(v, vi, H, W, K)
    assert int((index[:, 1] != -1).sum()) > 500 and int((index[:, 0] == -1).sum()) > 500
    folded = index.flatten(0, 1)
    _, bary = drtk_amd.render(v.repeat_interleave(K, 0), vi, folded)

    def rgba_of(attr):
        return drtk_amd.interpolate(attr.repeat_interleave(K, 0), vi, folded, bary).unflatten(0, (1, K))

    attr = attr0.clone().requires_grad_(True)
    img, T = drtk_amd.composite_layers(rgba_of(attr), index_img=index, background=bg)
    (img * weight).sum().backward()

    ref = attr0.clone().requires_grad_(True)
    rgba = rgba_of(ref) * (index != -1)[:, :, None]
    want_img, want_T = loop(rgba[:, :, :C], rgba[:, :, C], index, bg)
    (want_img * weight).sum().backward()
    assert th.equal(img, want_img) and th.equal(T, want_T)
    err, tol = float((attr.grad.double() - ref.grad.double()).abs().max()), 1e-5 + 1e-5 * float(ref.grad.abs().max())
    print(f"attribute gradient: max |d| {err:.3e}, bar {tol:.3e}")
    assert float(ref.grad.abs().max()) > 0 and err <= tol
