"""GPU (-m gpu): `mipmap_pyramid` through `drtk_amd.mipmap_pyramid` (with autograd) and through the C ABI binding, bit for
bit against its definition and against the backward recurrence, both written with elementwise torch operations on the
device; layout, strides, NaN containment, the `avg_pool2d` loop, graph capture, the textured pipeline and gradcheck."""
import functools

import pytest
import torch as th
import torch.nn.functional as thf
from conftest import mipmap_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def next_level(x):
    h, w = x.shape[-2] // 2, x.shape[-1] // 2
    a, b = x[..., 0:2 * h:2, 0:2 * w:2], x[..., 0:2 * h:2, 1:2 * w:2]
    c, d = x[..., 1:2 * h:2, 0:2 * w:2], x[..., 1:2 * h:2, 1:2 * w:2]
    return (((a + b) + c) + d) * 0.25


def max_levels(H, W):
    return min(11, min(H, W).bit_length())


def definition(x, levels):
    out = [x]
    for _ in range(levels - 1):
        out.append(next_level(out[-1]))
    return out


def recurrence(grads, like):
    """G_{L-1} = g_{L-1}; G_l = g_l + 0.25 * up(G_{l+1}); a texel of a dropped row / column keeps g_l alone.  An absent g_l
    (None) is zero."""
    G = None
    for l in range(len(grads) - 1, -1, -1):
        h, w = like.shape[-2] >> l, like.shape[-1] >> l
        g = grads[l].clone() if grads[l] is not None else like.new_zeros(*like.shape[:-2], h, w)
        if G is not None:
            up = G.repeat_interleave(2, -2).repeat_interleave(2, -1) * 0.25
            g[..., :up.shape[-2], :up.shape[-1]] = g[..., :up.shape[-2], :up.shape[-1]] + up
        G = g
    return G


SHAPES = [
    (1, 1, 2, 2),        # 2 levels
    (1, 1, 64, 64),      # exactly one tile, 7 levels, one launch
    (1, 2, 128, 128),    # 8 levels, the second launch fed by a 2 x 2 level
    (1, 1, 65, 63),      # partial tiles, odd on both axes
    (2, 3, 70, 130),     # 7 levels, odd drops inside a tile at levels 1 -> 2 and 2 -> 3
    (1, 1, 36, 4100),    # many tiles in a row with a partial last one, 6 levels
    (1, 1, 1024, 1024),  # all 11 levels, the second launch making 8, 4, 2 and 1
    (1, 1, 1100, 1030),  # 11 levels with odd drops deep in the chain
]
CASES = [(s, None) for s in SHAPES] + [((1, 2, 128, 128), L) for L in (1, 2, 7)]
DTYPES = [th.float32, th.float64]


@functools.lru_cache(maxsize=None)
def problem(shape, levels, dtype):
    """(x, the levels by the definition, a gradient per level, grad_input by the recurrence), on the device; shared between
    the tests and never modified."""
    L = levels or max_levels(*shape[2:])
    gen = th.Generator().manual_seed(sum(shape) + 131 * L)
    x = (th.rand(shape, generator=gen, dtype=th.float64) * 2 - 1).to(dtype).to(DEV)
    want = definition(x, L)
    grads = [(th.rand(t.shape, generator=gen, dtype=th.float64) * 6 - 3).to(dtype).to(DEV) for t in want]
    return x, want, grads, recurrence(grads, x)


def run_autograd(x, levels, grads):
    """(levels, x.grad) of drtk_amd.mipmap_pyramid; `grads[l] is None`: level l takes no part in the loss."""
    import drtk_amd

    leaf = x.clone().requires_grad_(True)
    out = drtk_amd.mipmap_pyramid(leaf, levels)
    assert out[0].data_ptr() == leaf.data_ptr()
    loss = sum((t * g).sum() for t, g in zip(out, grads) if g is not None)
    loss.backward()
    return out, leaf.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape,levels", CASES, ids=[f"{'x'.join(map(str, s))}-{L or 'all'}" for s, L in CASES])
def test_forward_and_backward_bit_for_bit(shape, levels, dtype):
    from drtk_amd import capi

    x, want, grads, want_grad = problem(shape, levels, dtype)
    out, grad = run_autograd(x, levels, grads)
    assert len(out) == len(want)
    for l, (a, b) in enumerate(zip(out, want)):
        assert a.shape == b.shape and th.equal(a, b), f"level {l}"
    assert th.equal(grad, want_grad)
    out = capi.mipmap_pyramid(x, len(want))
    assert out[0] is x
    for l, (a, b) in enumerate(zip(out, want)):
        assert a.shape == b.shape and th.equal(a, b), f"C ABI, level {l}"
    assert th.equal(capi.mipmap_pyramid_backward(grads), want_grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["only_g0", "only_coarsest", "every_second"])
def test_backward_with_absent_gradients(which, dtype):
    from drtk_amd import capi

    for shape in ((2, 3, 70, 130), (1, 2, 128, 128)):
        x, want, grads, _ = problem(shape, None, dtype)
        L = len(want)
        keep = {"only_g0": [0], "only_coarsest": [L - 1], "every_second": list(range(1, L, 2))}[which]
        some = [g if l in keep else None for l, g in enumerate(grads)]
        want_grad = recurrence(some, x)
        _, grad = run_autograd(x, None, some)
        assert th.equal(grad, want_grad)
        assert th.equal(capi.mipmap_pyramid_backward(some, grad_input=th.full_like(x, float("nan"))), want_grad)


def test_layout():
    """Element 0 is the input's memory; levels 1 and up lie back to back in ONE storage at multiples of 16 bytes."""
    import drtk_amd

    for dtype in DTYPES:
        x, want, _, _ = problem((2, 3, 70, 130), None, dtype)  # levels of 13650, 3264, 816 ... elements: offsets get rounded
        out = drtk_amd.mipmap_pyramid(x)
        assert out[0].data_ptr() == x.data_ptr() and len(out) == 7
        base = out[1].untyped_storage().data_ptr()
        assert base != x.untyped_storage().data_ptr()
        at = 0
        for t in out[1:]:
            assert t.is_contiguous() and t.untyped_storage().data_ptr() == base
            assert t.data_ptr() - base == at and at % 16 == 0
            at = (at + t.numel() * t.element_size() + 15) // 16 * 16
        assert out[1].untyped_storage().nbytes() == at
    assert drtk_amd.mipmap_pyramid(x, 1)[0].data_ptr() == x.data_ptr()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_nothing_is_written_outside_the_levels(dtype):
    """Through the C ABI, every level and grad_input carved out of one sentinel-filled buffer with gaps of 3 elements (so they
    are merely element-aligned): the gaps are untouched and no sentinel is left inside."""
    from drtk_amd import capi

    sentinel = -7.25
    for shape in ((2, 3, 70, 130), (1, 1, 65, 63), (1, 2, 128, 128)):
        x, want, grads, want_grad = problem(shape, None, dtype)
        targets = want[1:] + [want_grad]
        flat = th.full((sum(t.numel() + 3 for t in targets) + 3,), sentinel, dtype=dtype, device=DEV)
        views, gaps, at = [], [], 0
        for t in targets:
            gaps.append(flat[at:at + 3])
            views.append(flat[at + 3:at + 3 + t.numel()].view(t.shape))
            at += 3 + t.numel()
        gaps.append(flat[at:])
        capi.mipmap_pyramid(x, len(want), out=[None] + views[:-1])
        capi.mipmap_pyramid_backward(grads, grad_input=views[-1])
        for a, b in zip(views, targets):
            assert th.equal(a, b) and not bool((a == sentinel).any())
        for g in gaps:
            assert g.numel() == 3 and bool((g == sentinel).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_strides_and_alignment(dtype):
    import drtk_amd
    from drtk_amd import capi

    shape = (2, 3, 70, 130)
    x, want, grads, want_grad = problem(shape, None, dtype)
    # a base pointer offset by one element, for the input, the gradients and grad_input
    def shifted(t):
        buf = th.empty(t.numel() + 1, dtype=dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v

    xs = shifted(x)
    assert xs.data_ptr() % 16 == x.element_size()
    for a, b in zip(capi.mipmap_pyramid(xs, len(want)), want):
        assert th.equal(a, b)
    got = capi.mipmap_pyramid_backward([shifted(g) for g in grads], grad_input=shifted(th.full_like(x, float("nan"))))
    assert th.equal(got, want_grad)
    out, grad = run_autograd(xs, None, grads)
    assert all(th.equal(a, b) for a, b in zip(out, want)) and th.equal(grad, want_grad)
    # a channel slice is read in place
    wide = th.full((2, 6, 70, 130), float("nan"), dtype=dtype, device=DEV)
    wide[:, ::2] = x
    leaf = wide.clone().requires_grad_(True)
    sl = leaf[:, ::2]
    out = drtk_amd.mipmap_pyramid(sl)
    assert out[0].data_ptr() == sl.data_ptr() and not sl.is_contiguous()
    assert all(th.equal(a, b) for a, b in zip(out, want))
    sum((t * g).sum() for t, g in zip(out, grads)).backward()
    assert th.equal(leaf.grad[:, ::2], want_grad) and not bool(leaf.grad[:, 1::2].any())
    assert all(th.equal(a, b) for a, b in zip(capi.mipmap_pyramid(wide[:, ::2], len(want)), want))
    # planes that are not contiguous are copied once by the operator
    tr = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert all(th.equal(a, b) for a, b in zip(drtk_amd.mipmap_pyramid(tr), want))
    # one texture for N = 3 views: reduced once, returned expanded, the gradient is the sum over the views
    gen = th.Generator().manual_seed(5)
    leaf = x[:1].clone().requires_grad_(True)
    out = drtk_amd.mipmap_pyramid(leaf.expand(3, -1, -1, -1))
    assert out[0].data_ptr() == leaf.data_ptr()
    want1 = definition(x[:1], len(want))
    for a, b in zip(out, want1):
        assert a.shape[0] == 3 and a.stride(0) == 0 and th.equal(a, b.expand(3, -1, -1, -1))
    gv = [th.randint(-2, 3, t.shape, generator=gen).to(dtype).to(DEV) for t in out]  # small integers: every sum is exact
    sum((t * g).sum() for t, g in zip(out, gv)).backward()
    assert th.equal(leaf.grad, recurrence([g.sum(0, keepdim=True) for g in gv], x[:1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_nan_containment(dtype):
    import drtk_amd
    from drtk_amd import capi

    x, want, grads, _ = problem((2, 3, 70, 130), None, dtype)
    bad = x.clone()
    bad[1, 2, 5, 9] = float("nan")
    for out in (drtk_amd.mipmap_pyramid(bad), capi.mipmap_pyramid(bad, len(want))):
        for k, t in enumerate(out):
            expect = th.zeros_like(t, dtype=th.bool)
            expect[1, 2, 5 >> k, 9 >> k] = True
            assert th.equal(t.isnan(), expect), f"level {k}"
            assert th.equal(t[~expect], want[k][~expect])
    gbad = [g.clone() for g in grads]
    gbad[2][0, 1, 3, 7] = float("nan")
    expect = th.zeros_like(x, dtype=th.bool)
    expect[0, 1, 12:16, 28:32] = True
    _, grad = run_autograd(x, None, gbad)
    for got in (grad, capi.mipmap_pyramid_backward(gbad)):
        assert th.equal(got.isnan(), expect)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(2, 3, 70, 130), (1, 1, 1100, 1030)], ids=["70x130", "1100x1030"])
def test_against_the_avg_pool2d_loop_on_the_device(shape, dtype):
    """Positive inputs and gradients.  The levels are within 4 eps (relative, per texel) of the avg_pool2d chain -- three adds
    and a division that may or may not round as the multiply by 0.25 does --, grad_input within 2 * levels * eps of autograd
    of the chain.  Whether the two are bitwise equal is reported, not asserted."""
    import drtk_amd

    eps = th.finfo(dtype).eps
    gen = th.Generator().manual_seed(11)
    x = th.rand(shape, generator=gen, dtype=th.float64).to(dtype).to(DEV)
    L = max_levels(*shape[2:])
    leaf = x.clone().requires_grad_(True)
    chain = [leaf]
    for _ in range(L - 1):
        chain.append(thf.avg_pool2d(chain[-1], 2))
    grads = [th.rand(t.shape, generator=gen, dtype=th.float64).to(dtype).to(DEV) for t in chain]
    sum((t * g).sum() for t, g in zip(chain, grads)).backward()
    out, grad = run_autograd(x, None, grads)
    fwd_err = max(float(((a.detach() - b.detach()).abs() / b.detach().abs()).max()) for a, b in zip(out, chain))
    bwd_err = float(((grad - leaf.grad).abs() / leaf.grad.abs()).max())
    bitwise = all(th.equal(a.detach(), b.detach()) for a, b in zip(out, chain)), th.equal(grad, leaf.grad)
    print(f"mipmap_pyramid vs avg_pool2d loop {shape} {dtype}: forward rel err {fwd_err / eps:.2f} eps (bitwise equal: {bitwise[0]}), "
          f"backward rel err {bwd_err / eps:.2f} eps (bitwise equal: {bitwise[1]})")
    assert fwd_err <= 4 * eps
    assert bwd_err <= 2 * L * eps


def test_graph_capture_of_forward_and_backward():
    import drtk_amd

    shape = (2, 3, 70, 130)
    p = problem(shape, None, th.float32)
    x = p[0].clone().requires_grad_(True)
    grads = p[2]
    out = {}

    def step():
        out["levels"] = drtk_amd.mipmap_pyramid(x)
        loss = sum((t * g).sum() for t, g in zip(out["levels"], grads))
        loss.backward()
        return loss

    captured = drtk_amd.capture_step(step, [x])
    new = p[0].flip(-1) * 0.75 + 0.125  # other data for the replay
    with th.no_grad():
        x.copy_(new)
    captured()
    th.cuda.synchronize()
    want, want_grad = run_autograd(new, None, grads)
    for a, b in zip(out["levels"], want):
        assert th.equal(a, b)
    assert th.equal(x.grad, want_grad)


def test_end_to_end_with_the_sampler():
    """mipmap_grid_sample(mipmap_pyramid(tex), ...) on a 64 x 64 output of a 128 x 128 texture with C = 3: the image of the
    avg_pool2d-loop pipeline bit for bit; tex.grad within the sampler's own bar (tests/test_gpu_mipmap.py `close`:
    1e-5 + 1e-5 max|ref|, its float-atomic reordering) plus 2 * levels * eps of max|ref| for the fold."""
    import drtk_amd

    tex, grid, jac, gout = mipmap_inputs(77, 2, 3, 128, 1, 64, 64, th.float32)
    tex, grid, jac, gout = tex[0].to(DEV), grid.to(DEV), jac.to(DEV), gout.to(DEV)
    a = tex.clone().requires_grad_(True)
    img = drtk_amd.mipmap_grid_sample(drtk_amd.mipmap_pyramid(a), grid, jac, 4)
    (img * gout).sum().backward()
    b = tex.clone().requires_grad_(True)
    chain = [b]
    for _ in range(7):
        chain.append(thf.avg_pool2d(chain[-1], 2))
    ref = drtk_amd.mipmap_grid_sample(chain, grid, jac, 4)
    (ref * gout).sum().backward()
    assert th.equal(img, ref)
    top = float(b.grad.abs().max())
    err = float((a.grad - b.grad).abs().max())
    print(f"end to end: tex.grad max abs err {err:.3e}, max |ref| {top:.3e}")
    assert err <= 1e-5 + (1e-5 + 2 * 8 * th.finfo(th.float32).eps) * top


def test_gradcheck_and_double_backward():
    import drtk_amd

    gen = th.Generator().manual_seed(3)
    x = th.rand(1, 2, 6, 10, generator=gen, dtype=th.float64).to(DEV).requires_grad_(True)
    assert th.autograd.gradcheck(lambda t: tuple(drtk_amd.mipmap_pyramid(t)), (x,), eps=1e-6, atol=1e-9, rtol=1e-7)
    assert th.autograd.gradcheck(lambda t: tuple(drtk_amd.mipmap_pyramid(t, 2)[1:]), (x,), eps=1e-6, atol=1e-9, rtol=1e-7)
    out = drtk_amd.mipmap_pyramid(x)
    with pytest.raises(RuntimeError, match="double backward"):
        th.autograd.grad(sum(t.sum() for t in out), x, create_graph=True)


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_more_views_than_one_launch_takes(dtype):
    """N = 65 537 views of one 2 x 2 channel, two levels (the view is blockIdx.y: the entry points run two slices), both
    ways through the C ABI: the first two views and the two either side of the slice boundary equal, bit for bit, those
    same views run alone."""
    from drtk_amd import capi

    N = 65537
    g = th.Generator(device=DEV).manual_seed(11)
    x = th.rand(N, 1, 2, 2, device=DEV, dtype=dtype, generator=g)
    grads = [th.rand(N, 1, 2, 2, device=DEV, dtype=dtype, generator=g), th.rand(N, 1, 1, 1, device=DEV, dtype=dtype, generator=g)]
    level1 = capi.mipmap_pyramid(x, 2)[1]
    grad_x = capi.mipmap_pyramid_backward(grads)
    assert level1.shape == (N, 1, 1, 1) and grad_x.shape == x.shape
    for views in (slice(0, 2), slice(65535, 65537)):
        assert th.equal(capi.mipmap_pyramid(x[views].contiguous(), 2)[1], level1[views]), views
        assert th.equal(capi.mipmap_pyramid_backward([t[views].contiguous() for t in grads]), grad_x[views]), views
