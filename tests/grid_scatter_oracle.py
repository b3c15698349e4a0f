"""TEST INFRASTRUCTURE (CPU, torch only) -- what `grid_scatter` is held to.

1. The ADJOINT ORACLE.  grid_scatter is defined as the adjoint of torch.nn.functional.grid_sample with respect to its
   texture, and that runs on the CPU in float32 and in float64:
       forward    the VJP of grid_sample at a zero texture with `input` as cotangent;
       backward   s = grid_sample(grad_out, grid) is grad_input, autograd.grad(s, grid, input) is grad_grid
                  (grid_sample has no double backward, so the backward cannot be taken through the forward).
2. A float64 RESTATEMENT with explicit weights (`restate`): the reference kernel's coordinate rule -- for bicubic the
   centre goes through the padding transform before floor, and every tap index goes through it again
   (grid_scatter_kernel.cu:140-177, grid_utils.h:83-164), where grid_sample only unnormalises the centre.  The two agree
   for every bilinear mode, for bicubic with zeros padding, and for bicubic border / reflection wherever the unnormalised
   coordinate lies in [0, size - 1]; outside that region (1) does not apply and this is the statement of what is wanted.
3. ACCUMULATED MAGNITUDES A: `restate(..., absolute=True)`, the same operator on absolute values of weights and values,
   for the per-element bound of tests/f64_distance.py -- and S (`coordinate_sensitivity`), the same with the weights
   replaced by their sensitivity to the rounding of the source coordinate, which A knows nothing about.
4. The CELL-FLIP PREDICATE (`flip_pixels`): pixels at which the float32 and the float64 evaluation of the coordinate
   choose a different floor cell or a different clip / reflect branch, in either axis.  The grid gradient is
   discontinuous there, so these pixels are excluded from the grad_grid comparison (never more than FLIP_CAP of a case).
   Computed from the grid alone, never from a kernel's output.
"""
import torch as th
import torch.nn.functional as F

MODES = ("bilinear", "bicubic")
PADDINGS = ("zeros", "border", "reflection")
MODE_ENUM = {"bilinear": 0, "bicubic": 2}
PADDING_ENUM = {"zeros": 0, "border": 1, "reflection": 2}
FLIP_CAP = 1e-4  # of a case's pixels


# ---- 1. the adjoint oracle ---------------------------------------------------------------------------------------------
def scatter(input, grid, oh, ow, mode, padding, align):
    tex = th.zeros(input.shape[0], input.shape[1], oh, ow, dtype=input.dtype, requires_grad=True)
    s = F.grid_sample(tex, grid, mode=mode, padding_mode=padding, align_corners=align)
    (g,) = th.autograd.grad(s, tex, input)
    return g


def scatter_backward(grad_out, input, grid, mode, padding, align):
    g = grid.detach().clone().requires_grad_(True)
    s = F.grid_sample(grad_out, g, mode=mode, padding_mode=padding, align_corners=align)
    (gg,) = th.autograd.grad(s, g, input)
    return s.detach(), gg


# ---- 2. / 3. restatement with explicit weights ---------------------------------------------------------------------------
def _unnormalize(c, size, align):
    return ((c + 1) / 2) * (size - 1) if align else ((c + 1) * size - 1) / 2


def _reflect(x, twice_low, twice_high):
    """-> (reflected coordinate, its derivative +-1, number of flips)"""
    if twice_low == twice_high:
        return th.zeros_like(x), th.zeros_like(x), th.zeros_like(x)
    mn, span = twice_low / 2, (twice_high - twice_low) / 2
    d = x - mn
    sign = th.where(d < 0, -th.ones_like(d), th.ones_like(d))
    d = d.abs()
    extra = th.fmod(d, span)
    flips = th.floor(d / span)
    even = flips % 2 == 0
    return th.where(even, extra + mn, span - extra + mn), th.where(even, sign, -sign), flips


def _reflect_for(x, size, align):
    return _reflect(x, 0, 2 * (size - 1)) if align else _reflect(x, -1, 2 * size - 1)


def source_index(coord, size, padding, align):
    """-> (source index after the padding transform, d index / d coord, branch id): the reference's
    grid_sampler_compute_source_index_set_grad.  `branch` names the clip / reflect case taken (for flip_pixels)."""
    x = _unnormalize(coord, size, align)
    m = th.full_like(x, (size - 1) / 2 if align else size / 2)
    branch = th.zeros_like(x)
    if padding == "reflection":
        x, s, flips = _reflect_for(x, size, align)
        m = m * s
        branch = branch + 4 * flips + 2 * (s < 0)
    if padding in ("border", "reflection"):
        lo, hi = x <= 0, x >= size - 1
        m = th.where(lo | hi, th.zeros_like(m), m)
        branch = branch * 4 + lo.to(x.dtype) + 2 * hi.to(x.dtype)
        x = x.clamp(0, size - 1)
    return x, m, branch


def _tap_index(k, size, padding, align):
    """compute_coordinates on an (integer-valued) tap coordinate, then the bounds test: (index, valid)"""
    if padding == "border":
        k = k.clamp(0, size - 1)
    elif padding == "reflection":
        k = _reflect_for(k, size, align)[0].clamp(0, size - 1)
    valid = (k >= 0) & (k <= size - 1)
    return k.clamp(0, size - 1).long(), valid


def _axis(coord, size, mode, padding, align):
    """-> index [...,K] long, valid [...,K], weight w [...,K], dw / d source index [...,K], d2w [...,K], d index / d coord [...],
    and the magnitudes the polynomials of w and dw are evaluated at (the sum of their absolute terms) [...,K] each"""
    x, m, _ = source_index(coord, size, padding, align)
    fl = th.floor(x)
    t = x - fl
    if mode == "bilinear":
        w = th.stack([1 - t, t], -1)
        dw = th.stack([-th.ones_like(t), th.ones_like(t)], -1)
        k = fl[..., None] + th.arange(0, 2, dtype=x.dtype)
        valid = (k >= 0) & (k <= size - 1)
        return k.clamp(0, size - 1).long(), valid, w, dw, th.zeros_like(w), m, th.zeros_like(w), th.zeros_like(w)
    A = -0.75
    d = th.stack([t + 1, t, 1 - t, 2 - t], -1)  # distance of the four taps
    sgn = th.tensor([1.0, 1.0, -1.0, -1.0], dtype=x.dtype)  # d distance / d t
    near, far = ((A + 2) * d - (A + 3)) * d * d + 1, ((A * d - 5 * A) * d + 8 * A) * d - 4 * A
    dnear, dfar = (3 * (A + 2) * d - 2 * (A + 3)) * d, (3 * A * d - 10 * A) * d + 8 * A
    inner = th.tensor([False, True, True, False])
    w = th.where(inner, near, far)
    dw = th.where(inner, dnear, dfar) * sgn
    d2w = th.where(inner, 6 * (A + 2) * d - 2 * (A + 3), 6 * A * d - 10 * A)
    idx, valid = _tap_index(fl[..., None] + th.arange(-1, 3, dtype=x.dtype), size, padding, align)
    pw = th.where(inner, (A + 2) * d ** 3 + (A + 3) * d ** 2 + 1, -A * (d ** 3 + 5 * d ** 2 + 8 * d + 4))
    pdw = th.where(inner, 3 * (A + 2) * d ** 2 + 2 * (A + 3) * d, -A * (3 * d ** 2 + 10 * d + 8))
    return idx, valid, w, dw, d2w, m, pw, pdw


def restate(input, grid, oh, ow, mode, padding, align, grad_out=None, absolute=False, sensitivity=False):
    """The reference kernel's rule in the dtype of the arguments (use float64): out [N,C,oh,ow], and with grad_out also
    (grad_input, grad_grid).  absolute=True: every weight, value and product replaced by its absolute value -- the
    magnitudes A that were accumulated into each element.  sensitivity=True (with absolute): the weights replaced by what
    rounding moves them by, in units of u -- see `coordinate_sensitivity`."""
    N, C, H, W = input.shape
    xi, xv, wx, dwx, d2wx, mx, pwx, pdwx = _axis(grid[..., 0], ow, mode, padding, align)
    yi, yv, wy, dwy, d2wy, my, pwy, pdwy = _axis(grid[..., 1], oh, mode, padding, align)
    K = wx.shape[-1]
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    val = ab(input).reshape(N, C, H * W)
    out = th.zeros(N, C, oh * ow, dtype=input.dtype)
    gi = th.zeros(N, C, H * W, dtype=input.dtype)
    ggx = th.zeros(N, H * W, dtype=input.dtype)
    ggy = th.zeros(N, H * W, dtype=input.dtype)
    go = None if grad_out is None else ab(grad_out).reshape(N, C, oh * ow)
    for i in range(K):
        for j in range(K):
            ok = (xv[..., i] & yv[..., j]).reshape(N, 1, H * W).to(input.dtype)
            ax, ay, bx, by, cx, cy = (t.abs() for t in (wx[..., i], wy[..., j], dwx[..., i], dwy[..., j], d2wx[..., i], d2wy[..., j]))
            if sensitivity:
                ex, ey = bx * ow + pwx[..., i], by * oh + pwy[..., j]  # what u moves wx / wy by
                w = ex * ay + ax * ey
                wgx = (cx * ow + pdwx[..., i]) * ay + bx * ey
                wgy = ex * by + ax * (cy * oh + pdwy[..., j])
            else:
                w, wgx, wgy = ab(wx[..., i] * wy[..., j]), ab(dwx[..., i] * wy[..., j]), ab(dwy[..., j] * wx[..., i])
            w = w.reshape(N, 1, H * W) * ok
            idx = (yi[..., j] * ow + xi[..., i]).reshape(N, 1, H * W).expand(N, C, H * W)
            out.scatter_add_(2, idx, val * w)
            if go is not None:
                g = go.gather(2, idx) * ok
                gi += g * w
                ggx += (g * val).sum(1) * wgx.reshape(N, H * W)
                ggy += (g * val).sum(1) * wgy.reshape(N, H * W)
    out = out.reshape(N, C, oh, ow)
    if go is None:
        return out
    gg = th.stack([ab(mx).reshape(N, H * W) * ggx, ab(my).reshape(N, H * W) * ggy], -1).reshape(N, H, W, 2)
    return out, gi.reshape(N, C, H, W), gg


def magnitudes(input, grid, oh, ow, mode, padding, align, grad_out=None):
    """A of tests/f64_distance.py for the forward output (and, with grad_out, for grad_input and grad_grid)."""
    return restate(input.double(), grid.double(), oh, ow, mode, padding, align, None if grad_out is None else grad_out.double(), absolute=True)


def coordinate_sensitivity(input, grid, oh, ow, mode, padding, align, grad_out=None):
    """S: what A leaves out.  The weights are functions of the source coordinate x = ((c + 1) * size - 1) / 2 (or its
    align_corners form), and ANY float32 evaluation of x is off by a few u * size in absolute terms -- the operations
    round at the magnitude of (c + 1) * size, not of the fractional part the weights are made of.  A weight therefore
    carries an ABSOLUTE error of a few u * size * |dw/dx|, however small the weight itself is: an element fed through
    a weight of 1e-6 has A ~ 1e-6 |v| and an honest error of u * size * |v|, thousands of u * A.  S accumulates
    |v| * (|dw/dx| * ow + |dw/dy| * oh) per element (for grad_grid with the weights' second derivatives).  The bicubic
    weights add an absolute error of their own: they are cubic polynomials whose terms (up to 8 |A| d = 12 at d = 2) cancel
    to a weight that may be 1e-6 -- u times the sum of the absolute terms, whatever is left after the cancellation.  With
    both, u * (A + S) is the scale two correct float32 evaluations of one element differ by."""
    return restate(input.double(), grid.double(), oh, ow, mode, padding, align, None if grad_out is None else grad_out.double(), absolute=True, sensitivity=True)


def rules_coincide(grid, oh, ow, mode, padding, align):
    """Is the adjoint oracle the statement of what the kernel computes for this grid?  (docstring, 2.)"""
    if mode == "bilinear" or padding == "zeros":
        return True
    g = grid.double()
    x, y = _unnormalize(g[..., 0], ow, align), _unnormalize(g[..., 1], oh, align)
    return bool(((x >= 0) & (x <= ow - 1) & (y >= 0) & (y <= oh - 1)).all())


# ---- 4. the cell-flip predicate --------------------------------------------------------------------------------------------
def flip_pixels(grid, oh, ow, padding, align):
    """bool [N,H,W]: the float32 and float64 evaluations of the coordinate of this float32 grid disagree on the floor cell
    or on the clip / reflect branch in either axis -- under grid_sample's rule (floor of the unnormalised coordinate for
    bicubic) or under the reference's (floor after the padding transform)."""
    assert grid.dtype == th.float32
    flag = th.zeros(grid.shape[:3], dtype=th.bool)
    for axis, size in ((0, ow), (1, oh)):
        c32, c64 = grid[..., axis], grid[..., axis].double()
        x32, _, b32 = source_index(c32, size, padding, align)
        x64, _, b64 = source_index(c64, size, padding, align)
        flag |= th.floor(x32).double() != th.floor(x64)
        flag |= b32.double() != b64
        flag |= th.floor(_unnormalize(c32, size, align)).double() != th.floor(_unnormalize(c64, size, align))
    return flag


# ---- seeded inputs of the tests ---------------------------------------------------------------------------------------------
def make_case(seed, N, C, H, W, oh, ow, dtype=th.float32, kind="uniform", extent=1.2):
    """-> (input, grid, grad_out), CPU.  kind: `uniform` grid in [-extent, extent]^2 (incoherent: neighbouring pixels land
    anywhere), `warp` a smooth warp of the identity (coherent, stays inside [-extent, extent])."""
    g = th.Generator().manual_seed(seed)
    inp = (th.rand(N, C, H, W, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    if kind == "uniform":
        grid = (th.rand(N, H, W, 2, generator=g, dtype=th.float64) * 2 - 1) * extent
    else:
        ys, xs = th.meshgrid(th.linspace(-1, 1, H, dtype=th.float64), th.linspace(-1, 1, W, dtype=th.float64), indexing="ij")
        ph = th.rand(N, 4, generator=g, dtype=th.float64) * 6.28
        gx = xs[None] + 0.08 * th.sin(3 * ys[None] + ph[:, 0, None, None]) + 0.05 * th.cos(2 * xs[None] + ph[:, 1, None, None])
        gy = ys[None] + 0.08 * th.cos(2 * xs[None] + ph[:, 2, None, None]) + 0.05 * th.sin(3 * ys[None] + ph[:, 3, None, None])
        grid = th.stack([gx, gy], -1) * (extent / 1.13)
    gout = (th.rand(N, C, oh, ow, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    return inp, grid.to(dtype), gout
