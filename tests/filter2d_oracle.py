"""TEST INFRASTRUCTURE (CPU, torch + numpy only) -- what `filter2d` is held to.

1. A RESTATEMENT of the operator from its index rule (include/drtk_amd.h, csrc/filter2d.hip), per axis, in any floating
   type: zero-insertion by `up`, a k-tap filter, decimation by `down`, written as the gather
       u = o down + up - 1 - lead,  i0 = floor(u / up),  phase = (i0 + 1) up - u - 1,
       y[o] = sum_t X[i0 + t] F[phase + t up]   while phase + t up < k
   with lead = pad0 and F = f reversed for the forward, lead = k - 1 - pad0(up <-> down) and F = f for the `backward` flag
   (the call that is the gradient of the operator with the factors exchanged), X outside the image 0 or read at one
   reflection that does not repeat the edge.  Each axis becomes a matrix [out, in] (`axis_matrix`), the image operator is
   My X Mx^T, horizontal pass first.  It is the yardstick for what the reference's PyTorch model cannot give: the
   `backward` flag under reflection, half, configurations outside the reference's table.
2. ACCUMULATED MAGNITUDES: the same operator on |x| and |f| (`apply(..., absolute=True)`), for tests/f64_distance.py.
3. `gradient_reach`: how near the border the `backward`-flag call under reflection may differ from the derivative of the
   forward (it reflects the incoming gradient instead of folding the border contributions back).
4. The filter design of make_resampling_kernel (Kaiser, Lanczos) in numpy float64, and the seeded CASE TABLE of the GPU
   suite and of tests/gen_golden_filter2d.py.
"""
import functools
import math

import numpy as np
import torch as th


# ---- 1. the restatement --------------------------------------------------------------------------------------------------
def pad0(k, up, down):
    if up == 1 and down == 1:
        return k // 2
    return (k - down + 1) // 2 if down != 1 else (k + up - 1) // 2


def pad1(k, up, down):
    if up == 1 and down == 1:
        return (k - 1) // 2
    return (k - down) // 2 if down != 1 else (k - up) // 2


def geometry(n, k, up, down, backward=False):
    """-> (lead, total, out) of one axis; ValueError where the operator is not defined."""
    if n < 1 or k < 1 or up < 1 or down < 1:
        raise ValueError("filter2d: sizes and factors must be at least 1")
    total = pad0(k, up, down) + pad1(k, up, down)
    lead = k - 1 - pad0(k, down, up) if backward else pad0(k, up, down)
    if lead < 0 or total - lead < 0:
        raise ValueError("filter2d: filter too short for the sampling factors")
    out = (n * up + total - k + down) // down
    if out < 1:
        raise ValueError("filter2d: output smaller than 1")
    return lead, total, out


def output_size(n, k, up, down):
    return geometry(n, k, up, down)[2]


def reflect_ok(n, k, up, down, backward=False):
    """torch's rule for reflect padding: the pad on either side is smaller than the axis."""
    lead, total, _ = geometry(n, k, up, down, backward)
    return -(-lead // up) < n and -(-(total - lead) // up) < n


def axis_matrix(n, f, up, down, reflect, backward=False, absolute=False):
    """[out, n] in f's dtype: row o holds the taps output o applies to the n inputs of the axis."""
    k = f.shape[0]
    lead, total, out = geometry(n, k, up, down, backward)
    if reflect and not reflect_ok(n, k, up, down, backward):
        raise ValueError("filter2d: reflection padding must be smaller than the axis")
    F = f if backward else f.flip(0)
    if absolute:
        F = F.abs()
    M = th.zeros(out, n, dtype=f.dtype)
    for o in range(out):
        u = o * down + up - 1 - lead
        i0 = u // up
        phase = (i0 + 1) * up - u - 1
        t = 0
        while phase + t * up < k:
            p = i0 + t
            if reflect:
                p = abs(p)
                p = (n - 1) - abs(n - 1 - p)
                assert 0 <= p < n
            if 0 <= p < n:
                M[o, p] += F[phase + t * up]
            t += 1
    return M


def apply(x, f, up=1, down=1, reflect=False, backward=False, absolute=False):
    """The operator on x [N,C,H,W] in x's dtype (float32 or float64; f is cast to it)."""
    assert x.ndim == 4 and f.ndim == 1 and x.dtype in (th.float32, th.float64)
    f = f.to(x.dtype)
    My = axis_matrix(x.shape[2], f, up, down, reflect, backward, absolute)
    Mx = axis_matrix(x.shape[3], f, up, down, reflect, backward, absolute)
    xa = x.abs() if absolute else x
    return th.matmul(My, th.matmul(xa, Mx.t()))  # horizontal first


def gradient(grad_out, f, up, down, reflect, x_shape):
    """What the package's backward returns: the `backward`-flag call with the factors exchanged; ValueError where that
    has not the input's shape (down > 1 and H or W not a multiple of it)."""
    g = apply(grad_out, f, down, up, reflect, backward=True)
    if tuple(g.shape) != tuple(x_shape):
        raise ValueError(f"filter2d backward: gradient {tuple(g.shape)} for an input {tuple(x_shape)}")
    return g


def autograd_gradient(x, grad_out, f, up, down, reflect):
    """The derivative of the restated forward, by autograd."""
    xr = x.detach().clone().requires_grad_(True)
    (g,) = th.autograd.grad(apply(xr, f, up, down, reflect), xr, grad_out)
    return g


# ---- 3. where the reflection gradient is the derivative --------------------------------------------------------------------
def gradient_reach(k, up, down):
    """Elements p of an axis of n inputs with reach <= p <= n - 1 - reach get the derivative of the forward from the
    `backward`-flag call under reflection.  Derivation, near side (the far side is the same with total - lead for lead):
    the forward folds what it reads left of the image, X[-1 ... -ceil(lead / up)], back onto inputs 1 ... ceil(lead / up)
    -- the reference's gradient leaves that out --, and the gradient call for input p reads grad_out[o] down to
    o = ceil((p up + lead - k + 1) / down), reflected where negative instead of absent: p < (k - 1 - lead) / up.  With
    lead <= total both are covered by p < ceil(max(total, k - 1) / up) + 1."""
    total = pad0(k, up, down) + pad1(k, up, down)
    return -(-max(total, k - 1) // up) + 1


# ---- 4. filter design and the case table --------------------------------------------------------------------------------
KAISER, LANCZOS = 0, 1


def design(n_taps, m=1, freq_div=1.0, gain=1.0, alias_guard_band=0.0, filter_type=KAISER):
    """make_resampling_kernel in numpy float64 -> float32 tensor of n_taps * m weights."""
    fh = (math.sqrt(2.0) - 1) / 2 / freq_div
    fc = 1 / 2 / freq_div - fh * alias_guard_band
    n = n_taps * m
    x = (np.arange(n, dtype=np.float64) - (n - 1) / 2) / m
    if filter_type == KAISER:
        L = (n - 1) / m
        df = 2 * fh / (m / 2)
        A = 2.285 * (n - 1) * np.pi * df + 7.95
        beta = 0.1102 * (A - 8.7) if A > 50 else (0.0 if A < 21 else 0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21))
        r = 2 * x / L if L > 0 else np.zeros_like(x)
        w = np.i0(beta * np.sqrt(np.clip(1 - r * r, 0, None))) / np.i0(beta)
        v = w * 2 * fc * np.sinc(2 * fc * x)
    else:
        a = np.ceil(2 * fc * (n - 1) / 2 / m)
        v = 2 * fc * np.sinc(2 * fc * x) * np.sinc(2 * fc * x / a) * (np.abs(2 * fc * x) < a)
    return th.from_numpy((v / v.sum() * gain).astype(np.float32))


# name: (up, down, filter -- ("random", k) or ("design", n_taps, m, freq_div, gain, filter_type) --, x shape, paddings)
BOTH = ("zeros", "reflection")
CASES = {
    "filt5": (1, 1, ("random", 5), (2, 3, 37, 70), BOTH),
    "filt65": (1, 1, ("design", 65, 1, 4.0, 1.0, KAISER), (1, 1, 70, 66), BOTH),
    "up2": (2, 1, ("design", 6, 2, 1.0, 2.0, KAISER), (2, 2, 19, 41), BOTH),
    "up4": (4, 1, ("design", 6, 4, 1.0, 4.0, LANCZOS), (1, 2, 9, 23), BOTH),
    "up8": (8, 1, ("design", 4, 8, 1.0, 8.0, KAISER), (1, 2, 9, 11), BOTH),
    "down2": (1, 2, ("design", 6, 2, 1.0, 1.0, KAISER), (2, 2, 46, 70), BOTH),
    "down4": (1, 4, ("design", 4, 4, 1.0, 1.0, KAISER), (1, 2, 72, 100), BOTH),
    "down8": (1, 8, ("design", 6, 8, 1.0, 1.0, KAISER), (1, 1, 80, 72), BOTH),
    "generic_3_2_12": (3, 2, ("random", 12), (1, 2, 24, 30), BOTH),
    "generic_2_3_10": (2, 3, ("random", 10), (1, 2, 24, 30), BOTH),
    "generic_2_1_7": (2, 1, ("random", 7), (1, 2, 24, 30), BOTH),
    "generic_1_2_7": (1, 2, ("random", 7), (1, 2, 24, 30), BOTH),
    "generic_3_1_9": (3, 1, ("random", 9), (1, 2, 24, 30), BOTH),
    "generic_1_1_1": (1, 1, ("random", 1), (1, 2, 24, 30), BOTH),
    "tiny": (1, 4, ("design", 4, 4, 1.0, 1.0, KAISER), (1, 1, 4, 4), ("zeros",)),
    "planes": (1, 1, ("random", 3), (65539, 1, 4, 4), ("reflection",)),
}
TUNED = ("filt5", "filt65", "up2", "up4", "up8", "down2", "down4", "down8", "tiny", "planes")  # (up, down, k) of the reference's table
CASE_PADDINGS = [(name, padding) for name, c in CASES.items() for padding in c[4]]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> (x, f, grad_out, up, down): float32 tensors, the same from call to call (do not modify them)."""
    up, down, filt, shape, _ = CASES[name]
    g = th.Generator().manual_seed(1000 + list(CASES).index(name))
    if filt[0] == "random":
        f = th.rand(filt[1], generator=g) * 2 - 1
    else:
        f = design(*filt[1:])
    x = th.rand(*shape, generator=g) * 2 - 1
    k = f.shape[0]
    oh, ow = output_size(shape[2], k, up, down), output_size(shape[3], k, up, down)
    grad_out = th.rand(shape[0], shape[1], oh, ow, generator=g) * 2 - 1
    return x, f, grad_out, up, down


def divisible(name):
    """Does the case's backward exist (H and W multiples of down)?"""
    up, down, _, shape, _ = CASES[name]
    return shape[2] % down == 0 and shape[3] % down == 0


@functools.lru_cache(maxsize=None)
def expected(name, padding):
    """The oracle on a case, computed once: dict of out / grad (None where the backward does not exist) in float32 and
    float64 and the accumulated magnitudes of both."""
    x, f, gout, up, down = make_case(name)
    reflect = padding == "reflection"
    r = {}
    for tag, dt in (("32", th.float32), ("64", th.float64)):
        r["out" + tag] = apply(x.to(dt), f, up, down, reflect)
        r["grad" + tag] = gradient(gout.to(dt), f, up, down, reflect, x.shape) if divisible(name) else None
    r["out_mag"] = apply(x.double(), f, up, down, reflect, absolute=True)
    r["grad_mag"] = apply(gout.double(), f, down, up, reflect, backward=True, absolute=True) if divisible(name) else None
    return r


# ---- 5. every tuned family ------------------------------------------------------------------------------------------------
# The (up, down, k) csrc/filter2d.hip instantiates with compile-time taps (F2D_TUNED; tests/test_filter2d_host.py requires
# this table to be exactly that set).  Symmetric under exchanging up and down: the gradient call of (u, d, k) is the family
# (d, u, k) with the `backward` flag, so running forward and gradient of every entry launches every family with both
# settings of the flag.  Not part of CASES: those have recorded fixtures.
FAMILIES = tuple([(1, 1, k) for k in (3, 5, 7, 9, 11, 13, 17, 25, 33, 49, 65)]
                 + [(u, d, k) for k in (4, 6, 8, 10, 12) for u, d in ((1, 2), (2, 1))]
                 + [(u, d, k) for k in (16, 24) for u, d in ((1, 4), (4, 1))]
                 + [(u, d, k) for k in (32, 48) for u, d in ((1, 8), (8, 1))])
# The forward output of every family: at least two tiles per axis at the widest (64) and the tallest (32) tile of the
# planner, a ragged last column tile at each of its widths (72 mod 64, 32, 16 = 8) and a ragged last row tile at the
# heights 32 and 16 (40 mod 32, 16 = 8); 2 x 3 planes.
FAMILY_OUT = (40, 72)
FAMILY_PLANES = (2, 3)
TILE_WIDTHS, TILE_HEIGHTS = (64, 32, 16), (32, 16, 8, 4, 2, 1)  # f2d_plan's candidates


def family_input(up, down):
    """(H, W) of the input: FAMILY_OUT * down / up where that is whole (every tuned family) -- else the next multiple of
    `down` above it (a generic configuration such as (3, 2, 12): its output is then a little larger than FAMILY_OUT)."""
    def axis(n):
        m = -(-n * down // up)
        return -(-m // down) * down

    return tuple(axis(n) for n in FAMILY_OUT)


@functools.lru_cache(maxsize=None)
def family_case(up, down, k):
    """-> (x, f, grad_out): float32 tensors, the same from call to call (do not modify them); f is random in [-1, 1)."""
    g = th.Generator().manual_seed(20000 + 1000 * up + 100 * down + k)
    f = th.rand(k, generator=g) * 2 - 1
    H, W = family_input(up, down)
    x = th.rand(*FAMILY_PLANES, H, W, generator=g) * 2 - 1
    grad_out = th.rand(*FAMILY_PLANES, output_size(H, k, up, down), output_size(W, k, up, down), generator=g) * 2 - 1
    return x, f, grad_out


@functools.lru_cache(maxsize=None)
def family_expected(up, down, k, padding, half=False):
    """The oracle on a family's case, computed once: out / grad in float32 and float64 and the accumulated magnitudes of
    both, like `expected`; with `half` on the inputs rounded to float16 (what a float16 image holds)."""
    return expected_on(*family_case(up, down, k), up, down, padding, half)


def expected_on(x, f, gout, up, down, padding, half=False):
    """family_expected on any float32 tensors x [N,C,H,W] (H and W multiples of `down`), f [k], grad_out."""
    if half:
        x, gout = x.half().float(), gout.half().float()
    reflect = padding == "reflection"
    r = {}
    for tag, dt in (("32", th.float32), ("64", th.float64)):
        r["out" + tag] = apply(x.to(dt), f, up, down, reflect)
        r["grad" + tag] = gradient(gout.to(dt), f, up, down, reflect, x.shape)
    r["out_mag"] = apply(x.double(), f, up, down, reflect, absolute=True)
    r["grad_mag"] = apply(gout.double(), f, down, up, reflect, backward=True, absolute=True)
    return r
