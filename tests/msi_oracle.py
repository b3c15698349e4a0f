"""TEST INFRASTRUCTURE -- CPU oracle of `msi` (multi-sphere-image ray marching), written from the description of the
operator: the reference has a CUDA kernel only, no CPU kernel and no `*_ref` model, so there is nothing to record fixtures
from.  torch on the CPU, vectorised over rays, one Python iteration per marching step; everything (the ray geometry too) is
carried in the dtype of the texture, so the float64 run is the exact statement the float32 kernel is held to.

Per ray: d = ray_d / |ray_d|, tc = -o.d, h2 = o.o - tc^2, n = L * sub_step_count, s = 1 / n; for i = 0 .. n-1 (inside out):
a = (n - 1 - i + 0.5) / n, inv_r = (1 - a) max_inv_r + a min_inv_r, r = 1 / inv_r, det = r^2 - h2 (det < 0: the sphere is
skipped), pos = o + (tc + sqrt(det)) d, u = atan2(pos.z, pos.x) / pi, v = 2 atan2(pos.y, |(pos.x, pos.z)|) / pi, w = 1 - 2a;
the texture [L,4,H,W] is sampled at (u, v, w) -- align_corners=False unnormalisation, clipped to [0, size - 1], bilinear in
(x, y), cubic convolution (A = -0.75) over the layers floor(z) - 1 ... floor(z) + 2, each clipped to [0, L - 1] -- and a
sample with sigma > 0 is composited: p = sigma s, weight = exp(lt) (1 - exp(-p)), lt -= p, rgb_out += weight max(rgb, 0);
exp(lt) < stop_thresh sets lt = -1000 and ends the ray.

`march()` returns the forward, the backward by the REFERENCE'S formulas (its sigma gradient is not the derivative of the
forward: SIGMA_IDENTITY), the same backward on absolute values (accumulated magnitudes), the per-ray decision margin and
the bookkeeping the tests use to show that a case exercises what it is named for.

Backward (texture only; grad_out[:, 3] is ignored): re-march with g = grad_out[:, :3] and acc = g * out_rgb; at each counted
sample the colour gradient is [rgb >= 0] weight g (the reference tests max(rgb, 0) == rgb), then acc -= weight max(rgb, 0) g, and the sigma gradient is
sum_ch(max(rgb, 0) g exp(-sigma) exp(lt_after) - acc); the four values go through the same sixteen taps and weights.

SIGMA_IDENTITY: with T = exp(lt_after), d(loss)/d(sigma) of the forward is s (ref + sum_ch max(rgb, 0) g T (1 - exp(-sigma))),
`ref` the expression above.  The operator keeps `ref` (what users of the reference trained against).

Decision margin of a ray: the minimum over the steps it takes of |det| / r^2, and at a sample of |sigma|, of |pos.z| / |pos|
where pos.x < 0 (the seam of atan2), and -- where the sample counts -- of min |rgb| and |lt_after - ln(stop_thresh)|.  Every
branch of the march is a comparison of one of these with zero; a ray whose float64 margin is below FRAGILE_MARGIN may take
another branch in float32 and is left out of comparisons."""
import math
from types import SimpleNamespace

import torch as th

A = -0.75
FRAGILE_MARGIN = 1e-5  # float64 margin below which float32 and float64 may legitimately take different branches
FRAGILE_CAP = 1e-3     # fraction of a case's rays that may be fragile


def cubic_coefficients(t):
    """[..., 4] cubic-convolution weights of the taps floor - 1 ... floor + 2 at fractional position t"""
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    outer = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A  # noqa: E731
    inner = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1  # noqa: E731
    return th.stack([outer(x0), inner(x1), inner(x2), outer(x3)], -1)


def _unnormalise_clip(c, size):
    return (((c + 1) * size - 1) / 2).clamp(0, size - 1)


def taps(u, v, w, L, H, W):
    """The sixteen taps of a sample: flat texel indices (l * H + y) * W + x [M,4,4] (layer, corner), the bilinear corner
    weights [M,4] (nw, ne, sw, se; a +1 neighbour past the last column / row has weight 0 and index of the last one) and the
    layer coefficients [M,4]."""
    x, y, z = _unnormalise_clip(u, W), _unnormalise_clip(v, H), _unnormalise_clip(w, L)
    x0, y0, z0 = x.floor(), y.floor(), z.floor()
    wx1, wy1 = x - x0, y - y0
    wx0, wy0 = (x0 + 1) - x, (y0 + 1) - y
    x0, y0, z0 = x0.long(), y0.long(), z0.long()
    x1ok, y1ok = x0 + 1 < W, y0 + 1 < H
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    zero = th.zeros_like(wx0)
    wb = th.stack([wx0 * wy0, th.where(x1ok, wx1 * wy0, zero), th.where(y1ok, wx0 * wy1, zero), th.where(x1ok & y1ok, wx1 * wy1, zero)], -1)
    corner = th.stack([y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1], -1)  # [M,4]
    layers = (z0[:, None] - 1 + th.arange(4)).clamp(0, L - 1)  # [M,4]
    idx = layers[:, :, None] * (H * W) + corner[:, None, :]
    return idx, wb, cubic_coefficients(z - z0.to(z.dtype))


def march(ray_o, ray_d, texture, sub_step_count=2, min_inv_r=1.0, max_inv_r=0.0, stop_thresh=1e-7, grad_out=None, out=None, analytic_sigma=False):
    """Forward (grad_out None) or forward + backward.  Returns a namespace:
      out [N,4]; with grad_out [N,4] (column 3 is ignored) also grad_texture [L,4,H,W] and magnitudes [L,4,H,W] -- `out` (the
      saved forward result the backward starts its running sum from) defaults to this forward's;
      margin [N] (float64; the decision margin of the module docstring), skipped [N] (the ray skipped a sphere), stopped [N]
      (ended early), taken [N] / edge [N] (samples taken; of those, sigma <= 0 or a clamped colour).
    analytic_sigma: scatter the derivative of the forward instead of the reference's sigma expression (see
    `SIGMA_IDENTITY`); only the tests of the identity use it."""
    dt = texture.dtype
    L, C, H, W = texture.shape
    assert C == 4
    N = ray_o.shape[0]
    o = ray_o.to(dt)
    d = ray_d.to(dt)
    d = d / d.norm(dim=1, keepdim=True)
    tc = -(o * d).sum(1)
    h2 = (o * o).sum(1) - tc * tc
    n = L * int(sub_step_count)
    s = 1.0 / n
    texels = texture.permute(0, 2, 3, 1).reshape(L * H * W, 4)
    log_thresh = math.log(stop_thresh)

    def run(backward, absolute=False, fwd_out=None):
        lt = th.zeros(N, dtype=dt)
        rgb_out = th.zeros(N, 3, dtype=dt)
        alive = th.ones(N, dtype=th.bool)
        margin = th.full((N,), float("inf"), dtype=dt)
        skipped, stopped = th.zeros(N, dtype=th.bool), th.zeros(N, dtype=th.bool)
        taken, edge = th.zeros(N, dtype=th.long), th.zeros(N, dtype=th.long)
        if backward:
            g = grad_out[:, :3].to(dt)
            g = g.abs() if absolute else g
            acc = g * fwd_out[:, :3]
            grad = th.zeros(L * H * W, 4, dtype=dt)
        for i in range(n):
            a = (n - 1 - i + 0.5) / n
            r = 1.0 / ((1 - a) * max_inv_r + a * min_inv_r)
            det = r * r - h2
            hit = alive & ~(det < 0)
            margin = th.where(alive, th.minimum(margin, det.abs() / (r * r)), margin)
            skipped |= alive & (det < 0)
            m = hit.nonzero()[:, 0]
            if m.numel() == 0:
                continue
            pos = o[m] + (tc[m] + det[m].sqrt())[:, None] * d[m]
            u = th.atan2(pos[:, 2], pos[:, 0]) / math.pi
            v = 2 * th.atan2(pos[:, 1], th.sqrt(pos[:, 0] * pos[:, 0] + pos[:, 2] * pos[:, 2])) / math.pi
            w = th.full_like(u, 1 - 2 * a)
            idx, wb, co = taps(u, v, w, L, H, W)
            per_layer = (texels[idx] * wb[:, None, :, None]).sum(2)  # [M,4 layers,4 channels]
            sample = (per_layer * co[:, :, None]).sum(1)
            rgb, sigma = sample[:, :3], sample[:, 3]
            counted = sigma > 0
            seam = th.where(pos[:, 0] < 0, pos[:, 2].abs() / pos.norm(dim=1), th.full_like(u, float("inf")))
            step_margin = th.minimum(sigma.abs(), seam)
            step_margin = th.where(counted, th.minimum(step_margin, rgb.abs().min(1).values), step_margin)
            taken[m] += 1
            edge[m] += (~counted | (rgb < 0).any(1)).long()
            p = sigma * s
            weight = th.exp(lt[m]) * (1 - th.exp(-p))
            lt_after = lt[m] - p
            rgb01 = rgb.clamp(min=0)
            step_margin = th.where(counted, th.minimum(step_margin, (lt_after - log_thresh).abs()), step_margin)
            margin[m] = th.minimum(margin[m], step_margin)
            c = m[counted]
            if backward and c.numel():
                gc, wc = g[c], weight[counted][:, None]
                colour = (rgb[counted] >= 0).to(dt) * wc * gc  # the reference's max(rgb, 0) == rgb: a colour of exactly 0 passes its gradient on
                moved = wc * rgb01[counted] * gc
                acc[c] = acc[c] - moved
                term = rgb01[counted] * gc * th.exp(-sigma[counted])[:, None] * th.exp(lt_after[counted])[:, None]
                sig = (term + acc[c]).sum(1) if absolute else (term - acc[c]).sum(1)
                if analytic_sigma:
                    sig = s * (sig + (rgb01[counted] * gc * (th.exp(lt_after[counted]) * (1 - th.exp(-sigma[counted])))[:, None]).sum(1))
                g4 = th.cat([colour, sig[:, None]], 1)  # [K,4]
                cw = co[counted].abs() if absolute else co[counted]
                val = (wb[counted][:, None, :, None] * g4[:, None, None, :]) * cw[:, :, None, None]  # [K,4 layers,4 corners,4 channels]
                grad.index_add_(0, idx[counted].reshape(-1), val.reshape(-1, 4))
            rgb_out[c] = rgb_out[c] + weight[counted][:, None] * rgb01[counted]
            lt[c] = lt_after[counted]
            stop = c[th.exp(lt[c]) < stop_thresh]
            lt[stop] = -1000.0
            alive[stop] = False
            stopped[stop] = True
        res = SimpleNamespace(out=th.cat([rgb_out, lt[:, None]], 1), margin=margin.double(), skipped=skipped, stopped=stopped, taken=taken, edge=edge)
        if backward:
            res.grad = grad.reshape(L, H, W, 4).permute(0, 3, 1, 2).contiguous()
        return res

    res = run(False)
    if grad_out is not None:
        fwd_out = res.out if out is None else out.to(dt)
        res.grad_texture = run(True, False, fwd_out).grad
        res.magnitudes = run(True, True, fwd_out).grad
    return res


def forward_autograd(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh):
    """The forward once more, ray by ray with plain differentiable torch operations: what autograd makes of the forward
    (the colour gradient equals the reference's; the sigma gradient obeys `sigma_gradient_identity`).  Slow: tiny cases."""
    dt = texture.dtype
    L, _, H, W = texture.shape
    texels = texture.permute(0, 2, 3, 1).reshape(L * H * W, 4)
    n = L * int(sub_step_count)
    outs = []
    for k in range(ray_o.shape[0]):
        o = ray_o[k].to(dt)
        d = ray_d[k].to(dt)
        d = d / d.norm()
        tc = -(o * d).sum()
        h2 = (o * o).sum() - tc * tc
        lt = th.zeros((), dtype=dt)
        rgb_out = th.zeros(3, dtype=dt)
        for i in range(n):
            a = (n - 1 - i + 0.5) / n
            r = 1.0 / ((1 - a) * max_inv_r + a * min_inv_r)
            det = r * r - h2
            if det < 0:
                continue
            pos = o + (tc + det.sqrt()) * d
            u = th.atan2(pos[2], pos[0]) / math.pi
            v = 2 * th.atan2(pos[1], th.sqrt(pos[0] * pos[0] + pos[2] * pos[2])) / math.pi
            idx, wb, co = taps(u[None], v[None], th.full((1,), 1 - 2 * a, dtype=dt), L, H, W)
            sample = ((texels[idx[0]] * wb[0][None, :, None]).sum(1) * co[0][:, None]).sum(0)
            if sample[3] > 0:
                p = sample[3] / n
                rgb_out = rgb_out + th.exp(lt) * (1 - th.exp(-p)) * sample[:3].clamp(min=0)
                lt = lt - p
                if th.exp(lt) < stop_thresh:
                    lt = th.full((), -1000.0, dtype=dt)
                    break
        outs.append(th.cat([rgb_out, lt[None]]))
    return th.stack(outs)


def draw_rays(g, N, origin_radius):
    """(origins uniform in a ball, unnormalised directions of length 0.1 ... 3) [N,3] float64 from the generator `g`"""
    rnd = lambda *shape: th.rand(*shape, generator=g, dtype=th.float64)  # noqa: E731
    unit = lambda x: x / x.norm(dim=1, keepdim=True)  # noqa: E731
    o = unit(th.randn(N, 3, generator=g, dtype=th.float64)) * (rnd(N, 1) ** (1 / 3) * origin_radius)
    d = unit(th.randn(N, 3, generator=g, dtype=th.float64)) * (rnd(N, 1) * 2.9 + 0.1)
    return o, d


def make_case(seed, N, L, H, W, sigma_range, origin_radius, dtype=th.float32, generator=None):
    """Seeded inputs: rgb in [-0.2, 1.2] (three texels in ten in [-0.2, 0), the others in [0, 1.2]), sigma uniform in sigma_range, origins
    uniform in a ball, unnormalised directions of length 0.1 ... 3, grad_out in [-1, 1].  Generated in double and rounded to float32 (the rays always are float32).
    `generator`: one seeded by the caller, who goes on drawing from it (build_case), instead of a new one seeded with `seed`."""
    g = th.Generator().manual_seed(seed) if generator is None else generator
    rnd = lambda *shape: th.rand(*shape, generator=g, dtype=th.float64)  # noqa: E731
    tex = th.empty(L, 4, H, W, dtype=th.float64)
    # three colour texels in ten negative: after sixteen taps of averaging a uniform draw hardly ever clamps.  With rgb uniform
    # in [-0.2, 1.2] the share of samples with sigma <= 0 or a clamped colour, over seeds 1 ... 29 of each case, was 5.7 - 10.4 %
    # (inside), 6.0 - 12.7 % (outside_skip, 9 seeds), 3.7 - 7.8 % (early_stop): no seed of early_stop reaches the tenth the
    # cases must show, so the distribution inside the stated range was changed, not only the seed (now 16 - 35 %).
    tex[:, :3] = th.where(rnd(L, 3, H, W) < 0.3, rnd(L, 3, H, W) * -0.2, rnd(L, 3, H, W) * 1.2)
    tex[:, 3] = rnd(L, H, W) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
    o, d = draw_rays(g, N, origin_radius)
    gout = rnd(N, 4) * 2 - 1
    return o.float(), d.float(), tex.float().to(dtype), gout.float().to(dtype)


# The cases of tests/test_gpu_msi.py and tests/test_msi_host.py: name -> (seed, N, (L, H, W), sub_step_count, min_inv_r, max_inv_r, stop_thresh,
# sigma range, origin radius).  The seeds are the first for which the case shows what it is
# named for (tests/test_msi_host.py asserts it).
CASES = {
    "inside": (1, 4099, (4, 8, 16), 2, 1.0, 0.0, 1e-7, (-0.5, 2.5), 0.8),
    "outside_skip": (1, 4096, (3, 5, 7), 3, 1.0, 0.05, 1e-7, (-0.5, 2.5), 2.5),
    "early_stop": (9, 4096, (6, 8, 16), 2, 1.0, 0.1, 1e-2, (0.0, 12.0), 0.5),
    "one_layer": (1, 1024, (1, 4, 4), 1, 2.0, 0.5, 1e-7, (-0.5, 2.5), 0.3),
}
_cache = {}


def case(name):
    """(inputs, march arguments, fragile mask, float64 result, float32 result) of a case, computed once: the fragile rays'
    grad_out rows are zeroed, for the oracle here and for the kernel in the GPU suite alike."""
    if name not in _cache:
        _cache[name] = build_case(*CASES[name])
    return _cache[name]


REDRAW_ROUNDS = 20


def build_case(seed, N, shape, sub, mn, mx, stop, sig, rad, redraw=False):
    """`case` for any parameters (the tuple of a CASES entry).  `redraw` (tests/fuzz_added_ops.py, whose cases have too few
    rays for a share of them to be left out): the fragile rays are drawn again from the same generator until none is left,
    at most REDRAW_ROUNDS times, so that every ray is compared; the fragile mask returned is then empty."""
    L, H, W = shape
    g = th.Generator().manual_seed(seed)
    o, d, tex, gout = make_case(seed, N, L, H, W, sig, rad, generator=g)
    args = (sub, mn, mx, stop)
    fragile = march(o, d, tex.double(), *args).margin < FRAGILE_MARGIN
    if redraw:
        for _ in range(REDRAW_ROUNDS):
            if not bool(fragile.any()):
                break
            o2, d2 = draw_rays(g, int(fragile.sum()), rad)
            o, d = o.clone(), d.clone()
            o[fragile], d[fragile] = o2.float(), d2.float()
            fragile = march(o, d, tex.double(), *args).margin < FRAGILE_MARGIN
        assert not bool(fragile.any()), f"{int(fragile.sum())} fragile rays after {REDRAW_ROUNDS} redraws"
    gout = gout.clone()
    gout[fragile] = 0
    r64 = march(o, d, tex.double(), *args, grad_out=gout.double())
    r32 = march(o, d, tex, *args, grad_out=gout)
    return ((o, d, tex, gout), args, fragile, r64, r32)
