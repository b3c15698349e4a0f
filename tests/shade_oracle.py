"""TEST ORACLE for drtk_amd.shade -- the definition written in plain PyTorch for any dtype and device, independent of the
product (which never imports it), and the deterministic cases the CPU and GPU tests share.

    L = unit(light_dir);  n = unit(normal);  d = max(-(n . L), 0);  col = albedo * (d + ambient)
    specular:  w = unit(pos);  h = unit(L - w);  b = max(-(h . n), 1e-8);  col += b ** shininess * specular
    out = col where index != -1 else background (0 without one);   gamma:  out = max(out, 0) ** (1 / gamma)
    unit(x) = x / max(||x||, 1e-12)

Gradients come from autograd over `shade`, with the operator's conventions built into the expression: every max / clamp is a
`torch.where` select whose unused branch is fed a harmless value, so it can produce neither a gradient nor a NaN -- `d`
passes a gradient only where -(n . L) > 0, `b` only where -(h . n) > 1e-8, the gamma step only where its argument is > 0
(exactly 0 elsewhere), `unit` of a vector of norm <= 1e-12 is a constant, and the foreground images are replaced by ones at
background pixels (and the background by ones at foreground pixels) before anything is computed from them.

`reference` expands every parameter to one value per pixel first, so that autograd hands back the per-pixel terms of each
parameter gradient: their sum is the gradient, the sum of their absolute values is the magnitude that was accumulated into
it (the `acc_magnitude` of tests/f64_distance.py)."""
import os
import re
import zlib

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMAGES = ("normal_img", "pos_img", "background")  # albedo is either
PARAMS = {"light_dir": 3, "albedo": None, "ambient": None, "specular": None, "shininess": 1}  # None: C elements


def unit(x, dim=1):
    ss = (x * x).sum(dim, keepdim=True)
    big = ss.detach().sqrt() > 1e-12
    norm = th.where(big, ss, th.ones_like(ss)).sqrt()
    return th.where(big, x / norm, (x / 1e-12).detach())


def _per_pixel(p, N, H, W):
    """A parameter [K] / [N, K], or an image [N, K, H, W], as [N, K, H, W]."""
    if p.ndim == 4:
        return p
    return (p[None] if p.ndim == 1 else p)[:, :, None, None].expand(N, -1, H, W)


def shade(normal_img, light_dir, albedo, ambient, index_img=None, pos_img=None, specular=None, shininess=None, background=None,
          gamma=None):
    """The definition; parameters may be [K], [N, K] or already one value per pixel, [N, K, H, W]."""
    N, _, H, W = normal_img.shape
    fg = th.ones(N, 1, H, W, dtype=th.bool, device=normal_img.device) if index_img is None else (index_img != -1)[:, None]
    one = th.ones((), dtype=normal_img.dtype, device=normal_img.device)
    zero = th.zeros((), dtype=normal_img.dtype, device=normal_img.device)
    L = unit(_per_pixel(light_dir, N, H, W))
    n = unit(th.where(fg, normal_img, one))
    ndl = -(n * L).sum(1, keepdim=True)
    d = th.where(ndl > 0, ndl, zero)
    alb = _per_pixel(albedo, N, H, W)
    if albedo.ndim == 4:
        alb = th.where(fg, alb, one)
    col = alb * (d + _per_pixel(ambient, N, H, W))
    if specular is not None:
        w = unit(th.where(fg, pos_img, one))
        h = unit(L - w)
        hn = -(h * n).sum(1, keepdim=True)
        b = th.where(hn > 1e-8, hn, th.full_like(hn, 1e-8))
        col = col + th.pow(b, _per_pixel(shininess, N, H, W)) * _per_pixel(specular, N, H, W)
    if background is not None:
        out = th.where(fg, col, th.where(fg, one, background))
    else:
        out = th.where(fg, col, zero)
    if gamma is not None:
        pos = out > 0
        out = th.where(pos, th.pow(th.where(pos, out, one), 1.0 / gamma), zero)
    return out


def tutorial_shade(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, gloss, background):
    """The shading of the reference's hand-fitting tutorial, literally: blend with the mask, clamp(min=1e-8) ** (gloss * 40),
    pow(clamp(img, 0), 1 / 2.2).  Parameters [N, K]."""
    import torch.nn.functional as F

    mask = (index_img != -1)[:, None].to(normal_img.dtype)
    n = F.normalize(normal_img, dim=1)
    L = F.normalize(light_dir, dim=1)[:, :, None, None]
    diffuse = (-(n * L).sum(1, keepdim=True)).clamp(min=0)
    view = F.normalize(pos_img, dim=1)
    h = F.normalize(L - view, dim=1)
    spec = (-(h * n).sum(1, keepdim=True)).clamp(min=1e-8) ** (gloss[:, :, None, None] * 40)
    img = albedo[:, :, None, None] * (diffuse + ambient[:, :, None, None]) + spec * specular[:, :, None, None]
    img = mask * img + (1 - mask) * background
    return th.pow(img.clamp(min=0), 1 / 2.2)


def reference(inp, grad_out, dtype, device="cpu"):
    """{"out", "grad_<name>" for every floating-point input, "mag_<name>" for every parameter}: `inp` is a dict of the
    arguments of `shade` (CPU tensors, as `case` returns them); everything is evaluated in `dtype` on `device`."""
    N, _, H, W = inp["normal_img"].shape
    cast = lambda t: t.to(device=device, dtype=dtype) if t.is_floating_point() else t.to(device)  # noqa: E731
    leaves, full, args = {}, {}, {}
    for k, t in inp.items():
        if k == "gamma" or t is None:
            args[k] = t
            continue
        t = cast(t)
        if not t.is_floating_point():
            args[k] = t
            continue
        leaves[k] = t.detach().clone().requires_grad_(True)
        if leaves[k].ndim == 4:
            args[k] = leaves[k]
        else:  # a parameter: one value per pixel, so that its per-pixel terms can be read back
            full[k] = _per_pixel(leaves[k], N, H, W)
            full[k].retain_grad()
            args[k] = full[k]
    out = shade(**args)
    out.backward(cast(grad_out))
    res = {"out": out.detach()}
    for k, leaf in leaves.items():
        res["grad_" + k] = leaf.grad if leaf.grad is not None else th.zeros_like(leaf)
        if k in full:
            terms = full[k].grad if full[k].grad is not None else th.zeros(N, leaf.shape[-1], H, W, dtype=dtype, device=device)
            mag = terms.abs().sum((2, 3))
            res["mag_" + k] = (mag.sum(0) if leaf.ndim == 1 else mag).max()
    return res


# ---- the kernel's structure, read from its source ------------------------------------------------------------------------------

def kernel_constants():
    """(pixels per lane by dtype, pixels per workgroup by dtype, rows the finalize kernel adds per pass, doubles per row)."""
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "shade.hip")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(ROOT, "drtk_amd", "csrc", "common.hpp")).read()).group(1))
    num = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))  # noqa: E731
    P = {th.float32: num("kShadePixF32"), th.float64: num("kShadePixF64")}
    assert re.search(r"kShadePix = sizeof\(T\) == 4 \? kShadePixF32 : kShadePixF64;", src)
    assert re.search(r"tile_index\(a\.strip\)\) \* kBlock \+ threadIdx\.x\) \* P;", src)
    return P, {k: v * block for k, v in P.items()}, num("kShadeFinalRows"), num("kShadeTerms")


def _odd_width(total):
    """(H, W) with H W = total and W the odd divisor of total nearest its square root."""
    best = 1
    for w in range(1, int(total ** 0.5) + 2, 2):
        if total % w == 0:
            best = w
    return total // best, best


def _build_cases():
    P, B, S, _ = kernel_constants()
    cases = {}
    every = dict(index=True, specular=True, background=True, gamma=2.2, albedo_img=False)
    mixed = ("light_dir", "ambient")  # per view; the rest shared
    sizes = {1}
    for dt in P:
        sizes |= {P[dt] - 1, P[dt], P[dt] + 1, B[dt] - 1, B[dt], B[dt] + 1, 2 * B[dt] + 3}
    for hw in sorted(s for s in sizes if s >= 1):
        H, W = _odd_width(hw)
        cases[f"plane{hw}"] = dict(N=2, C=3, H=H, W=W, per_view=mixed, **every)
    for dt, tag in ((th.float32, "f32"), (th.float64, "f64")):
        for rows, name in ((S, "S"), (S + 1, "S+1"), (2 * S + 1, "2S+1")):
            H, W = _odd_width(rows * B[dt] - 1)
            cases[f"rows_{name}_{tag}"] = dict(N=2, C=3, H=H, W=W, per_view=(mixed if name == "S+1" else ()), **every)
    H, W = _odd_width(B[th.float32] + 1)
    for i, N in enumerate((1, 2, 3)):
        for j, C in enumerate((1, 3, 4)):
            cases[f"n{N}_c{C}"] = dict(N=N, C=C, H=H, W=W, per_view=(mixed if (i + j) % 2 else ("albedo", "specular", "shininess")),
                                       **dict(every, albedo_img=(i + j) % 2 == 0))
    cases["shared_all"] = dict(N=3, C=3, H=H, W=W, per_view=(), **every)
    cases["per_view_all"] = dict(N=3, C=3, H=H, W=W, per_view=tuple(PARAMS), **every)
    k = 0
    for index in (False, True):
        for specular in (False, True):
            for background in (False, True):
                for gamma in (None, 2.2):
                    cases[f"opt_i{int(index)}s{int(specular)}b{int(background)}g{int(gamma is not None)}"] = dict(
                        N=2, C=3, H=H, W=W, per_view=(mixed if k % 3 == 0 else ()), index=index, specular=specular,
                        background=background, gamma=gamma, albedo_img=k % 2 == 1)
                    k += 1
    return cases


CASES = _build_cases()
MARGIN = 1e-3


def categories(inp):
    """The per-pixel decisions of a case, in float64: dict of bool [N, H, W] (foreground, lit, highlight unclamped) and the
    smallest distance from a non-smooth point over the pixels that count."""
    n = unit(inp["normal_img"].double())
    N, _, H, W = n.shape
    L = unit(_per_pixel(inp["light_dir"].double(), N, H, W))
    ndl = -(n * L).sum(1)
    fg = th.ones(N, H, W, dtype=th.bool) if inp["index_img"] is None else inp["index_img"] != -1
    res = {"fg": fg, "lit": ndl > 0, "ndl": ndl}
    if inp["specular"] is not None:
        hv = L - unit(inp["pos_img"].double())
        hn = -(unit(hv) * n).sum(1)
        res.update(open=hn > 1e-8, hn=hn, hv=hv.norm(dim=1))
    return res


def case(name):
    """The arguments of `shade` for CASES[name] and a grad_out, as CPU float64 tensors whose values are float32 numbers (so
    both precisions see the same inputs): deterministic, and at a margin from every non-smooth point -- each pixel is drawn
    again until |n . L| >= 1e-3 and |h . n| >= 1e-3 (and ||L - w|| >= 0.1), input norms are >= 0.1, albedo, ambient, specular
    and background are >= 0.05 (so the value before gamma is >= 1e-3)."""
    return build_case(CASES[name], zlib.crc32(name.encode()), name)


def build_case(c, seed, name="case"):
    """`case` for any description `c` with the keys of a CASES entry (N, C, H, W, per_view, index, specular, background, gamma,
    albedo_img), drawn from a generator seeded with `seed` (tests/fuzz_added_ops.py draws its own descriptions)."""
    N, C, H, W = c["N"], c["C"], c["H"], c["W"]
    gen = th.Generator().manual_seed(seed)
    f32 = lambda t: t.float().double()  # noqa: E731
    rand = lambda *s: th.rand(*s, generator=gen, dtype=th.float64)  # noqa: E731

    def directions(*lead):
        g = th.randn(*lead, 3, generator=gen, dtype=th.float64)
        return g / g.norm(dim=-1, keepdim=True).clamp(min=1e-3)

    def param(key, value):
        return f32(value if key in c["per_view"] else value[0])

    def vectors(lo, hi):  # [N, 3, H, W], norms in [lo, hi]
        return f32((directions(N, H, W) * (lo + (hi - lo) * rand(N, H, W, 1))).permute(0, 3, 1, 2).contiguous())

    inp = {"normal_img": vectors(0.2, 2.0), "light_dir": param("light_dir", directions(N) * (0.5 + 1.5 * rand(N, 1)))}
    inp["albedo"] = f32(0.05 + 0.95 * rand(N, C, H, W)) if c["albedo_img"] else param("albedo", 0.05 + 0.95 * rand(N, C))
    inp["ambient"] = param("ambient", 0.05 + 0.45 * rand(N, C))
    inp["index_img"] = None
    if c["index"]:
        idx = th.randint(0, 1000, (N, H, W), generator=gen, dtype=th.int32)
        inp["index_img"] = th.where(rand(N, H, W) < 0.35, th.full_like(idx, -1), idx)
    inp["pos_img"] = inp["specular"] = inp["shininess"] = None
    if c["specular"]:
        inp["pos_img"] = vectors(0.5, 3.0)
        inp["specular"] = param("specular", 0.05 + 0.95 * rand(N, C))
        inp["shininess"] = param("shininess", 1.5 + 28.5 * rand(N, 1))
    inp["background"] = f32(0.05 + 0.95 * rand(N, C, H, W)) if c["background"] else None
    inp["gamma"] = c["gamma"]
    for _ in range(200):
        cat = categories(inp)
        bad = cat["ndl"].abs() < 2 * MARGIN
        if c["specular"]:
            bad |= (cat["hn"].abs() < 2 * MARGIN) | (cat["hv"] < 0.2)
        if not bool(bad.any()):
            break
        m = bad[:, None]
        inp["normal_img"] = th.where(m, vectors(0.2, 2.0), inp["normal_img"])
        if c["specular"]:
            inp["pos_img"] = th.where(m, vectors(0.5, 3.0), inp["pos_img"])
    else:
        raise AssertionError(f"{name}: no draw with the margins")
    t = th.arange(N * C * H * W, dtype=th.float64).view(N, C, H, W)
    grad_out = f32(th.cos(t * 0.37) * (0.5 + rand(N, C, H, W)))
    return inp, grad_out


def shares(inp):
    """The fraction of the case's pixels in each category it has: foreground / background (with an index image), lit / unlit,
    highlight clamped / unclamped (with specular) -- the last four among the foreground pixels, as fractions of all pixels."""
    cat = categories(inp)
    fg, total = cat["fg"], cat["fg"].numel()
    res = {"lit": (fg & cat["lit"]).sum() / total, "unlit": (fg & ~cat["lit"]).sum() / total}
    if inp["index_img"] is not None:
        res.update(foreground=fg.sum() / total, background=(~fg).sum() / total)
    if inp["specular"] is not None:
        res.update(unclamped=(fg & cat["open"]).sum() / total, clamped=(fg & ~cat["open"]).sum() / total)
    return {k: float(v) for k, v in res.items()}
