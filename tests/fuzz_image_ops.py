"""TEST INFRASTRUCTURE ONLY (not collected by pytest) -- seeded random shapes for the image losses (`ssim` as a map, `ssim` as
a mean, `photometric_loss`) and for `mipmap_pyramid`, each through the ctypes binding of the C ABI (poisoned outputs, and
with DRTK_CAPI_GUARD sentinels around every output and workspace) and through the Python API under autograd.

usage: python tests/fuzz_image_ops.py [--first S] [--cases K]      cases make_case(S) .. make_case(S + K - 1)

Image losses: 1 .. 6 views (one case in sixteen: 257 .. 600 views of at most 12 x 12 pixels, more partial sums than one pass
of the finalize kernel takes), 1 .. 4 channels, sizes drawn towards 1, the window's size and one either side of it, and the
tile's multiples 32, 64, 96 with two either side, up to 140; odd windows 3 .. 15, sigma 0.5 .. 3, both paddings, data ranges
1 and 255, no weight / bool [N,H,W] / bool [N,1,H,W] / float, both precisions, and inputs that are contiguous, a channel
slice of a wider tensor, a row and column slice of a larger image, or one element into a flat buffer.  Compared with
tests/image_loss_oracle.py under the two bounds of tests/test_gpu_image_loss.py (float64: 1e-12 of max(1, max|ref|);
float32: 4 x the float32 formulation's own error); the binding and the Python API agree bit for bit.

mipmap_pyramid: 1 .. 3 views, 1 .. 5 channels, 1 .. 200 texels a side drawn towards 63 .. 66 and 127 .. 130, 1 .. all levels,
a random subset of the level gradients absent, the input one element into a flat buffer in half of the cases.  Bit for bit
against the definition and the backward recurrence of tests/test_gpu_mipmap_pyramid.py.

tests/test_gpu_fuzz_image_ops.py runs seeds 0 .. 239 in five blocks of 48; tests/guarded_added_ops.py runs the first 20 under guards.
Measured on an MI355X: a block of 48 cases takes 0.6 to 2.5 s; `--first 0 --cases 200` runs its cases in 4.8 s, 7.1 s
of wall time with the start of the process.
"""
import argparse
import os

os.environ.setdefault("DRTK_CAPI_POISON", "1")  # outputs of the ctypes binding pre-filled with NaN / sentinels (drtk_amd/capi.py _out)
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

import image_loss_oracle as O  # noqa: E402

DEV = "cuda:0"
OPS = ("ssim_map", "ssim_mean", "photometric_loss", "mipmap_pyramid")
WEIGHTS = ("none", "bool_NHW", "bool_N1HW", "float")
LAYOUTS = ("contiguous", "channel_slice", "row_column_slice", "one_element_in")
MANY_VIEWS = (257, 600)  # more than the 256 slots of one pass of image_loss_finalize_kernel


def make_case(seed):
    """A dict of plain numbers and names; the tensors are made from them in run_case."""
    g = th.Generator().manual_seed(1000003 * seed + 29)
    r = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    pick = lambda seq: seq[r(0, len(seq) - 1)]  # noqa: E731
    op = pick(OPS)
    c = dict(seed=seed, op=op, dtype=pick(("f32", "f64")))
    if op == "mipmap_pyramid":
        near = [63, 64, 65, 66, 127, 128, 129, 130]
        size = lambda: pick(near) if r(0, 2) == 0 else r(1, 200)  # noqa: E731
        c.update(N=r(1, 3), C=r(1, 5), H=size(), W=size(), layout=pick(("contiguous", "one_element_in")))
        top = min(11, min(c["H"], c["W"]).bit_length())
        c["levels"] = r(1, top)
        absent = [r(0, 2) == 0 for _ in range(c["levels"])]
        if all(absent):
            absent[r(0, c["levels"] - 1)] = False
        c["absent"] = tuple(l for l, a in enumerate(absent) if a)
        return c
    k = 2 * r(1, 7) + 1
    many = r(0, 15) == 0
    if many and op == "ssim_map":  # the map has no partial sums: one of the two means instead
        op = c["op"] = pick(OPS[1:3])
    if many:
        near = [s for s in (1, k - 1, k, k + 1) if s <= 12]
        size = lambda: pick(near) if r(0, 2) == 0 else r(1, 12)  # noqa: E731
    else:
        near = [1, k - 1, k, k + 1, 31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 98]
        size = lambda: pick(near) if r(0, 2) < 2 else r(1, 140)  # noqa: E731
    c.update(N=r(*MANY_VIEWS) if many else r(1, 6), C=r(1, 4), H=size(), W=size(), k=k)
    c["sigma"] = 0.5 + 2.5 * float(th.rand(1, generator=g, dtype=th.float64))
    c["padding"] = pick(("same", "valid")) if min(c["H"], c["W"]) >= k else "same"
    c["data_range"] = pick((1.0, 255.0))
    c["weight"] = "none" if op == "ssim_map" else pick(WEIGHTS)
    c["layout"] = pick(LAYOUTS)
    return c


def describe(c):
    head = f"seed={c['seed']} {c['op']} N={c['N']} C={c['C']} H={c['H']} W={c['W']} {c['dtype']} {c['layout']}"
    if c["op"] == "mipmap_pyramid":
        return head + f" levels={c['levels']} absent={list(c['absent'])}"
    return head + f" window={c['k']} sigma={c['sigma']:.3f} {c['padding']} data_range={c['data_range']:g} weight={c['weight']}"


def one_element_in(t):
    """`t` as a contiguous tensor one element into a flat buffer: merely element-aligned."""
    flat = th.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def laid_out(t, layout, fill):
    """`t` [N,C,H,W] or [N,H,W] with the same values in another layout, whatever lies around it filled with `fill`."""
    if layout == "contiguous":
        return t
    if layout == "one_element_in":
        return one_element_in(t)
    if layout == "channel_slice" and t.ndim == 4:
        wide = th.full((t.shape[0], t.shape[1] + 1, *t.shape[2:]), fill, dtype=t.dtype, device=t.device)
        wide[:, :t.shape[1]] = t
        return wide[:, :t.shape[1]]
    H, W = t.shape[-2:]  # a row and column slice (for a weight [N,H,W] also where the images are channel slices)
    big = th.full((*t.shape[:-2], H + 5, W + 3), fill, dtype=t.dtype, device=t.device)
    big[..., 2:2 + H, 1:1 + W] = t
    return big[..., 2:2 + H, 1:1 + W]


def run_image_loss(c):
    import drtk_amd
    import test_gpu_image_loss as T
    from drtk_amd import capi

    dtype = th.float32 if c["dtype"] == "f32" else th.float64
    shape, k, dr = (c["N"], c["C"], c["H"], c["W"]), c["k"], c["data_range"]
    kw = dict(window_size=k, sigma=c["sigma"], data_range=dr, padding=c["padding"])
    cw = dict(window_size=k, sigma=c["sigma"], data_range=dr, valid=c["padding"] == "valid")
    # float32 values, so that both precisions and the oracle see the same numbers
    x32, y32 = O.make_images(shape, seed=c["seed"], dtype=th.float32, data_range=dr, device=DEV)
    gen = th.Generator().manual_seed(c["seed"])
    w = None
    if c["weight"] in ("bool_NHW", "bool_N1HW"):
        w = O.make_mask(shape, seed=c["seed"], device=DEV)
    elif c["weight"] == "float":
        w = th.rand(c["N"], c["H"], c["W"], generator=gen, dtype=th.float64).to(dtype).to(DEV)
    ref = T.reference(x32.double(), y32.double(), None if w is None else (w if w.dtype == th.bool else w.double()), kw, th.float64)
    form = None if dtype == th.float64 else T.reference(x32, y32, w, kw, th.float32, h=ref["h"])
    x, y = laid_out(x32.to(dtype), c["layout"], float("nan")), laid_out(y32.to(dtype), c["layout"], float("nan"))
    if w is not None:
        w = laid_out(w, c["layout"], True if w.dtype == th.bool else 1e3)
        w = w[:, None] if c["weight"] == "bool_N1HW" else w
    h = ref["h"].to(dtype)

    # the binding, then the Python API under autograd; `names`: what of the oracle's quantities this operator gives
    leaf = x.detach().requires_grad_(True)
    if c["op"] == "ssim_map":
        names = ("map", "grad_map")
        out, maps, scalars = capi.image_loss_forward(x, y, None, mode="map", with_maps=True, **cw)
        assert scalars is None
        grad = capi.image_loss_backward(x, y, None, maps, h, None, mode="map", **cw)
        py = drtk_amd.ssim(leaf, y, reduction="none", **kw)
        (py * h).sum().backward()
    else:
        mode = "ssim" if c["op"] == "ssim_mean" else "photometric"
        names = ("ssim", "grad_ssim") if mode == "ssim" else ("photo", "grad_photo")
        cm = dict(cw, mode=mode, l1_weight=T.L1W, ssim_weight=T.SSW)
        out, maps, scalars = capi.image_loss_forward(x, y, w, with_maps=True, **cm)
        assert bool(th.isfinite(scalars).all()), scalars
        grad = capi.image_loss_backward(x, y, w, maps, th.ones((), dtype=dtype, device=DEV), scalars, **cm)
        py = drtk_amd.ssim(leaf, y, w, **kw) if mode == "ssim" else drtk_amd.photometric_loss(leaf, y, w, T.L1W, T.SSW, **kw)
        py.backward()
        no_maps = capi.image_loss_forward(x, y, w, **cm)  # the no-grad call: no maps, the same scalars
        assert no_maps[1] is None and th.equal(no_maps[0], out) and th.equal(no_maps[2], scalars)
    assert bool(th.isfinite(maps).all()), "a gradient map was left unwritten"
    got = {names[0]: out, names[1]: grad}
    assert th.equal(py.detach(), out) and th.equal(leaf.grad, grad), "the Python API and the C ABI binding differ"
    if dtype == th.float64:
        for name in names:
            assert got[name].shape == ref[name].shape, name
            e, top = T.err(got[name], ref[name]), max(1.0, float(ref[name].abs().max()))
            assert e <= 1e-12 * top, (name, e, top)
    else:
        eps, map_bar = th.finfo(th.float32).eps, T.err(form["map"], ref["map"])
        bound = {"ssim": 4 * map_bar, "photo": T.SSW * 4 * map_bar + T.L1W * 4 * eps * dr}
        for name in names:
            assert got[name].shape == ref[name].shape, name
            e, tol = T.err(got[name], ref[name]), bound[name] if name in bound else 4 * T.err(form[name], ref[name])
            assert e <= tol, (name, e, tol)


def run_mipmap_pyramid(c):
    import test_gpu_mipmap_pyramid as T
    from drtk_amd import capi

    dtype = th.float32 if c["dtype"] == "f32" else th.float64
    shape, L = (c["N"], c["C"], c["H"], c["W"]), c["levels"]
    gen = th.Generator().manual_seed(c["seed"])
    x = (th.rand(shape, generator=gen, dtype=th.float64) * 2 - 1).to(dtype).to(DEV)
    want = T.definition(x, L)
    grads = [None if l in c["absent"] else (th.rand(t.shape, generator=gen, dtype=th.float64) * 6 - 3).to(dtype).to(DEV) for l, t in enumerate(want)]
    want_grad = T.recurrence(grads, x)
    if c["layout"] == "one_element_in":
        x = one_element_in(x)
    out = capi.mipmap_pyramid(x, L)
    assert out[0] is x and len(out) == L
    for l, (a, b) in enumerate(zip(out, want)):
        assert a.shape == b.shape and th.equal(a, b), f"C ABI, level {l}"
    # without a gradient of level 0 the binding is told H and W by grad_input: one of its own allocations, as it would make
    grad_input = capi._out(*shape, dtype=dtype, device=DEV) if grads[0] is None else None
    assert th.equal(capi.mipmap_pyramid_backward(grads, grad_input=grad_input), want_grad), "C ABI, grad_input"
    out, grad = T.run_autograd(x, L, grads)
    for l, (a, b) in enumerate(zip(out, want)):
        assert a.shape == b.shape and th.equal(a, b), f"level {l}"
    assert th.equal(grad, want_grad), "grad_input"


def run_case(c, check_guards=True):
    from drtk_amd import capi

    (run_mipmap_pyramid if c["op"] == "mipmap_pyramid" else run_image_loss)(c)
    if check_guards:  # DRTK_CAPI_GUARD=g: nothing was written outside an output or a workspace (no-op otherwise)
        capi.check_guards()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--first", type=int, default=0)
    a = ap.parse_args()
    bad, t0 = 0, time.time()
    for seed in range(a.first, a.first + a.cases):
        c = make_case(seed)
        try:
            run_case(c)
        except AssertionError as e:
            bad += 1
            print(f"FAIL {describe(c)}: {str(e)[:600]}", flush=True)
        except Exception as e:  # an error of the runtime or the library: nothing more is started on the device
            print(f"ERROR {describe(c)}: {type(e).__name__}: {str(e)[:600]}\nstopped after seed {seed}", flush=True)
            sys.exit(2)
    print(f"{time.time() - t0:.1f} s")
    print(f"{a.cases - bad}/{a.cases} cases passed")
    sys.exit(1 if bad else 0)
