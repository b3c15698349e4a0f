"""-m gpu: which kernel instantiation every call of the rasterizer launches (drtk_amd/csrc/rasterize.hip: raster_route,
launch_raster) -- the FULL name with every template argument and the launch counts, from the kernel timing report: the plain
kernel's <T, TILE_SHIFT, FM> for `rasterize` and for `rasterize_layers` with one layer, the layer kernel's
<T, TILE_SHIFT, FM, MODE> (MODE 1: layer 0, MODE 2: every later layer) for more, and the three binning kernels once per call.

The smallest scene at which the rule can differ: an 8 x 8 canvas (one tile per view), so the tile size turns on the batch alone --
2047 views: 32-pixel tiles, 2048 views: 64-pixel tiles (make_layout: t64 >= 2048).  Six triangles shared by all views
(vi_sN == 0), each at its own constant depth, 0.5 apart: one fills the screen, one faces backwards, one is culled at z <= 0.  Four
vertex sets repeat over the batch, so the CPU oracle runs on four views.  Every result is checked against the oracle, so that a
kernel cannot pass by name: the index in both depth orders (depths 0.5 apart: the owner cannot change), the depth bits under
"strict", the depth within 2e-6 relative under "fastmath" -- the rounding budget of the kernel's own bound, z_lower_bound_bits.

T stays T in the names: the element type is the call's."""
import functools

import numpy as np
import pytest
import torch as th
from test_gpu_rasterize_layers import DEV, depth_order

import layers_oracle as LO

pytestmark = pytest.mark.gpu

H = W = 8
K = 3
DTYPES = [th.float32, th.float64]
BATCHES = {2047: 5, 2048: 6}  # views -> TILE_SHIFT
FM_REL = 2e-6


@functools.lru_cache(maxsize=None)
def scene(dtype):
    """(v [4,18,3], vi [6,3]) and the oracle's answers on the four views: rasterize (depth, index) and the K layers."""
    import oracle as O

    rng = np.random.default_rng(1400)
    z = [2.5, 0.5, 1.0, 1.5, 2.0, 0.0]  # the screen-filling one is the farthest; the last is culled (z <= 0)
    v = np.zeros((4, 18, 3))
    for s in range(4):
        tris = [np.array([[-20.0, -20.0], [40.0, -20.0], [-20.0, 40.0]])]  # covers every pixel centre of the canvas
        for _ in range(5):
            c = rng.uniform(1.0, 6.0, size=2)
            tris.append(c + rng.uniform(-4.0, 4.0, size=(3, 2)))
        for f, t in enumerate(tris):
            den = (t[1, 0] - t[0, 0]) * (t[2, 1] - t[0, 1]) - (t[1, 1] - t[0, 1]) * (t[2, 0] - t[0, 0])
            if (den > 0) == (f == 4):  # triangle 4 alone has the other orientation
                t = t[[0, 2, 1]]
            v[s, 3 * f:3 * f + 3, :2] = t
            v[s, 3 * f:3 * f + 3, 2] = z[f]
    v = th.from_numpy(v).to(dtype)
    vi = th.arange(18, dtype=th.int32).reshape(6, 3)
    d, i = O.rasterize(v, vi, H, W)
    ld, li = LO.layers(v, vi, H, W, K)
    return v, vi, (d, i), (th.from_numpy(ld), th.from_numpy(li))


def test_the_scene_is_what_the_docstring_says():
    for dtype in DTYPES:
        v, vi, (d, i), (ld, li) = scene(dtype)
        assert int((i < 0).sum()) == 0 and int((li[:, 0] < 0).sum()) == 0  # triangle 0 fills the screen
        assert not bool((li == 5).any())  # the culled one is nowhere
        for f in range(5):
            assert bool((li == f).any()), f  # every other one has a fragment, the back-facing one included
        assert th.equal(li[:, 0], i) and th.equal(ld[:, 0].view(th.int32), d.view(th.int32))
        counts = (li >= 0).sum(dim=1)
        assert int(counts.min()) == 1 and int(counts.max()) == K  # pixels with fewer fragments than layers, and with all of them
        assert bool((ld[li < 0] == 0).all())
        assert len({tuple(v[s].flatten().tolist()) for s in range(4)}) == 4


def launched(fn):
    """fn() and {full name: launches} of the rasterizer's kernels it launched."""
    from drtk_amd import capi

    capi.kernel_timing_begin()
    out = fn()
    th.cuda.synchronize()
    return out, {k: n[0] for k, n in capi.kernel_timing_report().items() if k.startswith(("bin_", "tile_raster"))}


BINS = {"bin_count_kernel<T>": 1, "bin_scan_kernel": 1, "bin_fill_kernel": 1}


def expected_launches(call, shift, fm):
    flag = "true" if fm else "false"
    if call in ("rasterize", "layers1"):
        return dict(BINS, **{f"tile_raster_kernel<T, {shift}, {flag}>": 1})
    return dict(BINS, **{f"tile_raster_layer_kernel<T, {shift}, {flag}, 1>": 1, f"tile_raster_layer_kernel<T, {shift}, {flag}, 2>": K - 1})


def check(got, want, order, what):
    """got: [N,...] on the device; want: the four views' answer, repeated over the batch."""
    (gd, gi), (wd, wi) = got, want
    sel = th.arange(gd.shape[0], device=DEV) % 4
    wd, wi = wd.to(DEV)[sel], wi.to(DEV)[sel]
    assert gi.shape == wi.shape and gi.dtype == th.int32 and gd.dtype == th.float32, what
    assert th.equal(gi, wi), f"{what}: index differs in {int((gi != wi).sum())} pixels"
    if order == "strict":
        assert th.equal(gd.view(th.int32), wd.view(th.int32)), f"{what}: depth bits differ in {int((gd.view(th.int32) != wd.view(th.int32)).sum())} pixels"
    else:
        rel = ((gd - wd).abs() / wd.abs().clamp_min(1e-30)).max().item()
        print(f"{what}: largest relative depth difference {rel:.3e}")
        assert bool(((gd - wd).abs() <= FM_REL * wd.abs()).all()), (what, rel)  # (0.0 where there is no fragment: exact)
    assert bool((gd[gi < 0] == 0).all()), what


@pytest.mark.parametrize("N", list(BATCHES))
@pytest.mark.parametrize("order", ["strict", "fastmath"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_raster_instantiations(dtype, order, N):
    from drtk_amd import capi

    v4, vi, flat, layered = scene(dtype)
    v = v4.to(DEV)[th.arange(N, device=DEV) % 4].contiguous()
    vi = vi.to(DEV)
    shift, fm = BATCHES[N], order == "fastmath"
    with depth_order(order):
        for call in ("rasterize", "layers1", "layers"):
            what = f"{call} N={N} {order} {dtype}"
            if call == "rasterize":
                got, names = launched(lambda: capi.rasterize(v, vi, H, W))
                want = flat
            else:
                k = 1 if call == "layers1" else K
                got, names = launched(lambda: capi.rasterize_layers(v, vi, H, W, k))
                want = (layered[0][:, :k], layered[1][:, :k])
                if k == 1:
                    assert th.equal(want[1][:, 0], flat[1])
                else:
                    assert int((got[1][:, 1:] < 0).sum()) > 0  # pixels with fewer fragments than layers: -1 / 0.0 (checked below)
            print(f"{what}: {names}")
            assert names == expected_launches(call, shift, fm), what
            check(got, want, order, what)
