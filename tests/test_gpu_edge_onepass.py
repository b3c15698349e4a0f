"""-m gpu: the one-pass fused edge backward (edge_dots_kernel in SCATTER mode, drtk_amd/csrc/edge_grad.hip) on the smallest
shapes at which it can go wrong, every case through capi.edge_grad_backward_fused in float32 and held to the per-element
bound of tests/test_gpu_f64_distance.py's "fused edge_grad route" (its own ELEMENT_ULPS["edge"] and FLOOR) against the CPU
oracle in float32 and float64.

A wave of that kernel owns the pairs of a strip of 252 pixels x 2 rows (63 lanes x 4 pixels, lane 63 = halo), a workgroup
8 rows; a strip with at most LIST_CAP differing pairs compacts them into a list, a denser one keeps them per lane.  The
library takes the one-pass kernel by itself only for calls of a megapixel and more, so DRTK_AMD_EDGE_ONEPASS=1 (read per
call) sends these small images through it; one test checks from the kernel timing report that it did."""
import os
import sys

import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_f64_distance import ELEMENT_ULPS, FLOOR  # noqa: E402  (the bound of the route, not restated)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRIP_W, STRIP_H = 252, 2  # pixels of a wave's strip
LIST_CAP = 512             # kOnepassCap: pairs a strip's list holds


@pytest.fixture(autouse=True)
def _one_pass(monkeypatch):
    monkeypatch.setenv("DRTK_AMD_EDGE_ONEPASS", "1")


def _mesh(F, H, W, g):
    """F triangles over max(F, 8) shared vertices scattered over twice the image's extent, so that many of them contain the
    pixels that carry their id and their neighbours (any index image is a valid input)."""
    V = max(F, 8)
    v = th.stack([(th.rand(V, generator=g) * 2 - 0.5) * W, (th.rand(V, generator=g) * 2 - 0.5) * (H + 4), th.rand(V, generator=g) * 1.5 + 0.5], -1)
    vi = th.stack([th.randperm(V, generator=g)[:3] for _ in range(F)]).int()
    return v, vi


def _index(pattern, N, H, W, F, g):
    y, x = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    if pattern == "checker":    # every pair differs: 2 pairs per interior pixel, the worst case
        idx = ((x + y) % 2)[None].expand(N, -1, -1)
    elif pattern == "three":    # every pair differs, a third of the pixels background
        idx = ((x + y) % 3 - 1)[None].expand(N, -1, -1)
    elif pattern == "random":   # per-pixel ids in [-1, F)
        idx = th.randint(-1, F, (N, H, W), generator=g)
    else:                       # "blocks": 3 x 2 blocks of one id, a quarter of them background: runs along the rows, under a pair per pixel
        ids = th.randint(0, F, (N, (H + 1) // 2, (W + 2) // 3), generator=g)
        ids[th.rand(ids.shape, generator=g) < 0.25] = -1
        idx = ids[:, y // 2, x // 3]
    return idx.int().contiguous()


def _case(pattern, N, H, W, C, F, seed=0):
    g = th.Generator().manual_seed(1000 * seed + 7 * H + W + C)
    v1, vi = _mesh(F, H, W, g)
    v = (v1[None] + 0.25 * th.rand(N, *v1.shape, generator=g)).contiguous()
    idx = _index(pattern, N, H, W, F, g)
    bary = th.rand(N, 3, H, W, generator=g) + 0.05
    bary = (bary / bary.sum(1, keepdim=True)).contiguous()
    img = th.rand(N, C, H, W, generator=g) * (idx != -1)[:, None]
    go = th.rand(N, C, H, W, generator=g) * 2 - 1
    return v, vi, idx, bary, img, go


def _strip_pairs(idx):
    """Differing pairs of every wave's strip, inside the reference's stencil domain (x < W-1, y < H-1): [N, bands, strips]."""
    N, H, W = idx.shape
    cnt = th.zeros(N, H, W)
    if H > 1 and W > 1:
        cnt[:, :-1, :-1] = (idx[:, :-1, :-1] != idx[:, :-1, 1:]).float() + (idx[:, :-1, :-1] != idx[:, 1:, :-1]).float()
    return th.nn.functional.avg_pool2d(cnt[:, None], (STRIP_H, STRIP_W), ceil_mode=True, divisor_override=1)[:, 0]


def _check(v, vi, idx, bary, img, go, what, nonzero=True):
    import oracle as O
    from drtk_amd import capi
    from f64_distance import assert_elementwise_within as within

    v6, img6, go6, bary6 = v.double(), img.double(), go.double(), bary.double()
    out = {}
    for M in (1e4, 0.5):
        e32, e64 = O.edge_grad_backward(v, img, idx, vi, go, M), O.edge_grad_backward(v6, img6, idx, vi, go6, M)
        with O.accumulated_magnitudes():
            eA = O.edge_grad_backward(v6, img6, idx, vi, go6, M)
        v32, _ = O.interpolate_backward(e32, v, vi, idx, bary, True, False)
        v64, _ = O.interpolate_backward(e64, v6, vi, idx, bary6, True, False)
        vA, _ = O.interpolate_backward(eA, v6, vi, idx, bary6.abs(), True, False)
        got = capi.edge_grad_backward_fused(v.to(DEV), img.to(DEV), idx.to(DEV), vi.to(DEV), bary.to(DEV), go.to(DEV), M)
        print(f"{what}, max_dp_dr={M}: max|f64| = {float(v64.abs().max()):.3e}, |kernel - f64| = {float((got.cpu().double() - v64).abs().max()):.3e}, "
              f"|oracle_f32 - f64| = {float((v32.double() - v64).abs().max()):.3e}")
        assert bool(th.isfinite(v64).all()) and (float(v64.abs().max()) > 0) == nonzero, f"{what}: the reference itself"
        within(got, v32, v64, vA, ELEMENT_ULPS["edge"], f"{what}, max_dp_dr={M}", floor_rel=FLOOR)
        out[M] = (got, v64)
    return out


@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("W", [251, 252, 253, 256, 505])
def test_strip_seam(W, C):
    """The pair of lane 62's last pixel with lane 63's first, and the first pixel of the second strip; lists, not the dense path."""
    case = _case("blocks", 2, 5, W, C, 40)
    pairs = _strip_pairs(case[2])
    assert 0 < float(pairs.max()) <= LIST_CAP
    _check(*case, f"strip seam W={W} C={C}")


@pytest.mark.parametrize("W", [7, 300])
@pytest.mark.parametrize("H", [1, 2, 3, 8, 9, 17])
def test_band_seam_and_image_border(H, W):
    """A wave covers 2 rows, a workgroup 8: the halo row of a wave, of a workgroup, and the last row of the image."""
    from drtk_amd import capi

    case = _case("blocks", 2, H, W, 5, 40)
    out = _check(*case, f"band seam H={H} W={W}", nonzero=H > 1)
    if H == 1:  # no pair exists: exactly zero, written over the poisoned output
        assert capi._POISON, "conftest.py sets DRTK_CAPI_POISON before drtk_amd.capi is imported"
        for got, _ in out.values():
            assert bool((got == 0).all())


@pytest.mark.parametrize("shape", [(9, 505), (3, 251)])
@pytest.mark.parametrize("pattern,F", [("checker", 2), ("three", 2), ("random", 4), ("random", 300)])
def test_maximum_pair_density(pattern, F, shape):
    """Index images that differ at (nearly) every pixel: more pairs than any list shorter than the worst case holds."""
    H, W = shape
    case = _case(pattern, 2, H, W, 3, F)
    pairs = _strip_pairs(case[2])
    assert float(pairs.max()) > LIST_CAP
    if pattern == "checker" and shape == (9, 505):
        assert float(pairs.max()) == 2.0 * STRIP_W * STRIP_H  # the densest strip: 2 pairs per pixel
    out = _check(*case, f"density {pattern} F={F} {H}x{W}")
    for got, _ in out.values():
        assert bool(th.isfinite(got).all())


def _sphere():
    import oracle as O
    from drtk_amd import synthetic as S

    H, W, C = 24, 253, 16
    v, vi = S.sphere_views(2, 70, 72, H, W)
    _, idx = O.rasterize(v, vi, H, W, nthreads=0)
    _, bary = O.render(v, vi, idx, nthreads=0)
    g = th.Generator().manual_seed(11)
    attr = th.rand(2, v.shape[1], C, generator=g)
    img = O.interpolate(attr, vi, idx, bary, nthreads=0) * (idx != -1)[:, None]
    go = th.rand(2, C, H, W, generator=g) * 2 - 1
    return v, vi, idx, bary, img, go


def test_rendered_scene_with_subpixel_triangles():
    """10 080 triangles on 24 x 253 pixels: nearly every pair differs and many vertices are hit."""
    _check(*_sphere(), "sphere_views(2, 70, 72, 24, 253)")


def test_two_calls_agree():
    """The same inputs twice: atomics order only."""
    from drtk_amd import capi

    args = [t.to(DEV) for t in _sphere()]
    v, vi, idx, bary, img, go = args
    a = capi.edge_grad_backward_fused(v, img, idx, vi, bary, go)
    b = capi.edge_grad_backward_fused(v, img, idx, vi, bary, go)
    th.testing.assert_close(a, b, atol=1e-7, rtol=1e-5)


def test_the_switch_selects_the_kernels(monkeypatch):
    """What this file tests is the one-pass kernel: with the switch on, a float call launches edge_dots_kernel alone (and the
    fill); with it off, and for double, the two kernels."""
    from drtk_amd import capi

    v, vi, idx, bary, img, go = (t.to(DEV) for t in _case("blocks", 2, 9, 300, 3, 40))

    def launched(dtype, switch):
        monkeypatch.setenv("DRTK_AMD_EDGE_ONEPASS", switch)
        f = [t.to(dtype) for t in (v, img, bary, go)]
        capi.kernel_timing_begin()
        capi.edge_grad_backward_fused(f[0], f[1], idx, vi, f[2], f[3])
        th.cuda.synchronize()
        return {k.strip("()").split("<")[0] for k in capi.kernel_timing_report()}

    assert launched(th.float32, "1") == {"fill_bytes_kernel", "edge_dots_kernel"}
    assert launched(th.float32, "0") == {"edge_dots_kernel", "edge_scatter_pairs_kernel"}
    assert launched(th.float64, "1") == {"edge_dots_kernel", "edge_scatter_pairs_kernel"}
