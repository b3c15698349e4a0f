"""Scenes for the classification phase of the one-pass fused edge backward (edge_dots_kernel, SCATTER, drtk_amd/csrc/edge_grad.hip):
the kernel classifies its differing pixel pairs before it loads an image and streams only where a pair's term is used -- a
pair of two foreground pixels of which neither lies inside the other's triangle (a seam between neighbouring triangles of one
surface) is skipped, as the reference selects 0 for it.  Every scene here is dominated by such seams.

Builders return the tuple (v, vi, idx, bary, img, go) of tests/test_gpu_edge_onepass.py's `_check`; `conditions` derives what
a scene must satisfy from the CPU oracle -- a pixel that takes part in a differing pair is PRUNED if the oracle's output for it
is exactly zero -- never from a restated classifier.  tests/test_edge_prune_cases_host.py asserts the conditions without a GPU,
tests/test_gpu_edge_prune.py repeats them next to the kernel's checks."""
import functools
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_edge_onepass import LIST_CAP, _strip_pairs  # noqa: E402,F401  (the strip geometry of the kernel, not restated)

RENDERED = [(40, 0.0, 16), (24, 0.05, 3), (40, 0.0, 3), (24, 0.05, 16)]  # (n_lat = n_lon, lobes, C) of the two-sphere scene
HOLE_XS = (0, 3, 4, 247, 248, 250, 251, 252, 253, 255, 256, 503, 504)   # lane ends, the lane 62/63 hand-over, the strip seam, the border
HOLE_YS = (0, 1, 2, 3, 7, 8)                                             # a wave's halo row, a workgroup's, the last rows
QUAD_H, QUAD_W = 9, 505
SHEETS = [(9, 505), (5, 253)]


def _finish(v, vi, H, W, C, seed, holes=None):
    """Rasterized by the oracle, `holes` [N,H,W] bool set to background afterwards; random vertex attributes interpolated
    into img (zero on the background), random grad_output."""
    import oracle as O

    N = v.shape[0]
    _, idx = O.rasterize(v, vi, H, W, nthreads=0)
    if holes is not None:
        idx = idx.clone()
        idx[holes] = -1
    _, bary = O.render(v, vi, idx, nthreads=0)
    g = th.Generator().manual_seed(seed)
    attr = th.rand(N, v.shape[1], C, generator=g)
    img = O.interpolate(attr, vi, idx, bary, nthreads=0) * (idx != -1)[:, None]
    go = th.rand(N, C, H, W, generator=g) * 2 - 1
    return v.contiguous(), vi.contiguous(), idx.contiguous(), bary.contiguous(), img.contiguous(), go.contiguous()


@functools.lru_cache(maxsize=None)
def rendered(n, lobes, C):
    """Case 1: two interpenetrating spheres on 33 x 505 pixels -- two strips and the seam, five bands, a last odd row; silhouettes,
    occlusion contours and intersections among seams; lists, not the dense path."""
    from drtk_amd import synthetic as S

    H, W = 33, 505
    v, vi = S.sphere_views(2, n, n, H, W, lobes=lobes, second_sphere=True)
    return _finish(v, vi, H, W, C, 11)


def _quad(N, H, W):
    v = th.tensor([[-50.0, -40.0, 1.0], [W + 60.0, -40.0, 1.0], [W + 60.0, H + 70.0, 1.0], [-50.0, H + 70.0, 1.0]])
    return v[None].repeat(N, 1, 1), th.tensor([[0, 1, 2], [0, 2, 3]], dtype=th.int32)


def hole_positions():
    return [(x, y) for y in HOLE_YS for x in HOLE_XS]


@functools.lru_cache(maxsize=None)
def quad_holes():
    """Case 2: a two-triangle quad over the whole image -- the pairs along its diagonal are all seams -- with ONE background
    pixel per view, so that each view has one to four needed pairs at a chosen place."""
    pos = hole_positions()
    holes = th.zeros(len(pos), QUAD_H, QUAD_W, dtype=th.bool)
    for n, (x, y) in enumerate(pos):
        holes[n, y, x] = True
    v, vi = _quad(len(pos), QUAD_H, QUAD_W)
    return _finish(v, vi, QUAD_H, QUAD_W, 3, 12, holes)


def hole_nonzero_pixels(x, y, H, W):
    """Pixels that receive something from a lone background pixel at (x, y): the foreground ends of its pairs inside the
    reference's stencil domain (centres with x < W-1 and y < H-1)."""
    own = x < W - 1 and y < H - 1
    return 2 * int(own) + int(x >= 1 and y < H - 1) + int(y >= 1 and x < W - 1)


@functools.lru_cache(maxsize=None)
def quad_plain():
    v, vi = _quad(1, QUAD_H, QUAD_W)
    return _finish(v, vi, QUAD_H, QUAD_W, 3, 13)


@functools.lru_cache(maxsize=None)
def sheet(H, W, holes=True):
    """Case 3: a sheet of one-pixel cells, two triangles each, grid lines at integer + (0.3, 0.2): every pixel has a triangle
    of its own, every pair differs and every pair is a seam; about 3 % of the pixels, seeded, set to background."""
    ys, xs = th.meshgrid(th.arange(-2, H + 2), th.arange(-2, W + 2), indexing="ij")
    v1 = th.stack([xs.flatten() + 0.3, ys.flatten() + 0.2, th.ones(xs.numel())], -1).float()
    nx = W + 4
    j, i = th.meshgrid(th.arange(H + 3), th.arange(W + 3), indexing="ij")
    a = (j * nx + i).flatten()
    vi = th.cat([th.stack([a, a + 1, a + nx + 1], -1), th.stack([a, a + nx + 1, a + nx], -1)]).int()
    g = th.Generator().manual_seed(5 * H + W)
    hole = th.rand(2, H, W, generator=g) < 0.03 if holes else None
    return _finish(v1[None].repeat(2, 1, 1), vi, H, W, 3, 14, hole)


def edge_pixels(idx):
    """Pixels that take part in a differing pair inside the reference's stencil domain: [N,H,W] bool."""
    e = th.zeros_like(idx, dtype=th.bool)
    hp = idx[:, :-1, :-1] != idx[:, :-1, 1:]
    vp = idx[:, :-1, :-1] != idx[:, 1:, :-1]
    e[:, :-1, :-1] |= hp | vp
    e[:, :-1, 1:] |= hp
    e[:, 1:, :-1] |= vp
    return e


def conditions(case):
    """From the CPU oracle on the case's own (generic random) img / grad_output."""
    import oracle as O

    v, vi, idx, bary, img, go = case
    out = O.edge_grad_backward(v, img, idx, vi, go)
    edge, nz = edge_pixels(idx), (out != 0).any(1)
    assert not bool((nz & ~edge).any()), "the oracle writes to edge pixels only"
    return {
        "out": out, "edge": edge, "nonzero": nz,
        "edge_pixels": int(edge.sum()), "nonzero_pixels": int(nz.sum()), "z_pixels": int((out[:, 2] != 0).sum()),
        "pruned": float((edge & ~nz).sum()) / max(int(edge.sum()), 1),
        "max_strip_pairs": float(_strip_pairs(idx).max()),
    }


def poisoned(case, cond, seed=3):
    """Case 4: img = NaN and grad_output = +Inf at a seeded 30 % of the edge pixels whose oracle output is zero on the pixel
    and on its four neighbours -- pixels of pairs whose term the reference discards with a select.  Returns (img, go, count)."""
    v, vi, idx, bary, img, go = case
    nz = cond["nonzero"]
    near = nz.clone()
    near[:, 1:] |= nz[:, :-1]
    near[:, :-1] |= nz[:, 1:]
    near[:, :, 1:] |= nz[:, :, :-1]
    near[:, :, :-1] |= nz[:, :, 1:]
    g = th.Generator().manual_seed(seed)
    sel = cond["edge"] & ~near & (th.rand(idx.shape, generator=g) < 0.3)
    m = sel[:, None].expand_as(img)
    return img.masked_fill(m, float("nan")), go.masked_fill(m, float("inf")), int(sel.sum())
