"""Cases for the batched loads of the one-pass fused edge backward (edge_dots_kernel, SCATTER, drtk_amd/csrc/edge_grad.hip): the
kernel issues the loads of each of its phases together, without a branch around any of them -- the quads of the index rows,
the row loads of a channel, the ids, faces and vertices of ROUNDS x 64 pairs of the classification -- so a load may be issued
for an element that does not exist, and what it returns must never be used.

Builders return the tuple (v, vi, idx, bary, img, go) of tests/test_gpu_edge_onepass.py's `_check`.  What a case must
satisfy is asserted on the CPU by tests/test_edge_chain_cases_host.py; tests/test_gpu_edge_chain.py runs the kernel on them."""
import functools
import math
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_edge_onepass import STRIP_H, STRIP_W, _case, _mesh, _strip_pairs  # noqa: E402,F401  (the strip geometry of the kernel, not restated)

ROUNDS = 2  # kClassifyRounds of edge_grad.hip: rounds of 64 pairs the classification keeps in flight
WIDTHS = (1, 2, 3, 5, 6, 254, 506)  # W % 4 = 2, W < 4, and the same past one and two strips
HEIGHTS = (1, 2, 3, 9)
CHANNELS = (1, 3, 16)
VIEWS = 3


def shapes():
    """Every width with every height; the channel counts rotate so that each occurs with every width and every height."""
    return [(W, H, CHANNELS[(i + j) % 3]) for i, W in enumerate(WIDTHS) for j, H in enumerate(HEIGHTS)]


@functools.lru_cache(maxsize=None)
def shape_case(W, H, C):
    """Blocks of 3 x 2 pixels of one id; where the image is narrower than two blocks, diagonals of background and two triangles
    (every pair differs, and a pair with a background pixel always has its term used)."""
    return _case("blocks", VIEWS, H, W, C, 40) if W >= 4 else _case("three", VIEWS, H, W, C, 2)


def shape_has_pairs(W, H):
    """The reference's stencil domain (x < W-1, y < H-1) is not empty."""
    return W > 1 and H > 1


# ---- views inside a larger buffer
def embed(t, row):
    """`t` as a contiguous view into a larger flat buffer (same device), one element past a 16-byte boundary of it, with at
    least `row` elements before and after: NaN for floats, the valid triangle id 0 for the index (an invalid id there could
    send a gather of a kernel that used it out of range).  Returns (view, buffer, offset)."""
    front = 4 * math.ceil(max(row, 1) / 4) + 1
    back = max(row, 1) + 3
    flat = th.full((front + t.numel() + back,), float("nan") if t.is_floating_point() else 0, dtype=t.dtype, device=t.device)
    flat[front:front + t.numel()] = t.reshape(-1)
    return flat[front:front + t.numel()].view(t.shape), flat, front


# ---- pair counts around the round grouping
PAIR_W, PAIR_H = STRIP_W + 1, STRIP_H + 1  # one strip with pairs: the second strip's only pixel and the last row own none
ALL_PAIRS = 2 * STRIP_W * STRIP_H  # 1008: every pair of the strip, both axes
PAIR_COUNTS = (1, 63, 64, 65, 64 * ROUNDS - 1, 64 * ROUNDS, 64 * ROUNDS + 1, 191, 192, 193, ALL_PAIRS)


def _pair_image(K, F, g):
    """[PAIR_H, PAIR_W] ids with exactly K differing pairs in the strip: rows 0 and 1 share a pattern of K // 2 changes
    (K // 2 horizontal pairs each, no vertical pair between them), the halo row repeats it but for one pixel if K is odd.
    The first and the last run of the pattern are background, and so is the odd pixel: the first and the last pair of the
    kernel's list (horizontal pairs row-major, then vertical ones) have a background pixel -- their term is used."""
    if K == ALL_PAIRS:  # background / triangle 0 checker: every pair differs and every pair has a background pixel
        y, x = th.meshgrid(th.arange(PAIR_H), th.arange(PAIR_W), indexing="ij")
        return ((x + y) % 2 - 1).int()
    h, odd = K // 2, K % 2
    assert h <= STRIP_W
    cuts = th.sort(th.randperm(STRIP_W, generator=g)[:h]).values  # a change between pixels x and x + 1, x <= 251
    run = th.zeros(PAIR_W, dtype=th.long)
    run[cuts + 1] = 1
    run = run.cumsum(0)  # run number of every pixel, 0 .. h
    ids = th.randint(0, F, (h + 1,), generator=g)
    for r in range(1, h + 1):  # neighbouring runs differ
        if ids[r] == ids[r - 1]:
            ids[r] = (ids[r] + 1) % F
    if h >= 1:
        ids[0] = -1
    if h >= 2:
        ids[h] = -1  # (run h - 1 >= 1 is a triangle)
    row = ids[run]
    img = row[None].repeat(PAIR_H, 1)
    if odd:
        xv = int(th.randint(0, STRIP_W, (1,), generator=g))
        while int(row[xv]) == -1:
            xv = (xv + 1) % STRIP_W
        img[PAIR_H - 1, xv] = -1
    return img.int()


@functools.lru_cache(maxsize=None)
def pair_counts_case(C=3, F=40):
    """One view per count of PAIR_COUNTS."""
    g = th.Generator().manual_seed(97)
    N = len(PAIR_COUNTS)
    idx = th.stack([_pair_image(K, F, g) for K in PAIR_COUNTS]).contiguous()
    v1, vi = _mesh(F, PAIR_H, PAIR_W, g)
    v = (v1[None] + 0.25 * th.rand(N, *v1.shape, generator=g)).contiguous()
    bary = th.rand(N, 3, PAIR_H, PAIR_W, generator=g) + 0.05
    bary = (bary / bary.sum(1, keepdim=True)).contiguous()
    img = th.rand(N, C, PAIR_H, PAIR_W, generator=g) * (idx != -1)[:, None]
    go = th.rand(N, C, PAIR_H, PAIR_W, generator=g) * 2 - 1
    return v, vi, idx, bary, img, go


def listed_pairs(idx_view):
    """The differing pairs of the strip at the origin of one view, in the order of the kernel's list: horizontal pairs
    row-major, then vertical pairs row-major.  Rows of (xa, ya, xb, yb)."""
    H, W = idx_view.shape
    out = []
    for axis in (0, 1):
        for y in range(min(STRIP_H, H - 1)):
            for x in range(min(STRIP_W, W - 1)):
                xb, yb = (x + 1, y) if axis == 0 else (x, y + 1)
                if int(idx_view[y, x]) != int(idx_view[yb, xb]):
                    out.append((x, y, xb, yb))
    return out


# ---- a strip that owes one pair
MIXED_H, MIXED_W = 9, 505
MIXED_HOLE = (STRIP_W - 1, STRIP_H)  # lane 62's fourth pixel, in the halo row of the first wave


@functools.lru_cache(maxsize=None)
def mixed_strip_case():
    """The two-triangle quad of tests/edge_prune_cases.py -- the pairs along its diagonal are seams -- with one background pixel
    in the halo row of the strip at the origin, under lane 62's fourth pixel: of the pairs that strip owns, the vertical one
    that ends in the hole is the only one whose term is used."""
    import edge_prune_cases as P

    holes = th.zeros(1, MIXED_H, MIXED_W, dtype=th.bool)
    holes[0, MIXED_HOLE[1], MIXED_HOLE[0]] = True
    v, vi = P._quad(1, MIXED_H, MIXED_W)
    return P._finish(v, vi, MIXED_H, MIXED_W, 3, 15, holes)
