"""GPU (-m gpu): `rasterize_layers` on random triangle soups (tests/fuzz_layers.py: interpenetrating triangles, more
fragments per pixel than layers, long runs of exact depth ties, depths at and across the 1/eps cap, screen-filling
triangles between the soup's depths, a tile list long enough to be split, triangles that take the cooperative pass, the
64-pixel-tile kernels, float64 vertices, per-view topology) -- against the CPU oracle (tests/layers_oracle.py), against
itself with fewer layers, against a composition of plain `rasterize` calls under both depth orders, and across the two
tile sizes.  Every comparison is `th.equal` on the index and on the depth BITS of all 8 layers.

tests/test_rasterize_layers_host.py proves, from the oracle alone, that the cases deliver what these tests rely on."""
import numpy as np
import pytest
import torch as th

import fuzz_layers as FL
import layers_oracle as LO
from test_gpu_rasterize_layers import DEV, check_order, depth_order, routes, same

pytestmark = pytest.mark.gpu

K = FL.K
SOUPS = list(FL.CASES)


def want_of(name, views=None):
    """(case, (depth, index)) -- the first K layers of the oracle's, as tensors of their own"""
    c, wd, wi = FL.reference(name)
    wd, wi = FL.whole_batch(c, wd[:, :K], wi[:, :K])
    sel = slice(None) if views is None else views
    return c, (th.from_numpy(wd[sel].copy()), th.from_numpy(wi[sel].copy()))


def on_device(c):
    return c["v"].to(DEV), c["vi"].to(DEV)


def expect_same(got, want, c, what):
    """`same`, after a report that names the first differing layer, the pixel, both keys and the case"""
    diff = FL.first_difference(tuple(t.cpu().numpy() for t in got), tuple(t.cpu().numpy() for t in want), c)
    assert diff is None, f"{what}: {diff}"
    same(got, want, what)


# ---------------------------------------------------------------------------------------------------------------------
# a. the CPU oracle, strict depth order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [(n, "capi") for n in SOUPS] + [("free", "op"), ("cap64", "python")])
def test_soup_layers_are_bit_exact_against_the_cpu_oracle(name, route):
    c, want = want_of(name)
    v, vi = on_device(c)
    with depth_order("strict"):
        got = routes()[route](v, vi, c["H"], c["W"], K)
    expect_same(got, want, c, f"{name} through {route}")
    check_order(*got)


# ---------------------------------------------------------------------------------------------------------------------
# b. a prefix of the layers is the layers of a smaller K (k = 1: the plain kernel; k >= 2: another image stride)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOUPS)
def test_soup_layers_of_a_smaller_k_are_a_prefix(name):
    import drtk_amd
    from drtk_amd import capi

    c = FL.named_case(name)
    v, vi = on_device(c)
    d, i = capi.rasterize_layers(v, vi, c["H"], c["W"], K)
    assert all(int((i[n, 1] >= 0).sum()) > 0 for n in c["live"][:3])
    for k in (1, 2, 3, 5):
        dk, ik = capi.rasterize_layers(v, vi, c["H"], c["W"], k)
        expect_same((dk, ik), (d[:, :k].contiguous(), i[:, :k].contiguous()), c, f"{name}: K={k} against the first {k} of K={K}")
    d0, i0 = drtk_amd.rasterize_with_depth(v, vi, c["H"], c["W"])
    expect_same((d[:, :1].contiguous(), i[:, :1].contiguous()), (d0[:, None], i0[:, None]), c, f"{name}: layer 0 against rasterize_with_depth")


# ---------------------------------------------------------------------------------------------------------------------
# c. both depth orders: every triangle rasterized alone by plain `rasterize`, the keys sorted per pixel on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def compose(c):
    """the first K layers of the views that hold a soup, from one plain rasterize call with a view per (view, triangle).
    The lone triangle's indices are [0, 1, 2]: in the same (increasing) order as its own three in `vi`, so an evaluation
    that orders an edge's end points by vertex index sees the same order.  Only the fragments (a few per cent of views x
    triangles x pixels) leave the device; they are packed and sorted per pixel on the CPU."""
    import drtk_amd

    F, H, W, views = c["F"], c["H"], c["W"], c["live"]
    v, vi = on_device(c)
    assert bool((vi[..., 0] < vi[..., 1]).all()) and bool((vi[..., 1] < vi[..., 2]).all())
    sel = th.tensor(views, device=DEV)
    vi_sel = (vi[sel] if vi.ndim == 3 else vi[None].expand(len(views), -1, -1)).long()  # [n, F, 3]
    alone = v[sel][th.arange(len(views), device=DEV)[:, None, None], vi_sel]  # [n, F, 3 corners, 3]
    one = th.tensor([[0, 1, 2]], dtype=th.int32, device=DEV)
    depth, index = drtk_amd.rasterize_with_depth(alone.reshape(len(views) * F, 3, 3).contiguous(), one, H, W)
    assert bool(((index == 0) | ((index == -1) & (depth == 0))).all())
    hit = index.view(len(views), F, H * W) == 0
    view, tri, pixel = (a.cpu().numpy() for a in hit.nonzero(as_tuple=True))  # in row-major order, as hit's True elements
    keys = LO.pack_keys(depth.view(len(views), F, H * W)[hit].cpu().numpy(), tri.astype(np.int32))
    cell = view * (H * W) + pixel
    by_cell_then_key = np.lexsort((keys, cell))
    cell, keys = cell[by_cell_then_key], keys[by_cell_then_key]
    rank = np.arange(len(cell)) - np.searchsorted(cell, cell, side="left")  # of a fragment among its pixel's
    top = np.full((len(views) * H * W, K), LO.EMPTY, dtype=np.uint64)
    top[cell[rank < K], rank[rank < K]] = keys[rank < K]
    d, i = LO.unpack_keys(top.reshape(len(views), H, W, K).transpose(0, 3, 1, 2))
    return th.from_numpy(np.ascontiguousarray(d)), th.from_numpy(np.ascontiguousarray(i))


@pytest.mark.parametrize("order", ["strict", "fastmath"])
@pytest.mark.parametrize("name", SOUPS)
def test_soup_layers_equal_a_composition_of_plain_rasterize_under_both_depth_orders(name, order):
    import drtk_amd
    from drtk_amd import capi

    c = FL.named_case(name)
    views = c["live"]
    v, vi = on_device(c)
    before = drtk_amd.get_depth_order()
    with depth_order(order):
        assert drtk_amd.get_depth_order() == order
        want = compose(c)
        d, i = capi.rasterize_layers(v, vi, c["H"], c["W"], K)
    assert drtk_amd.get_depth_order() == before
    got = (d[views].contiguous(), i[views].contiguous())
    expect_same(got, want, c, f"{name} {order}: rasterize_layers against the composition")
    if len(views) < c["N"]:  # the other views hold nothing but culled triangles
        rest = th.ones(c["N"], dtype=th.bool, device=DEV)
        rest[views] = False
        assert bool((i[rest] == -1).all()) and bool((d[rest] == 0).all())
    if order == "strict":  # ... which ties the two oracles together
        expect_same(want, want_of(name, views)[1], c, f"{name}: the composition against the CPU oracle")


# ---------------------------------------------------------------------------------------------------------------------
# d. the two tile sizes: views of tiles64 alone (32-pixel tiles) against their slice of the batch (64-pixel tiles)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles64", "heavy64"])
def test_soup_views_alone_equal_their_slice_of_the_batch_that_takes_64_pixel_tiles(name):
    from drtk_amd import capi

    c = FL.named_case(name)
    N, H, W = c["N"], c["H"], c["W"]
    assert c["vi"].ndim == 2 and N * -(-W // 64) * -(-H // 64) >= 2048 > -(-W // 64) * -(-H // 64)
    v, vi = on_device(c)
    d, i = capi.rasterize_layers(v, vi, H, W, K)
    for n in sorted({0, 1, N - 1} | set(c["live"] if len(c["live"]) < N else ())):
        d1, i1 = capi.rasterize_layers(v[n:n + 1].contiguous(), vi, H, W, K)
        assert (int((i1[:, 2] >= 0).sum()) > 0) == (n in c["live"])
        expect_same((d[n:n + 1].contiguous(), i[n:n + 1].contiguous()), (d1, i1), c, f"view {n} of the batch against the view alone")


# ---------------------------------------------------------------------------------------------------------------------
# e. every element of all K planes is written, nothing outside them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOUPS)
def test_soup_layers_overwrite_every_poisoned_element(name):
    from drtk_amd import capi

    assert capi._POISON, "conftest.py sets DRTK_CAPI_POISON before drtk_amd.capi is imported"
    c = FL.named_case(name)
    v, vi = on_device(c)
    d, i = capi.rasterize_layers(v, vi, c["H"], c["W"], K)
    assert d.shape == (c["N"], K, c["H"], c["W"]) and i.shape == d.shape
    assert int(d.isnan().sum()) == 0, "a depth was left unwritten"
    assert int(((i < -1) | (i >= c["F"])).sum()) == 0, "an index was left unwritten or is no triangle's id"
    assert int(((i < 0) & (d != 0)).sum()) == 0 and int(((i >= 0) & ~(d > 0)).sum()) == 0
    capi.check_guards()  # with DRTK_CAPI_GUARD (the diagnostic run of the suite): the peel launches stayed inside their buffers
