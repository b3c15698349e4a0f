"""The cases of tests/edge_chain_cases.py are what tests/test_gpu_edge_chain.py relies on -- the shapes, the padding around the
views, the pair counts around the classification's round grouping, the strip that owes one pair -- decided on the CPU with
the oracle and plain tensor arithmetic (no GPU)."""
import pytest
import torch as th

import edge_chain_cases as K
import edge_prune_cases as P


def test_shapes_cover_the_issue():
    s = K.shapes()
    assert {w for w, _, _ in s} == {1, 2, 3, 5, 6, 254, 506} and {h for _, h, _ in s} == {1, 2, 3, 9}
    assert len(s) == 28 and len(set(s)) == 28
    for W in K.WIDTHS:
        assert {c for w, _, c in s if w == W} == {1, 3, 16}
    for H in K.HEIGHTS:
        assert {c for _, h, c in s if h == H} == {1, 3, 16}
    assert any(W % 4 == 2 for W in K.WIDTHS) and any(W < 4 for W in K.WIDTHS)


@pytest.mark.parametrize("W,H,C", K.shapes())
def test_shape_cases_have_a_gradient_where_pairs_exist(W, H, C):
    import oracle as O

    v, vi, idx, bary, img, go = K.shape_case(W, H, C)
    assert idx.shape == (K.VIEWS, H, W) and K.VIEWS == 3 and img.shape[1] == C
    out = O.edge_grad_backward(v, img, idx, vi, go)
    assert bool(out.any()) == K.shape_has_pairs(W, H)
    if K.shape_has_pairs(W, H):
        assert float(K._strip_pairs(idx).sum()) > 0


@pytest.mark.parametrize("dtype", [th.float32, th.int32])
@pytest.mark.parametrize("W", K.WIDTHS)
def test_views_are_padded_by_a_row_and_start_past_a_boundary(W, dtype):
    t = (th.arange(3 * 2 * 9 * W).reshape(3, 2, 9, W) + 1).to(dtype)
    view, flat, off = K.embed(t, W)
    assert view.is_contiguous() and th.equal(view, t)
    assert view.data_ptr() - flat.data_ptr() == off * t.element_size() and (off * t.element_size()) % 16 == t.element_size()
    front, back = flat[:off], flat[off + t.numel():]
    assert front.numel() >= W and back.numel() >= W, "a full row on both sides"
    if dtype == th.float32:
        assert bool(th.isnan(front).all()) and bool(th.isnan(back).all())
    else:
        assert bool((front == 0).all()) and bool((back == 0).all()), "the valid triangle id 0"


def test_pair_counts_occur_with_needed_pairs_in_the_first_and_the_last_round():
    v, vi, idx, bary, img, go = K.pair_counts_case()
    pairs = K._strip_pairs(idx)  # [N, bands, strips]
    assert set(K.PAIR_COUNTS) >= {1, 63, 64, 65, 64 * K.ROUNDS - 1, 64 * K.ROUNDS, 64 * K.ROUNDS + 1, 1008}
    for n, count in enumerate(K.PAIR_COUNTS):
        assert float(pairs[n, 0, 0]) == count and float(pairs[n].sum()) == count, f"view {n}: one strip with {count} pairs"
        listed = K.listed_pairs(idx[n])
        assert len(listed) == count
        needed = [int(idx[n, ya, xa]) < 0 or int(idx[n, yb, xb]) < 0 for xa, ya, xb, yb in listed]  # a background pixel: eval_pair uses the term
        last_round = 64 * ((count - 1) // 64)
        assert any(needed[:64]), f"view {n}: a needed pair in the first round"
        assert any(needed[last_round:]), f"view {n}: a needed pair in the last round"
    assert int(idx.max()) < vi.shape[0] and int(idx.min()) == -1


def test_the_mixed_strip_owes_exactly_one_pair():
    case = K.mixed_strip_case()
    c = P.conditions(case)
    idx = case[2]
    hx, hy = K.MIXED_HOLE
    assert (hx, hy) == (62 * 4 + 3, K.STRIP_H) and int(idx[0, hy, hx]) == -1 and int((idx == -1).sum()) == 1
    listed = K.listed_pairs(idx[0])  # the pairs of the strip at the origin
    assert len(listed) > 1, "seams beside the one pair"
    assert listed[-1] == (hx, hy - 1, hx, hy), "the vertical pair into the halo row at lane 62's fourth pixel"
    assert all(int(idx[0, ya, xa]) >= 0 and int(idx[0, yb, xb]) >= 0 for xa, ya, xb, yb in listed[:-1])
    # the oracle: of the pixels of that strip's pairs, only the pixel above the hole receives anything, and only along y
    nz = c["nonzero"][0]
    rows = nz[:K.STRIP_H, :K.STRIP_W + 1]
    assert int(rows.sum()) == 1 and bool(rows[hy - 1, hx])
    out = c["out"][0, :, hy - 1, hx]
    assert float(out[0]) == 0 and float(out[1]) != 0
