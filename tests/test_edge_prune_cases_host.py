"""The scenes of tests/edge_prune_cases.py satisfy what tests/test_gpu_edge_prune.py relies on -- seam-dominated, with enough
pairs whose term IS used, at the places and densities named there -- decided by the CPU oracle alone (no GPU)."""
import pytest
import torch as th

import edge_prune_cases as P


@pytest.mark.parametrize("n,lobes,C", P.RENDERED)
def test_rendered_scenes_are_seam_dominated(n, lobes, C):
    c = P.conditions(P.rendered(n, lobes, C))
    print(f"rendered {n}x{n} lobes={lobes} C={C}: {c['edge_pixels']} edge pixels, {100 * c['pruned']:.1f} % pruned, "
          f"{c['nonzero_pixels']} non-zero ({c['z_pixels']} with z), at most {c['max_strip_pairs']:.0f} pairs per strip")
    assert c["pruned"] >= 0.90
    assert c["nonzero_pixels"] >= 40
    assert c["z_pixels"] > 0, "intersections"
    assert 0 < c["max_strip_pairs"] <= P.LIST_CAP, "the list path"


def test_quad_seams_are_pruned_and_each_hole_counts():
    plain = P.conditions(P.quad_plain())
    assert plain["edge_pixels"] > 0 and plain["nonzero_pixels"] == 0 and not bool(plain["out"].any())
    c = P.conditions(P.quad_holes())
    per_view = c["nonzero"].flatten(1).sum(1).tolist()
    want = [P.hole_nonzero_pixels(x, y, P.QUAD_H, P.QUAD_W) for x, y in P.hole_positions()]
    assert per_view == want
    assert max(want) == 4 and sum(w == 4 for w in want) >= 40  # the holes away from the border
    idx = P.quad_holes()[2]
    assert int((idx == -1).sum()) == len(want)


@pytest.mark.parametrize("H,W", P.SHEETS)
def test_sheets_are_dense_and_pruned(H, W):
    plain = P.conditions(P.sheet(H, W, holes=False))
    assert plain["max_strip_pairs"] > P.LIST_CAP and plain["pruned"] >= 0.90
    c = P.conditions(P.sheet(H, W))
    print(f"sheet {H}x{W}: {plain['max_strip_pairs']:.0f} pairs in the densest strip, {100 * plain['pruned']:.1f} % pruned without holes; "
          f"with holes {c['max_strip_pairs']:.0f} pairs, {c['nonzero_pixels']} non-zero pixels, {100 * c['pruned']:.1f} % pruned")
    assert c["max_strip_pairs"] > P.LIST_CAP
    assert c["nonzero_pixels"] >= 40


@pytest.mark.parametrize("which", ["rendered0", "rendered1", "sheet0", "sheet1"])
def test_the_oracle_ignores_poison_at_pruned_pixels(which):
    import oracle as O

    case = P.rendered(*P.RENDERED[int(which[-1])]) if which.startswith("rendered") else P.sheet(*P.SHEETS[int(which[-1])])
    c = P.conditions(case)
    img_p, go_p, count = P.poisoned(case, c)
    print(f"{which}: {count} poisoned pixels")
    assert count >= 100
    v, vi, idx, bary, img, go = case
    for M in (1e4, 0.5):
        assert th.equal(O.edge_grad_backward(v, img_p, idx, vi, go_p, M), O.edge_grad_backward(v, img, idx, vi, go, M))
