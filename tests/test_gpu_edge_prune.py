"""-m gpu: the classification phase of the one-pass fused edge backward (edge_dots_kernel in SCATTER mode, needed_pair_flags,
drtk_amd/csrc/edge_grad.hip) -- the kernel classifies its differing pairs first and loads img / grad_output only where a
pair's term is used.  Scenes made of seams (tests/edge_prune_cases.py; their conditions are asserted on the CPU oracle, here
and in tests/test_edge_prune_cases_host.py), every case through tests/test_gpu_edge_onepass.py's `_check`: the CPU oracle in
float32 and float64, that route's own per-element bound, both max_dp_dr values."""
import pytest
import torch as th

import edge_prune_cases as P
from test_gpu_edge_onepass import DEV, LIST_CAP, _check  # (ELEMENT_ULPS["edge"] and FLOOR are applied inside _check)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_pass(monkeypatch):
    monkeypatch.setenv("DRTK_AMD_EDGE_ONEPASS", "1")


@pytest.mark.parametrize("n,lobes,C", P.RENDERED)
def test_rendered_list_path(n, lobes, C):
    """Two interpenetrating spheres: silhouettes, occlusion contours and intersections among nine seams in ten."""
    case = P.rendered(n, lobes, C)
    c = P.conditions(case)
    assert c["pruned"] >= 0.90 and c["nonzero_pixels"] >= 40 and c["z_pixels"] > 0 and 0 < c["max_strip_pairs"] <= LIST_CAP
    _check(*case, f"two spheres {n}x{n} lobes={lobes} C={C}")


def test_one_needed_pair_at_a_time():
    """One background pixel per view in a quad whose other pairs are all seams: a lane whose only needed pair is its fourth
    pixel's (the next lane loads for it), the lane 62/63 hand-over, the first pixel of the second strip, a vertical pair into
    a wave's and a workgroup's halo row, and no early return of a wave that still owes a pair."""
    case = P.quad_holes()
    c = P.conditions(case)
    want = [P.hole_nonzero_pixels(x, y, P.QUAD_H, P.QUAD_W) for x, y in P.hole_positions()]
    assert c["nonzero"].flatten(1).sum(1).tolist() == want
    _check(*case, "quad with one hole per view")


def test_seams_only_is_exactly_zero():
    """No pair's term is used: every wave returns after the classification, and the output is exactly zero over the poison."""
    from drtk_amd import capi

    case = P.quad_plain()
    c = P.conditions(case)
    assert c["edge_pixels"] > 0 and c["nonzero_pixels"] == 0
    out = _check(*case, "quad without a hole", nonzero=False)
    assert capi._POISON, "conftest.py sets DRTK_CAPI_POISON before drtk_amd.capi is imported"
    for got, _ in out.values():
        assert bool((got == 0).all())


@pytest.mark.parametrize("H,W", P.SHEETS)
def test_dense_strips_with_pruning(H, W):
    """More differing pairs than the pair list holds, nearly all of them seams: the classification takes any density."""
    case = P.sheet(H, W)
    c = P.conditions(case)
    assert c["max_strip_pairs"] > LIST_CAP and c["nonzero_pixels"] >= 40
    _check(*case, f"sheet {H}x{W}")


@pytest.mark.parametrize("which", ["rendered0", "rendered1", "sheet0", "sheet1"])
def test_skipping_equals_the_references_select(which, monkeypatch):
    """NaN in img and +Inf in grad_output where the reference discards the term with a select: the oracle's output is
    unchanged, and the kernel, given the poisoned images, meets the bound against the oracle of the clean ones."""
    import oracle as O
    from drtk_amd import capi

    case = P.rendered(*P.RENDERED[int(which[-1])]) if which.startswith("rendered") else P.sheet(*P.SHEETS[int(which[-1])])
    img_p, go_p, count = P.poisoned(case, P.conditions(case))
    assert count >= 100
    v, vi, idx, bary, img, go = case
    for M in (1e4, 0.5):
        assert th.equal(O.edge_grad_backward(v, img_p, idx, vi, go_p, M), O.edge_grad_backward(v, img, idx, vi, go, M))
    real = capi.edge_grad_backward_fused
    # _check computes its references from the clean case; the kernel alone is handed the poisoned images
    monkeypatch.setattr(capi, "edge_grad_backward_fused", lambda v_, img_, idx_, vi_, bary_, go_, M_: real(v_, img_p.to(DEV), idx_, vi_, bary_, go_p.to(DEV), M_))
    out = _check(*case, f"{which}, {count} poisoned pixels")
    for got, _ in out.values():
        assert bool(th.isfinite(got).all())


def test_two_calls_agree():
    """The same inputs twice: atomics order only."""
    from drtk_amd import capi

    v, vi, idx, bary, img, go = (t.to(DEV) for t in P.rendered(*P.RENDERED[0]))
    a = capi.edge_grad_backward_fused(v, img, idx, vi, bary, go)
    b = capi.edge_grad_backward_fused(v, img, idx, vi, bary, go)
    th.testing.assert_close(a, b, atol=1e-7, rtol=1e-5)
