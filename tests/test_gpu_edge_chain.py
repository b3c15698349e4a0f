"""-m gpu: the batched loads of the one-pass fused edge backward (edge_dots_kernel in SCATTER mode, drtk_amd/csrc/edge_grad.hip).
Each phase of that kernel issues its loads together and without a branch around any of them, so loads are issued for
elements that do not exist -- past the end of a row, below the image, for lanes without a pair -- and must neither leave
the tensors nor reach the result.  Every case goes through tests/test_gpu_edge_onepass.py's `_check`: the CPU oracle in
float32 and float64, the route's per-element bound, both max_dp_dr values.  The cases are tests/edge_chain_cases.py's;
tests/test_edge_chain_cases_host.py asserts on the CPU that they are what they claim to be."""
import pytest
import torch as th

import edge_chain_cases as K
from test_gpu_edge_onepass import DEV, _check

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_pass(monkeypatch):
    monkeypatch.setenv("DRTK_AMD_EDGE_ONEPASS", "1")


@pytest.fixture
def in_buffers(monkeypatch):
    """capi.edge_grad_backward_fused with img, index_img, bary_img and grad_output re-placed as views into larger buffers
    (edge_chain_cases.embed): NaN around the float tensors, triangle 0 around the index.  `_check` compares with the oracle
    of the bare tensors, so a load that strays into the padding and is used changes the result."""
    from drtk_amd import capi

    real = capi.edge_grad_backward_fused

    def embedded(v_pix, img, index_img, vi, bary_img, grad_output, *args, **kwargs):
        row = img.shape[-1]
        views = [K.embed(t, row)[0] for t in (img, index_img, bary_img, grad_output)]
        for t in views:
            assert t.is_contiguous() and t.data_ptr() % 16 == t.element_size()
        return real(v_pix, views[0], views[1], vi, views[2], views[3], *args, **kwargs)

    monkeypatch.setattr(capi, "edge_grad_backward_fused", embedded)


@pytest.mark.parametrize("W,H,C", K.shapes())
def test_widths_and_heights_in_buffers(W, H, C, in_buffers):
    """W % 4 = 2 and W < 4 (a quad reaches past its row, at the last row past the view), one to nine rows, three views."""
    _check(*K.shape_case(W, H, C), f"{K.VIEWS} x {H} x {W}, C={C}, views in buffers", nonzero=K.shape_has_pairs(W, H))


def test_pair_counts_around_the_rounds(in_buffers):
    """Strips with 1, 63, 64, 65, ... 1008 differing pairs: a last round of one lane, a full one, a group of rounds with idle rounds."""
    _check(*K.pair_counts_case(), f"pair counts {K.PAIR_COUNTS}")


def test_strip_that_owes_one_pair(in_buffers):
    """All pairs of the strip are seams but one, in the halo row at lane 62's fourth pixel."""
    out = _check(*K.mixed_strip_case(), "mixed strip")
    for got, _ in out.values():
        assert bool((got != 0).any())


def test_two_calls_agree():
    """The same inputs twice: atomics order only (the bound of test_gpu_edge_onepass.py's test_two_calls_agree)."""
    from drtk_amd import capi

    v, vi, idx, bary, img, go = (t.to(DEV) for t in K.pair_counts_case())
    a = capi.edge_grad_backward_fused(v, img, idx, vi, bary, go)
    b = capi.edge_grad_backward_fused(v, img, idx, vi, bary, go)
    th.testing.assert_close(a, b, atol=1e-7, rtol=1e-5)
