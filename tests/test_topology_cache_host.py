"""CPU: the topology tables of the torch-op shim -- the chunked-CSR builders behind vertex_incidence and joint_incidence
(ATen, so they run on CPU tensors too) against capi's numpy restatement, and the cache protocol every family shares:
keyed by tensor identity + version counter + the family's own integer, 128 entries, LRU, one instance per family."""
import numpy as np
import pytest
import torch as th

import drtk_amd  # noqa: F401
from drtk_amd import capi

ops = th.ops.drtk_amd_ext


def _joint_cases():
    g = th.Generator().manual_seed(7)
    holes = th.tensor([[0, 1, -1], [2, -1, -1], [4, 0, 1], [1, 1, 4], [-1, -1, -1], [0, 2, 4], [4, 4, 4]])  # joint 3 unused
    k1 = th.randint(-1, 5, (9, 1), generator=g)
    k8 = th.randint(-1, 5, (11, 8), generator=g)
    kv = th.randint(-1, 5, (3, 7), generator=g)  # [K,V]; its transpose is a non-contiguous [V,K]
    return {
        "V7_K3_holes": (holes, 5),
        "K1": (k1, 5),
        "K8": (k8, 5),
        "V0": (th.empty(0, 3, dtype=th.int64), 5),
        "int32": (holes.int(), 5),
        "int64": (holes.long(), 5),
        "transposed": (kv.t(), 5),
    }


@pytest.mark.parametrize("case", list(_joint_cases()))
def test_joint_incidence_matches_numpy(case):
    idx, J = _joint_cases()[case]
    if case == "transposed":
        assert not idx.is_contiguous()
    crow, entries = ops.joint_incidence(idx, J)
    ref_crow, ref_entries = capi.joint_incidence_numpy(idx.contiguous().numpy(), J)[:2]
    assert crow.dtype == th.int32 and entries.dtype == th.int32
    assert np.array_equal(crow.numpy(), ref_crow)
    used = int(crow[J])
    assert used == int((idx >= 0).sum())
    assert np.array_equal(entries.numpy()[:used], ref_entries[:used])


@pytest.mark.parametrize("bad", [5, -2])
def test_joint_incidence_rejects_an_index_out_of_range_and_caches_nothing(bad):
    before = list(ops.skin_cache_stats())
    idx = th.tensor([[0, 1, -1], [2, bad, 4]])
    with pytest.raises(RuntimeError, match=r"outside \[-1, 5\)"):
        ops.joint_incidence(idx, 5)
    assert list(ops.skin_cache_stats()) == before


FAMILIES = {
    "geometry": (lambda t, n: ops.vertex_incidence(t, n), lambda: list(ops.geometry_cache_stats()),
                 lambda: ops.geometry_cache_clear(), lambda: th.tensor([[0, 1, 2], [2, 1, 3]], dtype=th.int32),
                 lambda: th.tensor([[0, 1, 2]], dtype=th.int32)),
    "skin": (lambda t, n: ops.joint_incidence(t, n), lambda: list(ops.skin_cache_stats()),
             lambda: ops.skin_cache_clear(), lambda: th.tensor([[0, 1], [3, -1], [2, 2]], dtype=th.int32),
             lambda: th.tensor([[0, 1, 2]], dtype=th.int32)),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_cache_protocol(family):
    call, stats, clear, make, make_row = FAMILIES[family]
    t = make()
    clear()
    assert stats() == [0, 0, 0]
    call(t, 4)
    assert stats() == [0, 1, 1]
    call(t, 4)
    assert stats() == [1, 1, 1]  # hit: same tensor, same version
    call(t.clone(), 4)
    assert stats() == [1, 2, 2]  # another tensor with equal content misses
    t.add_(0)  # in-place edit bumps the version counter
    call(t, 4)
    assert stats() == [1, 3, 3]
    call(t, 9)  # num_vertices / num_joints is part of the key
    assert stats() == [1, 4, 4]

    # eviction: 128 entries, least recently used first
    clear()
    keep = [make_row() for _ in range(130)]
    for r in keep:
        call(r, 3)
    assert stats() == [0, 130, 128]
    call(keep[0], 3)  # the oldest was evicted
    assert stats() == [0, 131, 128]
    call(keep[129], 3)
    assert stats() == [1, 131, 128]
    clear()
    assert stats() == [0, 0, 0]


def test_families_keep_their_own_entries_and_counters():
    all_stats = {
        "normal_matrix": lambda: list(ops.normal_matrix_cache_stats()),
        "geometry": lambda: list(ops.geometry_cache_stats()),
        "skin": lambda: list(ops.skin_cache_stats()),
        "kinematics": lambda: list(ops.kinematics_cache_stats()),
    }
    vi = th.tensor([[[0, 1, 2], [2, 1, 3]]], dtype=th.int32)
    calls = {
        "normal_matrix": lambda: ops.normal_matrix_structure(vi, 4),
        "geometry": lambda: ops.vertex_incidence(vi, 4),
        "skin": lambda: ops.joint_incidence(vi[0], 4),
    }
    for clear in (ops.normal_matrix_cache_clear, ops.geometry_cache_clear, ops.skin_cache_clear, ops.kinematics_cache_clear):
        clear()
    for name, call in calls.items():
        before = {k: s() for k, s in all_stats.items()}
        call()  # a miss: the same tensor is new to this family though the others hold it
        call()  # a hit
        after = {k: s() for k, s in all_stats.items()}
        assert after[name] == [1, 1, 1]
        for other in all_stats:
            if other != name:
                assert after[other] == before[other], (name, other)
    for clear in (ops.normal_matrix_cache_clear, ops.geometry_cache_clear, ops.skin_cache_clear):
        clear()


def test_vertex_incidence_batched_and_expanded():
    g = th.Generator().manual_seed(11)
    V, F = 9, 13
    vi = th.randint(0, V, (2, F, 3), generator=g, dtype=th.int32)
    crow, entries = ops.vertex_incidence(vi, V)
    ref = capi.vertex_incidence_numpy(vi.numpy(), V)
    assert crow.shape == (2 * V + 1,) and entries.shape == (3 * 2 * F,)
    assert np.array_equal(crow.numpy(), ref[0]) and np.array_equal(entries.numpy(), ref[1])

    one = vi[1]  # [F,3]
    shared = one[None].expand(4, -1, -1)  # stride-0 batch: analysed as one row
    assert shared.stride(0) == 0
    crow_s, entries_s = ops.vertex_incidence(shared, V)
    ref1 = capi.vertex_incidence_numpy(one.contiguous().numpy(), V)
    assert crow_s.shape == (V + 1,) and entries_s.shape == (3 * F,)
    assert np.array_equal(crow_s.numpy(), ref1[0]) and np.array_equal(entries_s.numpy(), ref1[1])
