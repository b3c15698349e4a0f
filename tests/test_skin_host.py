"""No GPU: drtk_amd.skin's PyTorch formulation (the route of CPU tensors) against the independent dense oracle
(tests/skin_oracle.py) in float64 -- forward and all three gradients on every structural case and seed --, known answers,
sparse_skin_weights, the numpy joint incidence of the C ABI, names, and the guarded script's case list."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch as th
from conftest import ROOT

import skin_oracle as O

KEYS = ("out", "grad_v", "grad_w", "grad_t")


def assert_exact_zeros(got, joint_idx, transforms, what):
    """The elements stated to be exactly 0 (compared with th.equal)"""
    z = O.exact_zeros(joint_idx, transforms)
    for k, mask in (("out", z["out"]), ("grad_w", z["grad_w"])):
        sel = got[k][:, mask] if k == "out" else got[k][mask]
        assert th.equal(sel, th.zeros_like(sel)), (what, k)
    gt = got["grad_t"]
    assert th.equal(gt[:, z["grad_t_joint"]], th.zeros_like(gt[:, z["grad_t_joint"]])), (what, "unnamed joint")
    if gt.shape[2] == 4:
        assert th.equal(gt[:, :, 3], th.zeros_like(gt[:, :, 3])), (what, "row 3")


@pytest.mark.parametrize("key", list(O.CASES) + list(O.SEEDS))
def test_cpu_formulation_matches_the_oracle_in_float64(key):
    import drtk_amd

    inputs = O.case(key) if isinstance(key, str) else O.build_case(key)
    got = O.results(drtk_amd.skin, *inputs, th.float64)
    ref = O.reference(key, th.float64)
    for k in KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == th.float64, (key, k)
        scale = float(ref[k].abs().max())
        assert scale > 0, (key, k)
        assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * scale, (key, k)
    assert_exact_zeros(got, inputs[1], inputs[3], key)


def test_cases_have_the_structure_they_are_named_for():
    from drtk_amd import capi

    assert O.CHUNK == capi.SKIN_CHUNK and O.LDS_JOINTS >= 1
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    assert re.search(r"#define\s+DRTK_SKIN_CHUNK\s+%d\b" % O.CHUNK, hdr)
    idx = O.case("chunked")[1]
    counts = th.bincount(idx.reshape(-1), minlength=5)
    assert counts[:4].tolist() == [O.CHUNK, O.CHUNK + 1, 2 * O.CHUNK + 37, 0] and O.case("chunked")[3].shape[0] == 2
    crow, entries, chunk_ptr, chunk_begin, chunk_joint = capi.joint_incidence_numpy(idx.numpy(), 5)
    assert np.diff(chunk_ptr).tolist()[:4] == [1, 2, 3, 0]
    for j in range(5):
        e = entries[crow[j]:crow[j + 1]]
        assert (np.diff(e) > 0).all() and (idx.reshape(-1).numpy()[e] == j).all()
    for c in range(len(chunk_joint)):
        j = chunk_joint[c]
        assert chunk_begin[c] == crow[j] + (c - chunk_ptr[j]) * O.CHUNK < crow[j + 1]
    assert O.case("many_joints")[3].shape[1] == O.LDS_JOINTS + 1 and O.case("many_joints")[0].shape[1] == 64
    k8 = O.case("k8_slots")[1]
    assert k8.shape[1] == 8 and bool((k8[3] < 0).all()) and int((k8[5] == 2).sum()) >= 2 and bool((k8 < 0).any())
    assert O.case("block_edge")[0].shape == (3, 257, 3)
    assert O.case("shared_v_expand")[0].stride(0) == 0 and O.case("shared_v")[0].shape[0] == 1
    assert not O.case("mat4_view")[3].is_contiguous() and O.case("mat4")[3].shape[-2:] == (4, 4)
    with pytest.raises(ValueError, match="outside"):
        capi.joint_incidence_numpy(np.array([[0, 5]]), 5)
    shapes = {(tuple(O.build_case(s)[0].shape), tuple(O.build_case(s)[3].shape)) for s in O.SEEDS}
    assert len(shapes) > 30
    for s in O.SEEDS:
        v, idx, w, t, g = O.build_case(s)
        assert v.shape[-2] <= 700 and t.shape[1] <= 40 and idx.shape[1] <= 8 and t.shape[0] <= 3


def test_known_answers():
    import drtk_amd

    gen = th.Generator().manual_seed(5)
    v = th.randn(2, 9, 3, dtype=th.float64, generator=gen)
    idx = th.randint(0, 4, (9, 3), generator=gen)
    idx[2, 1] = -1
    w = th.rand(9, 3, dtype=th.float64, generator=gen)
    eye = th.eye(4, dtype=th.float64)[:3].expand(2, 4, 3, 4).contiguous()
    wsum = th.where(idx >= 0, w, th.zeros_like(w)).sum(1)
    assert th.allclose(drtk_amd.skin(v, idx, w, eye), v * wsum[None, :, None], rtol=0, atol=1e-15)
    # a pure translation per joint: out = v * sum_k w + sum_k w t_j
    tr = eye.clone()
    tr[..., 3] = th.randn(2, 4, 3, dtype=th.float64, generator=gen)
    want = v * wsum[None, :, None] + (th.where(idx >= 0, w, th.zeros_like(w))[None, ..., None] * tr[:, idx.clamp(min=0), :, 3]).sum(2)
    assert th.allclose(drtk_amd.skin(v, idx, w, tr), want, rtol=0, atol=1e-14)
    # one joint rotating 90 degrees about z with weight 1: (x, y, z) -> (-y, x, z); [V,3] rest pose, 4x4 transforms, int32
    c, s = math.cos(math.pi / 2), math.sin(math.pi / 2)
    rot = th.tensor([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=th.float64)[None, None]
    out = drtk_amd.skin(v[0], th.zeros(9, 1, dtype=th.int32), th.ones(9, 1, dtype=th.float64), rot)
    assert out.shape == (1, 9, 3)
    assert th.allclose(out[0], th.stack([-v[0, :, 1], v[0, :, 0], v[0, :, 2]], 1), rtol=0, atol=1e-15)
    # every slot empty: exactly 0, whatever the weights hold
    out = drtk_amd.skin(v, th.full((9, 2), -1), th.full((9, 2), float("nan"), dtype=th.float64), tr)
    assert th.equal(out, th.zeros(2, 9, 3, dtype=th.float64))


def test_empty_inputs_on_the_cpu():
    import drtk_amd

    idx = th.zeros(4, 2, dtype=th.int64)
    w = th.ones(4, 2, dtype=th.float64, requires_grad=True)
    out = drtk_amd.skin(th.zeros(1, 4, 3, dtype=th.float64), idx, w, th.zeros(0, 3, 3, 4, dtype=th.float64))
    assert out.shape == (0, 4, 3)
    out.sum().backward()
    assert th.equal(w.grad, th.zeros_like(w))
    out = drtk_amd.skin(th.zeros(2, 0, 3), th.zeros(0, 2, dtype=th.int64), th.zeros(0, 2), th.zeros(2, 3, 3, 4))
    assert out.shape == (2, 0, 3)


def test_argument_errors_on_the_cpu():
    import drtk_amd

    v, idx, w, t, _ = O.case("tiny")
    with pytest.raises(ValueError, match="outside"):
        drtk_amd.skin(v, idx + 2, w, t)
    with pytest.raises(ValueError, match="outside"):
        drtk_amd.skin(v, idx - 2, w, t)
    with pytest.raises(ValueError, match="K = 9"):
        drtk_amd.skin(v, idx.expand(-1, 9), w.expand(-1, 9), t)
    with pytest.raises(TypeError, match="dtype of v"):
        drtk_amd.skin(v, idx, w.float(), t)
    with pytest.raises(TypeError, match="dtype of v"):
        drtk_amd.skin(v, idx, w, t.float())
    with pytest.raises(TypeError, match="int32 or int64"):
        drtk_amd.skin(v, idx.double(), w, t)
    for bad in (lambda: drtk_amd.skin(v[..., :2], idx, w, t), lambda: drtk_amd.skin(v, idx[:-1], w[:-1], t),
                lambda: drtk_amd.skin(v, idx, w[:, :0], t), lambda: drtk_amd.skin(v, idx, w, t[0]),
                lambda: drtk_amd.skin(v.expand(2, -1, -1), idx, w, t), lambda: drtk_amd.skin(v, idx, w, t[..., :3])):
        with pytest.raises(ValueError, match="expected"):
            bad()


def test_sparse_skin_weights_reproduces_the_dense_result():
    import drtk_amd

    gen = th.Generator().manual_seed(11)
    num_v, num_j = 50, 9
    dense = th.rand(num_v, num_j, dtype=th.float64, generator=gen)
    keep = th.rand(num_v, num_j, generator=gen).argsort(1) < th.randint(0, 5, (num_v, 1), generator=gen)  # 0 ... 4 non-zeros a row
    dense = dense * keep
    dense = dense / dense.sum(1, keepdim=True).clamp(min=1e-30) * (dense.sum(1, keepdim=True) > 0)
    v = th.randn(2, num_v, 3, dtype=th.float64, generator=gen)
    t = th.randn(2, num_j, 3, 4, dtype=th.float64, generator=gen)
    want = th.einsum("nvab,nvb->nva", th.einsum("vj,njab->nvab", dense, t)[..., :3], v) + th.einsum("vj,nja->nva", dense, t[..., 3])
    for k in (4, 6, 8):
        idx, w = drtk_amd.sparse_skin_weights(dense, k=k)
        assert idx.shape == (num_v, k) and w.shape == (num_v, k) and idx.dtype == th.int64
        assert th.equal(idx < 0, w == 0) and int((idx >= 0).sum()) == int(keep.sum())
        assert float((drtk_amd.skin(v, idx, w, t) - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # fewer slots than non-zeros: the k largest, renormalised to the row's sum of 1 -- or kept as they are
    idx, w = drtk_amd.sparse_skin_weights(dense, k=2)
    rows = keep.sum(1) >= 2
    assert th.allclose(w[rows].sum(1), th.ones(int(rows.sum()), dtype=th.float64))
    idx, w = drtk_amd.sparse_skin_weights(dense, k=2, renormalize=False)
    assert th.equal(w, th.gather(dense, 1, idx.clamp(min=0)) * (idx >= 0))
    assert th.equal(w[:, 0], dense.max(1).values)
    idx, w = drtk_amd.sparse_skin_weights(dense[:, :3], k=5)  # more slots than joints
    assert idx.shape == (num_v, 5) and bool((idx[:, 3:] == -1).all())
    with pytest.raises(ValueError):
        drtk_amd.sparse_skin_weights(dense, k=9)


def test_names_are_exported_and_declared():
    import drtk_amd
    from drtk_amd import capi

    for n in ("skin", "sparse_skin_weights"):
        assert n in drtk_amd.__all__ and callable(getattr(drtk_amd, n))
    assert drtk_amd.skin.__module__ == "drtk_amd.skin"
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    for n in ("drtk_amd_skin_forward", "drtk_amd_skin_backward", "drtk_amd_skin_backward_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in capi.EXPORTS
    import drtk

    assert not hasattr(drtk, "skin")  # the drop-in mirrors the reference, which has no such name


def test_c_abi_argument_validation_without_gpu():
    import ctypes

    from drtk_amd import capi

    L = capi.lib()
    i64, z, p = ctypes.c_int64, ctypes.c_void_p(0), ctypes.c_void_p(64)
    out = ctypes.c_size_t(0)
    assert L.drtk_amd_skin_backward_workspace_bytes(ctypes.c_int(0), i64(3), i64(5), ctypes.byref(out)) == 0
    assert out.value == 3 * 5 * 12 * 8
    assert L.drtk_amd_skin_backward_workspace_bytes(ctypes.c_int(1), i64(3), i64(5), ctypes.byref(out)) == 0 and out.value == 3 * 5 * 12 * 8
    assert L.drtk_amd_skin_backward_workspace_bytes(ctypes.c_int(7), i64(3), i64(5), ctypes.byref(out)) == -1

    def fwd(N=1, V=4, J=2, K=2, v_sN=12, t_sN=24, t_sJ=12, dtype=0):
        return L.drtk_amd_skin_forward(ctypes.c_int(dtype), p, i64(v_sN), p, p, p, i64(t_sN), i64(t_sJ), i64(N), i64(V), i64(J), i64(K), p, z)

    assert fwd(K=9) == -1 and fwd(K=0) == -1 and fwd(v_sN=5) == -1 and fwd(t_sJ=11) == -1 and fwd(t_sN=20) == -1 and fwd(dtype=5) == -1
    assert fwd(N=0) == 0 and fwd(V=0, v_sN=0) == 0  # nothing to launch

    def bwd(ws, nbytes, gt=p, rows=3, C=1, gv_B=1, outs=True):
        return L.drtk_amd_skin_backward(ctypes.c_int(0), p, p, i64(12), p, p, p, i64(24), i64(12), p, p, p, p, p, i64(C), i64(1), i64(4),
                                        i64(2), i64(2), i64(gv_B), z, z, i64(rows), gt if outs else z, ctypes.c_void_p(ws),
                                        ctypes.c_size_t(nbytes), z)

    assert bwd(0, 0) == -2 and bwd(4096, 95) == -2  # DRTK_ERR_WORKSPACE_TOO_SMALL
    assert bwd(4096 + 4, 1 << 20) == -1             # misaligned
    assert bwd(4096, 1 << 20, rows=5) == -1 and bwd(4096, 1 << 20, outs=False) == -1


def test_guarded_script_lists_its_cases():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_skin.py"), "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    names = r.stdout.split()
    assert len(names) == len(set(names)) >= 2 * len(O.CASES) and all(n.count("/") >= 2 for n in names)
