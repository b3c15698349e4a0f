"""No GPU: drtk_amd.forward_kinematics' PyTorch formulation (the route of CPU tensors) against the independent matrix_exp /
4x4 oracle (tests/kinematics_oracle.py) -- both outputs and all three gradients on every structural case and seed, in
float64 and float32 --, the zero pose, argument errors, the numpy schedule of the C ABI against hand-written answers, the C
entry points' argument checks, names, and forward_kinematics followed by skin against a directly written LBS."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch as th
from conftest import ROOT

import kinematics_oracle as O
from f64_distance import assert_within_f64_distance


def compare(got, r64, r32, dtype, what):
    """float64: 1e-12 of each result's scale from the float64 oracle; float32: within the project's float64-distance bound,
    max(1e-5 max|f64|, 3 |oracle_f32 - f64|), the oracles run on the float32 inputs.  A result the oracle has as exactly 0
    everywhere must be exactly 0."""
    for k in O.KEYS:
        assert got[k].dtype == dtype and got[k].shape == r64[k].shape, (what, k, got[k].shape, r64[k].shape)
        assert bool(th.isfinite(got[k]).all()), (what, k)
        scale = float(r64[k].abs().max()) if r64[k].numel() else 0.0
        err = float((got[k].double() - r64[k]).abs().max()) if r64[k].numel() else 0.0
        print(f"{what} {k} {dtype}: |got - f64| = {err:.3e}, max|f64| = {scale:.3e}"
              + (f", |oracle_f32 - f64| = {float((r32[k].double() - r64[k]).abs().max()):.3e}" if r32 is not None and r64[k].numel() else ""))
        if scale == 0:
            assert err == 0, (what, k)
        elif dtype == th.float64:
            assert err <= 1e-12 * scale, (what, k, err, scale)
        else:
            assert_within_f64_distance(got[k], r32[k], r64[k], f"{what} {k}")


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("key", list(O.CASES) + list(O.SEEDS))
def test_cpu_formulation_matches_the_oracle(key, dtype):
    import drtk_amd

    got = O.results(drtk_amd.forward_kinematics, O.key_case(key), dtype)
    compare(got, O.reference(key, th.float64), O.reference(key, th.float32) if dtype == th.float32 else None, dtype, str(key))


def test_cases_have_the_structure_they_are_named_for():
    from drtk_amd import capi
    from drtk_amd import kinematics as K

    assert O.MAX_JOINTS == capi.FK_MAX_JOINTS == K.MAX_JOINTS >= 256
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    assert re.search(r"#define\s+DRTK_FK_MAX_JOINTS\s+%d\b" % O.MAX_JOINTS, hdr)
    assert 2 * 12 * 8 * O.MAX_JOINTS <= 65536  # the backward's LDS state in double
    for dt in (th.float32, th.float64):
        assert abs(O.THETA0[dt] ** 2 - K.TAYLOR_THETA2[dt]) < 1e-15
    assert len(O.case("at_cap")["parents"]) == O.MAX_JOINTS and len(O.case("past_cap")["parents"]) == O.MAX_JOINTS + 1
    assert O.case("star70")["parents"] == [-1] + [0] * 69 and O.case("wide130")["parents"].count(-1) == 2
    assert O.case("chain32")["parents"] == [-1] + list(range(31))
    assert len(O.BODY24) == 24 and len(O.HAND16) == 16
    assert float(O.case("zero_pose")["rot_leaf"].abs().max()) == 0
    norms = O.case("tiny_pose")["rot_leaf"].norm(dim=-1)
    for dt in (th.float32, th.float64):
        for f in (0.5, 2.0):
            assert bool(((norms - f * O.THETA0[dt]).abs() < 1e-6).any()), (dt, f)
    assert abs(float(O.case("big_angle")["rot_leaf"].norm(dim=-1).max()) - 2.5 * np.pi) < 1e-5
    c = O.case("sliced_pose")
    assert c["rot_leaf"].shape == (3, 3 + 48) and not c["rot_view"](c["rot_leaf"]).is_contiguous()
    c = O.case("strided_pose")
    assert c["rot_view"](c["rot_leaf"]).stride() == (16 * 6, 6, 2)
    c = O.case("expanded_joints")
    assert c["joints_view"](c["joints_leaf"]).stride(0) == 0 and c["joints_view"](c["joints_leaf"]).shape == (3, 16, 3)
    assert O.case("per_view_joints")["joints_leaf"].shape == (3, 16, 3) and O.case("hand16")["joints_leaf"].shape == (16, 3)
    assert O.case("one_view")["rot_leaf"].shape[0] == 1 and O.case("no_translation")["translation"] is None
    assert O.case("only_posed_grad")["gA"] is None and O.case("only_transforms_grad")["gP"] is None
    assert O.case("matrices")["rot_leaf"].shape == (3, 24, 3, 3)
    seen = set()
    for s in O.SEEDS:
        c = O.build_case(s)
        p = c["parents"]
        assert 1 <= len(p) <= 96 and 1 <= p.count(-1) <= 3 and all(q == -1 or 0 <= q < j for j, q in enumerate(p))
        assert 1 <= c["rot_leaf"].shape[0] <= 5
        seen.add((c["rot_leaf"].dim(), c["joints_leaf"].dim(), c["translation"] is None, c["gA"] is None, c["gP"] is None))
    assert len(seen) >= 10


def test_zero_pose_gives_the_identity_and_the_generators():
    import drtk_amd

    case = O.case("zero_pose")
    for dtype in (th.float32, th.float64):
        got = O.results(drtk_amd.forward_kinematics, case, dtype)
        ref = O.reference("zero_pose", dtype)
        eye = th.eye(3, dtype=dtype).expand(3, 24, 3, 3)
        assert th.equal(got["transforms"][..., :3], eye)  # R = I bit for bit
        assert bool(th.isfinite(got["grad_rot"]).all()) and float(got["grad_rot"].abs().max()) > 0
        tol = 1e-12 if dtype == th.float64 else 1e-5
        assert float((got["grad_rot"] - ref["grad_rot"]).abs().max()) <= tol * float(ref["grad_rot"].abs().max())
    # one joint, r = 0, gradient M to R: the three generators, (M21 - M12, M02 - M20, M10 - M01)
    r = th.zeros(1, 1, 3, dtype=th.float64, requires_grad=True)
    t, _ = drtk_amd.forward_kinematics(r, th.zeros(1, 3, dtype=th.float64), [-1])
    m = th.arange(9, dtype=th.float64).view(3, 3) ** 1.5
    (g,) = th.autograd.grad((t[0, 0, :, :3] * m).sum(), r)
    want = th.stack([m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    assert float((g[0, 0] - want).abs().max()) <= 1e-14 * float(want.abs().max())


def test_known_answers():
    import drtk_amd

    # a two-joint arm along x, the elbow at (1, 0, 0), the root turned 90 degrees about z: the elbow lands at (0, 1, 0); the
    # elbow's own rotation moves nothing but its frame
    half_pi = float(np.pi / 2)
    r = th.tensor([[[0.0, 0.0, half_pi], [0.3, -0.2, 0.1]]], dtype=th.float64)
    c = th.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=th.float64)
    t, posed = drtk_amd.forward_kinematics(r, c, th.tensor([-1, 0], dtype=th.int32))
    assert t.shape == (1, 2, 3, 4) and posed.shape == (1, 2, 3)
    assert th.allclose(posed[0], th.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=th.float64), rtol=0, atol=1e-15)
    # the skinning matrix maps the rest joint to the posed joint
    assert th.allclose((t[0, :, :, :3] @ c[..., None])[..., 0] + t[0, :, :, 3], posed[0], rtol=0, atol=1e-15)
    # a translation moves everything; the identity pose gives [I | translation]
    tr = th.tensor([[0.5, -1.0, 2.0]], dtype=th.float64)
    t, posed = drtk_amd.forward_kinematics(th.zeros(1, 2, 3, dtype=th.float64), c[None], [-1, 0], tr)
    assert th.equal(t[0, :, :, :3], th.eye(3, dtype=th.float64).expand(2, 3, 3)) and th.allclose(t[0, :, :, 3], tr.expand(2, 3))
    assert th.allclose(posed[0], c + tr)
    # matrices are used as given: a scale of 2 at the root doubles the offset of the child
    m = th.stack([2 * th.eye(3, dtype=th.float64), th.eye(3, dtype=th.float64)])[None]
    _, posed = drtk_amd.forward_kinematics(m, c, (-1, 0))
    assert th.allclose(posed[0, 1], th.tensor([2.0, 0.0, 0.0], dtype=th.float64))


def test_empty_inputs_on_the_cpu():
    import drtk_amd

    c = th.zeros(4, 3, dtype=th.float64, requires_grad=True)
    t, p = drtk_amd.forward_kinematics(th.zeros(0, 4, 3, dtype=th.float64), c, [-1, 0, 1, 1])
    assert t.shape == (0, 4, 3, 4) and p.shape == (0, 4, 3)
    (t.sum() + p.sum()).backward()
    assert th.equal(c.grad, th.zeros_like(c))
    tr = th.zeros(2, 3, requires_grad=True)
    t, p = drtk_amd.forward_kinematics(th.zeros(2, 0, 3), th.zeros(0, 3), [], tr)
    assert t.shape == (2, 0, 3, 4) and p.shape == (2, 0, 3)
    (t.sum() + p.sum()).backward()
    assert th.equal(tr.grad, th.zeros_like(tr))


def test_parents_errors():
    import drtk_amd

    r, c = th.zeros(2, 4, 3, dtype=th.float64), th.zeros(4, 3, dtype=th.float64)
    for bad in ([-1, 0, 2, 1], [-1, 1, 0, 0], [0, 0, 1, 2], [-1, 0, -2, 1], [-1, 0, 1], [-1, 0, 1, 2, 3]):
        for make in (list, lambda p: th.tensor(p, dtype=th.int32), lambda p: th.tensor(p, dtype=th.int64)):
            with pytest.raises(ValueError, match="parents"):
                drtk_amd.forward_kinematics(r, c, make(bad))
    with pytest.raises((TypeError, ValueError), match="parents"):
        drtk_amd.forward_kinematics(r, c, th.tensor([-1.0, 0.0, 1.0, 2.0]))
    with pytest.raises((TypeError, ValueError), match="parents"):
        drtk_amd.forward_kinematics(r, c, [-1, 0.0, 1, 2])
    with pytest.raises(ValueError, match="parents"):
        drtk_amd.forward_kinematics(r, c, th.tensor([[-1, 0, 1, 2]]))


def test_shape_and_dtype_errors():
    import drtk_amd

    r, c, p = th.zeros(2, 4, 3, dtype=th.float64), th.zeros(4, 3, dtype=th.float64), [-1, 0, 1, 2]
    for args in ((r[..., :2], c, p), (r[0], c, p), (th.zeros(2, 4, 3, 4, dtype=th.float64), c, p), (r, c[:3], p), (r, c[:, :2], p),
                 (r, c.expand(3, -1, -1), p), (r, c, p, th.zeros(3, 3, dtype=th.float64)), (r, c, p, th.zeros(2, 4, dtype=th.float64))):
        with pytest.raises(ValueError, match="expected"):
            drtk_amd.forward_kinematics(*args)
    for args in ((r, c.float(), p), (r, c, p, th.zeros(2, 3)), (r.long(), c, p)):
        with pytest.raises(TypeError, match="expected"):
            drtk_amd.forward_kinematics(*args)


def test_names_are_exported_and_declared():
    import drtk_amd
    from drtk_amd import capi

    assert "forward_kinematics" in drtk_amd.__all__ and callable(drtk_amd.forward_kinematics)
    assert drtk_amd.forward_kinematics.__module__ == "drtk_amd.kinematics"
    from drtk_amd import kinematics as K

    for n in ("kinematic_schedule", "kinematics_cache_stats", "kinematics_cache_clear"):
        assert callable(getattr(K, n))
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    for n in ("drtk_amd_kinematics_forward", "drtk_amd_kinematics_backward", "drtk_amd_kinematics_backward_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in capi.EXPORTS
    import drtk

    assert not hasattr(drtk, "forward_kinematics")  # the drop-in mirrors the reference, which has no such name


def test_schedule_builder_against_hand_written_answers():
    from drtk_amd import capi

    parents, order, level_start, crow, entries = capi.kinematic_schedule_numpy([-1, 0, 1, 2, 3])  # chain5
    assert order.tolist() == [0, 1, 2, 3, 4] and level_start.tolist() == [0, 1, 2, 3, 4, 5]
    assert crow.tolist() == [0, 1, 2, 3, 4, 4] and entries.tolist() == [1, 2, 3, 4] and parents.tolist() == [-1, 0, 1, 2, 3]
    parents, order, level_start, crow, entries = capi.kinematic_schedule_numpy(np.array([-1] + [0] * 69, dtype=np.int32))  # star70
    assert order.tolist() == list(range(70)) and level_start.tolist() == [0, 1, 70]
    assert crow.tolist() == [0] + [69] * 70 and entries.tolist() == list(range(1, 70))
    # a forest: roots 0 and 2; 0 -> {1, 6}, 2 -> {3}, 1 -> {4}, 3 -> {5}
    parents, order, level_start, crow, entries = capi.kinematic_schedule_numpy(th.tensor([-1, 0, -1, 2, 1, 3, 0]).numpy())
    assert order.tolist() == [0, 2, 1, 3, 6, 4, 5] and level_start.tolist() == [0, 2, 5, 7]
    assert crow.tolist() == [0, 2, 3, 4, 5, 5, 5, 5] and entries.tolist() == [1, 6, 4, 3, 5]
    assert all(a.dtype == np.int32 for a in (parents, order, level_start, crow, entries))
    empty = capi.kinematic_schedule_numpy(np.zeros(0, dtype=np.int64))
    assert [a.tolist() for a in empty] == [[], [], [0], [0], []]
    for bad in ([-1, 1], [0], [-2], [-1, 0, 2]):
        with pytest.raises(ValueError, match="parents"):
            capi.kinematic_schedule_numpy(bad)
    with pytest.raises(ValueError, match="parents"):
        capi.kinematic_schedule_numpy(np.array([-1.0, 0.0]))


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    i64, z, p = ctypes.c_int64, ctypes.c_void_p(0), ctypes.c_void_p(64)
    strides = (ctypes.c_int64 * 4)(12, 3, 1, 0)
    out = ctypes.c_size_t(7)
    ws = L.drtk_amd_kinematics_backward_workspace_bytes
    assert ws(ctypes.c_int(0), i64(3), i64(5), i64(1), ctypes.byref(out)) == 0 and out.value == 3 * 5 * 3 * 4
    assert ws(ctypes.c_int(1), i64(3), i64(5), i64(1), ctypes.byref(out)) == 0 and out.value == 3 * 5 * 3 * 8
    assert ws(ctypes.c_int(1), i64(3), i64(5), i64(3), ctypes.byref(out)) == 0 and out.value == 0  # per view: no second launch
    assert ws(ctypes.c_int(1), i64(1), i64(5), i64(1), ctypes.byref(out)) == 0 and out.value == 0  # one view
    assert ws(ctypes.c_int(1), i64(3), i64(5), i64(0), ctypes.byref(out)) == 0 and out.value == 0  # no grad_joints
    assert ws(ctypes.c_int(7), i64(3), i64(5), i64(1), ctypes.byref(out)) == -1
    assert ws(ctypes.c_int(0), i64(3), i64(5), i64(2), ctypes.byref(out)) == -1
    assert ws(ctypes.c_int(0), i64(3), i64(capi.FK_MAX_JOINTS + 1), i64(1), ctypes.byref(out)) == -1

    def fwd(N=2, J=4, D=2, mat=0, c_sN=0, dtype=0, st=strides):
        return L.drtk_amd_kinematics_forward(ctypes.c_int(dtype), p, ctypes.c_int(mat), st, p, i64(c_sN), z, p, p, p, i64(D), i64(N), i64(J),
                                             p, p, z)

    assert fwd(J=capi.FK_MAX_JOINTS + 1, D=3) == -1  # past the cap: the invalid-argument status
    assert fwd(dtype=5) == -1 and fwd(c_sN=5) == -1 and fwd(mat=2) == -1 and fwd(D=0) == -1 and fwd(D=5) == -1 and fwd(N=-1) == -1
    assert fwd(st=None) == -1
    assert fwd(N=0) == 0 and fwd(J=0, D=0) == 0  # nothing to launch

    def bwd(ws_ptr=4096, nbytes=1 << 20, N=3, J=4, D=2, B=1, outs=(p, p, p), dtype=0):
        return L.drtk_amd_kinematics_backward(ctypes.c_int(dtype), p, p, p, ctypes.c_int(0), strides, p, i64(0), p, p, p, p, i64(D), p, p,
                                              i64(N), i64(J), outs[0], i64(B), outs[1], outs[2], ctypes.c_void_p(ws_ptr),
                                              ctypes.c_size_t(nbytes), z)

    assert bwd(ws_ptr=0, nbytes=0) == -2 and bwd(nbytes=3 * 4 * 3 * 4 - 1) == -2  # DRTK_ERR_WORKSPACE_TOO_SMALL
    assert bwd(ws_ptr=4096 + 4) == -1                                              # misaligned
    assert bwd(outs=(z, z, z)) == -1 and bwd(B=2) == -1 and bwd(J=capi.FK_MAX_JOINTS + 1) == -1 and bwd(dtype=3) == -1
    assert bwd(N=0, J=0, D=0) == 0


def test_forward_kinematics_then_skin_reproduces_a_directly_written_lbs():
    import drtk_amd

    gen = th.Generator().manual_seed(9)
    N, V, J = 2, 60, 16
    pose = 0.4 * th.randn(N, J, 3, dtype=th.float64, generator=gen)
    joints = 0.3 * th.randn(J, 3, dtype=th.float64, generator=gen)
    v = th.randn(V, 3, dtype=th.float64, generator=gen)
    dense = th.softmax(3 * th.randn(V, J, dtype=th.float64, generator=gen), 1)
    idx, w = drtk_amd.sparse_skin_weights(dense, k=4)
    tr = th.randn(N, 3, dtype=th.float64, generator=gen)
    transforms, posed = drtk_amd.forward_kinematics(pose, joints, O.HAND16, tr)
    got = drtk_amd.skin(v, idx, w, transforms)
    # directly: world matrices by the textbook recursion on points, v' = sum_j w_ij (G_j.R (v - c_j) + G_j.t)
    rot = th.linalg.matrix_exp(O._skew(pose))
    gr, gt = [None] * J, [None] * J
    for j, p in enumerate(O.HAND16):
        if p < 0:
            gr[j], gt[j] = rot[:, j], joints[j] + tr
        else:
            gr[j] = gr[p] @ rot[:, j]
            gt[j] = (gr[p] @ (joints[j] - joints[p])[:, None])[..., 0] + gt[p]
    valid = idx >= 0
    want = th.zeros(N, V, 3, dtype=th.float64)
    for k in range(4):
        for i in range(V):
            if valid[i, k]:
                j = int(idx[i, k])
                want[:, i] += w[i, k] * ((gr[j] @ (v[i] - joints[j])[:, None])[..., 0] + gt[j])
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert float((posed - th.stack(gt, 1)).abs().max()) <= 1e-14


def test_guarded_script_lists_its_cases():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_kinematics.py"), "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    names = r.stdout.split()
    assert len(names) == len(set(names)) >= 2 * (len(O.CASES) - 1) and all(n.count("/") >= 2 for n in names)
