"""GPU: drtk_amd.forward_kinematics on the HIP route (csrc/kinematics.hip through drtk_amd_ext::forward_kinematics and through
the C ABI) -- both outputs and all three gradients against the independent matrix_exp oracle (tests/kinematics_oracle.py) on
its structural cases and 30 seeded trees, the C ABI, either parents dtype and a list, cold and warm cache bit for bit, each
gradient on its own, exact zeros, the launches of each combination, empty inputs, errors, graph capture, the chain into
skin, and the C ABI between sentinel elements (tests/guarded_kinematics.py in a child process)."""
import importlib
import os
import subprocess
import sys

import pytest
import torch as th
from conftest import ROOT

import kinematics_oracle as O
import skin_oracle as SO
from test_kinematics_host import compare

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("rotations", "joints", "translation")


def capi_results(case, dtype, grads=ALL):
    """O.results through the C ABI's two entry points (int32 schedule built with numpy) the way
    csrc/torch_ops/kinematics.cpp calls them; the gradients that `grads` names, mapped back to the leaves."""
    from drtk_amd import capi

    rl, jl = case["rot_leaf"].to(dtype).to(DEV), case["joints_leaf"].to(dtype).to(DEV)
    rot = case["rot_view"](rl)
    joints = case["joints_view"](jl)  # (an expanded rest pose: N rows to the C ABI, their gradients added as autograd adds them)
    expanded = joints.shape != jl.shape
    tr = None if case["translation"] is None else case["translation"].to(dtype).to(DEV)
    sch = capi.kinematic_schedule_numpy(case["parents"])
    transforms, posed = capi.kinematics_forward(rot, joints, sch, tr)
    res = {"transforms": transforms, "posed": posed}
    gA = None if case["gA"] is None else case["gA"].to(dtype).to(DEV)
    gP = None if case["gP"] is None else case["gP"].to(dtype).to(DEV)
    gr, gc, gt = capi.kinematics_backward(gA, gP, rot, joints, sch, tr, grads=grads)
    if gr is not None:
        leaf = th.zeros_like(rl)
        case["rot_view"](leaf).copy_(gr)
        res["grad_rot"] = leaf
    if gc is not None:
        res["grad_joints"] = (gc.sum(0, keepdim=True) if expanded else gc).view(jl.shape)
    if "translation" in grads:
        res["grad_tr"] = gt if gt is not None else th.zeros(rot.shape[0], 3, dtype=dtype)
    return {k: x.detach().cpu() for k, x in res.items()}


def hip_results(case, dtype, api="ops", parents=None):
    import drtk_amd

    if api == "capi":
        return capi_results(case, dtype)
    return O.results(drtk_amd.forward_kinematics, case, dtype, DEV, parents=parents)


def check_key(key, dtype, api="ops"):
    got = hip_results(O.key_case(key), dtype, api)
    compare(got, O.reference(key, th.float64), O.reference(key, th.float32) if dtype == th.float32 else None, dtype, f"{key} {api}")
    return got


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("key", list(O.CASES) + list(O.SEEDS))
def test_outputs_and_all_gradients_match_the_oracle(key, dtype):
    """(`past_cap` takes the PyTorch formulation on the device: same bounds)"""
    check_key(key, dtype)


@pytest.mark.parametrize("key", [k for k in O.CASES if k != "past_cap"] + [2, 11, 23])
def test_c_abi_and_every_form_of_parents_give_the_operators_results_bit_for_bit(key):
    case = O.key_case(key)
    for dtype in (th.float32, th.float64):
        a = hip_results(case, dtype)
        others = {"capi": hip_results(case, dtype, "capi"),
                  "int32": hip_results(case, dtype, parents=th.tensor(case["parents"], dtype=th.int32, device=DEV)),
                  "int64 cpu": hip_results(case, dtype, parents=th.tensor(case["parents"], dtype=th.int64)),
                  "tuple": hip_results(case, dtype, parents=tuple(case["parents"]))}
        for name, b in others.items():
            for k in O.KEYS:
                assert th.equal(a[k], b[k]), (key, dtype, k, name)


def test_past_the_cap_the_c_abi_refuses_and_the_operator_raises():
    from drtk_amd import capi

    case = O.case("past_cap")
    with pytest.raises(capi.DrtkAmdError, match="status -1"):
        capi_results(case, th.float32)
    rot, c = case["rot_leaf"].to(DEV), case["joints_leaf"].to(DEV)
    with pytest.raises(RuntimeError, match="at most"):
        th.ops.drtk_amd_ext.forward_kinematics(rot, c, None, case["parents"], None)


def test_bitwise_reproducible_cold_and_warm():
    K = importlib.import_module("drtk_amd.kinematics")
    for name in ("wide130", "body24", "matrices", "expanded_joints"):
        for dtype in (th.float32, th.float64):
            K.kinematics_cache_clear()
            a = hip_results(O.case(name), dtype)
            assert K.kinematics_cache_stats()[1] == 1  # one build per parent list
            K.kinematics_cache_clear()
            b = hip_results(O.case(name), dtype)
            c = hip_results(O.case(name), dtype)
            assert K.kinematics_cache_stats()[:2] == (1, 1)
            for k in O.KEYS:
                assert th.equal(a[k], b[k]) and th.equal(a[k], c[k]), (name, dtype, k)
    # one parents tensor, used twice: a hit; edited in place: a miss; a list is keyed by its contents
    import drtk_amd

    case = O.case("no_translation")
    r, c = case["rot_leaf"].to(DEV), case["joints_leaf"].to(DEV)
    parents = th.tensor(case["parents"], device=DEV)
    K.kinematics_cache_clear()
    first = drtk_amd.forward_kinematics(r, c, parents)[0]
    assert th.equal(drtk_amd.forward_kinematics(r, c, parents)[0], first) and K.kinematics_cache_stats()[:2] == (1, 1)
    parents[4] = 0
    assert not th.equal(drtk_amd.forward_kinematics(r, c, parents)[0], first) and K.kinematics_cache_stats()[:2] == (1, 2)
    drtk_amd.forward_kinematics(r, c, list(case["parents"]))
    drtk_amd.forward_kinematics(r, c, tuple(case["parents"]))
    assert K.kinematics_cache_stats()[:2] == (2, 3)
    order, level_start, crow, entries = K.kinematic_schedule(case["parents"], DEV)
    assert K.kinematics_cache_stats()[0] == 3
    assert order.tolist() == [0, 2, 1, 3, 6, 4, 5] and level_start.tolist() == [0, 2, 5, 7]
    assert crow.tolist() == [0, 2, 3, 4, 5, 5, 5, 5] and entries.tolist() == [1, 6, 4, 3, 5] and order.dtype == th.int32
    with pytest.raises(ValueError, match="parents"):
        drtk_amd.forward_kinematics(r, c, th.tensor([-1, 0, 2, 1, 1, 1, 1], device=DEV))
    with pytest.raises(ValueError, match="parents"):
        drtk_amd.forward_kinematics(r, c, [-1, 0, 1])


@pytest.mark.parametrize("name", ["body24", "matrices", "hand16", "per_view_joints", "wide130"])
def test_each_gradient_alone_has_the_bits_it_has_with_all(name):
    import drtk_amd

    case = O.case(name)
    for dtype in (th.float32, th.float64):
        full = hip_results(case, dtype)
        for which, key in enumerate(("grad_rot", "grad_joints", "grad_tr")):
            leaves = [case["rot_leaf"], case["joints_leaf"], case["translation"]]
            r, c, t = (x.to(dtype).to(DEV).clone().requires_grad_(i == which) for i, x in enumerate(leaves))
            transforms, posed = drtk_amd.forward_kinematics(case["rot_view"](r), case["joints_view"](c), case["parents"], t)
            loss = (transforms * case["gA"].to(dtype).to(DEV)).sum() + (posed * case["gP"].to(dtype).to(DEV)).sum()
            loss.backward()
            got = (r, c, t)[which].grad
            assert all(x.grad is None for i, x in enumerate((r, c, t)) if i != which)
            assert th.equal(got.cpu(), full[key]), (name, dtype, key)
            assert th.equal(transforms.detach().cpu(), full["transforms"]) and th.equal(posed.detach().cpu(), full["posed"])
        # the C ABI likewise
        for grads, key in ((("rotations",), "grad_rot"), (("joints",), "grad_joints"), (("translation",), "grad_tr")):
            assert th.equal(capi_results(case, dtype, grads)[key], full[key]), (name, dtype, key, "capi")


def test_exact_zeros_where_the_definition_has_them():
    import drtk_amd

    for dtype in (th.float32, th.float64):
        # only the posed joints are used: a joint without children moves no joint, so its rotation gets exactly 0
        got = hip_results(O.case("only_posed_grad"), dtype)
        leaf = O.leaf_joints(O.HAND16)
        assert bool(leaf.any()) and th.equal(got["grad_rot"][:, leaf], th.zeros_like(got["grad_rot"][:, leaf]))
        assert float(got["grad_rot"][:, ~leaf].abs().amax(-1).min()) > 0
        # only the transforms are used, through their translation column of one joint: the joints that are not its ancestors
        # get exactly 0, and so does a translation's gradient in the views whose output gradient is 0
        case = O.case("hand16")
        r = case["rot_leaf"].to(dtype).to(DEV).requires_grad_(True)
        t = case["translation"].to(dtype).to(DEV).requires_grad_(True)
        transforms, _ = drtk_amd.forward_kinematics(r, case["joints_leaf"].to(dtype).to(DEV), case["parents"], t)
        gr, gt = th.autograd.grad(transforms[1, 9, :, 3].sum(), (r, t))
        on_path = th.zeros(16, dtype=th.bool)
        on_path[[0, 7, 8, 9]] = True  # 9 <- 8 <- 7 <- 0
        assert th.equal(gr[:, ~on_path].cpu(), th.zeros(3, 12, 3, dtype=dtype)) and th.equal(gr[[0, 2]].cpu(), th.zeros(2, 16, 3, dtype=dtype))
        assert float(gr[1, on_path].abs().amax(-1).min()) > 0
        assert th.equal(gt[[0, 2]].cpu(), th.zeros(2, 3, dtype=dtype)) and th.equal(gt[1].cpu(), th.ones(3, dtype=dtype))
        # the zero pose: R = I bit for bit, in every view
        z = hip_results(O.case("zero_pose"), dtype)
        assert th.equal(z["transforms"][..., :3], th.eye(3, dtype=dtype).expand(3, 24, 3, 3))
        assert bool(th.isfinite(z["grad_rot"]).all()) and float(z["grad_rot"].abs().max()) > 0


@pytest.mark.parametrize("name, need, launches", [
    ("hand16", (True, True, True), 2),            # a shared rest pose of three views: the second launch
    ("hand16", (True, False, True), 1),
    ("hand16", (False, True, False), 2),
    ("hand16", (False, False, True), 1),
    ("per_view_joints", (True, True, True), 1),
    ("expanded_joints", (True, True, True), 1),   # one row per view; autograd adds an expand's rows
    ("one_view", (True, True, True), 1),
    ("matrices", (True, True, False), 2),
    ("no_translation", (True, False, False), 1),
    ("hand16", (False, False, False), 0),
])
def test_one_launch_forward_and_one_backward_and_a_second_only_for_a_shared_rest_pose(name, need, launches):
    import drtk_amd
    from drtk_amd import capi

    case = O.case(name)
    leaves = [case["rot_leaf"], case["joints_leaf"], case["translation"]]
    r, c, t = (None if x is None else x.float().to(DEV).clone().requires_grad_(n) for x, n in zip(leaves, need))
    drtk_amd.forward_kinematics(case["rot_view"](r), case["joints_view"](c), case["parents"], t)  # (the schedule: cached)
    th.cuda.synchronize()
    capi.kernel_timing_begin()
    transforms, posed = drtk_amd.forward_kinematics(case["rot_view"](r), case["joints_view"](c), case["parents"], t)
    th.cuda.synchronize()
    fwd = capi.kernel_timing_report()
    assert sum(n for _, (n, _) in fwd.items()) == 1 and all("fk_forward_kernel" in k for k in fwd), fwd
    capi.kernel_timing_begin()
    if transforms.requires_grad:
        (transforms * case["gA"].float().to(DEV)).sum().backward()
    th.cuda.synchronize()
    rep = capi.kernel_timing_report()
    count = lambda name: sum(n for k, (n, _) in rep.items() if name in k)  # noqa: E731
    assert all("fk_" in k for k in rep), rep
    assert count("fk_backward_kernel") == int(any(need)) and count("fk_joint_sum_kernel") == launches - int(any(need)), (need, rep)
    if any(need):
        (kernel,) = [k for k in rep if "fk_backward_kernel" in k]
        flags = [a.strip() for a in kernel.split("<")[1].split(">")[0].split(",")]
        want = [str(case["rot_leaf"].dim() == 4).lower()] + [str(bool(n)).lower() for n in need]
        assert flags[1:] == want, kernel
    for x, n in zip((r, c, t), need):
        assert x is None or (x.grad is not None) == n


def test_no_views_and_no_joints():
    import drtk_amd

    for dtype in (th.float32, th.float64):
        c = th.randn(4, 3, dtype=dtype, device=DEV, requires_grad=True)
        r0 = th.zeros(0, 4, 3, dtype=dtype, device=DEV, requires_grad=True)
        tr0 = th.zeros(0, 3, dtype=dtype, device=DEV, requires_grad=True)
        transforms, posed = drtk_amd.forward_kinematics(r0, c, [-1, 0, 1, 1], tr0)
        assert transforms.shape == (0, 4, 3, 4) and posed.shape == (0, 4, 3)
        (transforms.sum() + posed.sum()).backward()
        assert th.equal(c.grad, th.zeros_like(c)) and r0.grad.shape == (0, 4, 3) and tr0.grad.shape == (0, 3)  # the empty sum
        tr = th.randn(2, 3, dtype=dtype, device=DEV, requires_grad=True)
        r = th.zeros(2, 0, 3, dtype=dtype, device=DEV, requires_grad=True)
        c0 = th.zeros(0, 3, dtype=dtype, device=DEV, requires_grad=True)
        transforms, posed = drtk_amd.forward_kinematics(r, c0, [], tr)
        assert transforms.shape == (2, 0, 3, 4) and posed.shape == (2, 0, 3)
        (transforms.sum() + posed.sum()).backward()
        assert th.equal(tr.grad, th.zeros_like(tr)) and r.grad.shape == (2, 0, 3) and c0.grad.shape == (0, 3)  # no roots


def test_errors():
    import drtk_amd

    case = O.case("hand16")
    r, c = case["rot_leaf"].to(DEV), case["joints_leaf"].to(DEV)
    p = case["parents"]
    with pytest.raises(RuntimeError, match="HIP"):
        th.ops.drtk_amd_ext.forward_kinematics(r.cpu(), c.cpu(), None, p, None)
    for args in ((r[..., :2], c, None, p, None), (r, c[:3], None, p, None), (r, c, None, p, th.zeros(2, 3, dtype=r.dtype, device=DEV)),
                 (r, c.float(), None, p, None), (r, c.cpu(), None, p, None)):
        with pytest.raises(RuntimeError, match="expected"):
            th.ops.drtk_amd_ext.forward_kinematics(*args)
    with pytest.raises((TypeError, ValueError), match="parents"):
        drtk_amd.forward_kinematics(r, c, th.tensor(p, device=DEV).float())
    with pytest.raises(TypeError, match="int32 or int64"):
        th.ops.drtk_amd_ext.forward_kinematics(r, c, th.tensor(p, device=DEV).double(), [], None)
    rr, cc = r.clone().requires_grad_(True), c.clone().requires_grad_(True)
    tt = case["translation"].to(DEV).requires_grad_(True)
    for wrt in (rr, cc, tt):
        transforms, posed = drtk_amd.forward_kinematics(rr, cc, p, tt)
        with pytest.raises(RuntimeError, match="double backward"):
            th.autograd.grad(transforms.square().sum() + posed.square().sum(), wrt, create_graph=True)
        (g,) = th.autograd.grad(drtk_amd.forward_kinematics(rr, cc, p, tt)[1].square().sum(), wrt)  # a plain backward still works
        assert bool(th.isfinite(g).all())


def test_a_capture_on_a_cold_cache_raises_and_a_captured_step_replays_the_eager_bits():
    import drtk_amd

    K = importlib.import_module("drtk_amd.kinematics")
    case = O.case("body24")
    theta = th.cat([th.zeros(3, 3, dtype=th.float64), case["rot_leaf"].reshape(3, -1)], 1).float().to(DEV).requires_grad_(True)
    c = case["joints_leaf"].float().to(DEV).requires_grad_(True)
    tr = case["translation"].float().to(DEV).requires_grad_(True)
    parents = th.tensor(case["parents"], dtype=th.int32, device=DEV)
    gA, gP = case["gA"].float().to(DEV), case["gP"].float().to(DEV)

    K.kinematics_cache_clear()
    err = None
    g, s = th.cuda.CUDAGraph(), th.cuda.Stream()
    with th.cuda.stream(s), th.cuda.graph(g, stream=s):
        try:
            drtk_amd.forward_kinematics(theta.detach()[:, 3:].view(3, 24, 3), c.detach(), parents)
        except RuntimeError as e:
            err = str(e)
    th.cuda.synchronize()
    assert err is not None and "before the capture" in err, err

    def step():
        transforms, posed = drtk_amd.forward_kinematics(theta[:, 3:].view(3, 24, 3), c, parents, tr)
        loss = (transforms * gA).sum() + (posed * gP).sum()
        loss.backward()
        return loss

    leaves = [theta, c, tr]
    cap = drtk_amd.capture_step(step, leaves)
    cap()
    th.cuda.synchronize()
    got = [cap.outputs.detach().clone()] + [x.grad.clone() for x in leaves]
    for x in leaves:
        x.grad = None
    want = [step().detach()] + [x.grad for x in leaves]
    for a, b in zip(got, want):
        assert bool(th.isfinite(a).all()) and float(a.abs().max()) > 0
        assert th.equal(a, b)


def test_pose_to_skinned_vertices_end_to_end_against_the_composed_oracles():
    """forward_kinematics -> skin -> weighted sum, backward to the pose, the rest joints and the translation"""
    import drtk_amd

    case = O.case("hand16")
    gen = th.Generator().manual_seed(77)
    V = 300
    v = th.randn(V, 3, dtype=th.float64, generator=gen).float().double()
    idx, w = drtk_amd.sparse_skin_weights(th.softmax(3 * th.randn(V, 16, dtype=th.float64, generator=gen), 1), k=4)
    w = w.float().double()
    gv = th.randn(3, V, 3, dtype=th.float64, generator=gen).float().double()

    def run(fk, skin, dtype, dev):
        leaves = [x.to(dtype).to(dev).clone().requires_grad_(True) for x in (case["rot_leaf"], case["joints_leaf"], case["translation"])]
        transforms, _ = fk(leaves[0], leaves[1], case["parents"], leaves[2])
        out = skin(v.to(dtype).to(dev), idx.to(dev), w.to(dtype).to(dev), transforms)
        grads = th.autograd.grad((out * gv.to(dtype).to(dev)).sum(), leaves)
        return [out.detach().cpu()] + [g.cpu() for g in grads]

    r64, r32 = run(O.forward_kinematics, SO.skin, th.float64, "cpu"), run(O.forward_kinematics, SO.skin, th.float32, "cpu")
    from f64_distance import assert_within_f64_distance

    for dtype in (th.float32, th.float64):
        got = run(drtk_amd.forward_kinematics, drtk_amd.skin, dtype, DEV)
        for k, (a, b64, b32) in enumerate(zip(got, r64, r32)):
            scale = float(b64.abs().max())
            err = float((a.double() - b64).abs().max())
            print(f"end to end {k} {dtype}: |hip - f64| = {err:.3e}, max|f64| = {scale:.3e}, |oracle_f32 - f64| = {float((b32.double() - b64).abs().max()):.3e}")
            if dtype == th.float64:
                assert scale > 0 and err <= 1e-12 * scale, (k, err)
            else:
                assert_within_f64_distance(a, b32, b64, f"end to end {k}")


def test_c_abi_between_sentinels_in_a_child_process():
    env = dict(os.environ, DRTK_CAPI_GUARD="1", DRTK_CAPI_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_kinematics.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cases passed" in r.stdout
