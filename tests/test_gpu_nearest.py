"""GPU: drtk_amd.nearest_points on the HIP route (csrc/nearest.hip through drtk_amd_ext::nearest_points and through the C ABI)
-- the forward bit for bit against the independent oracle (tests/nearest_oracle.py) on its structural cases and 40 seeded
shapes, ties, rejected candidates, both gradients against the float64 oracle, bitwise reproducibility and the stability of
the sort, the C ABI, strided inputs read in place, empty shapes, errors, graph capture, chamfer_distance, and the C ABI
between sentinel elements (tests/guarded_nearest.py in a child process)."""
import os
import subprocess
import sys

import pytest
import torch as th
from conftest import ROOT

import nearest_oracle as O
from f64_distance import assert_within_f64_distance
from test_nearest_host import assert_exact_zeros

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRADS = ("grad_p", "grad_q")
KEYS = ("dist2", "idx") + GRADS


def hip_results(inputs, dtype, api="ops", grads=("p", "q"), order=None):
    """O.results on the device: through the package (`ops`) or through the C ABI's two entry points (`capi`: int32 indices,
    a stable sort made with torch on the CPU unless `order` is given).  Tensors on the CPU; with `capi`, only `grads`."""
    import drtk_amd
    from drtk_amd import capi

    p, q, g = inputs
    if api == "ops":
        assert grads == ("p", "q") and order is None
        return O.results(drtk_amd.nearest_points, p, q, g, dtype, DEV)
    expanded = lambda x: x.dim() == 3 and x.shape[0] > 1 and x.stride(0) == 0  # noqa: E731

    def on_device(x):  # (leaf, the tensor to pass): a stride-0 expand is rebuilt on the device from its one row
        leaf = (x[:1] if expanded(x) else x).to(dtype).to(DEV)
        return leaf, (leaf.expand(x.shape[0], -1, -1) if expanded(x) else leaf)

    (pl, pd), (ql, qd) = on_device(p), on_device(q)
    dist2, idx = capi.nearest_forward(pd, qd)
    assert idx.dtype == th.int32
    res = {"dist2": dist2, "idx": idx.long()}
    if order is None:
        order = th.sort(idx.cpu(), dim=1, stable=True).indices
    gp, gq = capi.nearest_backward(g.to(dtype).to(DEV), pd, qd, idx, order.to(DEV), grads=grads)
    # an expanded input gets one gradient row per view, which autograd's expand then sums
    if gp is not None:
        res["grad_p"] = (gp.sum(0, keepdim=True) if expanded(p) else gp).view(pl.shape)
    if gq is not None:
        res["grad_q"] = (gq.sum(0, keepdim=True) if expanded(q) else gq).view(ql.shape)
    return {k: x.detach().cpu() for k, x in res.items()}


def compare(got, key, dtype, what):
    """Forward: th.equal.  Gradients, float64: 1e-12 of each result's scale from the float64 oracle; float32: within the
    project's float64-distance bound, max(1e-5 max|f64|, 3 |oracle_f32 - f64|), the oracles run on the float32 inputs."""
    ref = O.reference(key, dtype)
    assert got["dist2"].dtype == dtype and got["idx"].dtype == th.int64
    assert th.equal(got["idx"], ref["idx"]), (what, "idx", int((got["idx"] != ref["idx"]).sum()))
    assert th.equal(got["dist2"], ref["dist2"]), (what, "dist2")
    for k in GRADS:
        if k not in got:
            continue
        r64 = ref[k]
        assert got[k].dtype == dtype and got[k].shape == r64.shape, (what, k, got[k].shape, r64.shape)
        scale = float(r64.abs().max())
        assert scale > 0 or key in O.ALL_ZERO, (what, k)
        err = float((got[k].double() - r64).abs().max())
        print(f"{what} {k} {dtype}: |hip - f64| = {err:.3e}, max|f64| = {scale:.3e}")
        if dtype == th.float64:
            assert err <= 1e-12 * scale, (what, k, err)
        else:
            assert_within_f64_distance(got[k], ref[k + "_own"], r64, f"{what} {k}")
    if all(k in got for k in GRADS):
        assert_exact_zeros(got, ref, what)


def check_key(key, dtype, api="ops"):
    inputs = O.case(key) if isinstance(key, str) else O.build_case(key)
    got = hip_results(inputs, dtype, api)
    compare(got, key, dtype, str(key))
    return got


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("key", list(O.CASES) + list(O.SEEDS))
def test_forward_bit_for_bit_and_both_gradients_match_the_oracle(key, dtype):
    check_key(key, dtype)


@pytest.mark.parametrize("key", list(O.CASES) + [3, 17, 29])
def test_c_abi_gives_the_operators_results_bit_for_bit(key):
    """... with int32 indices on the C side and a stable sort made on the CPU: the shim's device sort is stable too"""
    inputs = O.case(key) if isinstance(key, str) else O.build_case(key)
    for dtype in (th.float32, th.float64):
        a = hip_results(inputs, dtype, "ops")
        b = hip_results(inputs, dtype, "capi")
        for k in KEYS:
            assert th.equal(a[k], b[k]), (key, dtype, k)


@pytest.mark.parametrize("key", ["all_one_target", "runs_end_on_chunk_edges", "minus_one_front", "shared_q", "shared_p", 5])
def test_bitwise_reproducible_and_each_gradient_alone_has_the_same_bits(key):
    inputs = O.case(key) if isinstance(key, str) else O.build_case(key)
    for dtype in (th.float32, th.float64):
        a = hip_results(inputs, dtype)
        b = hip_results(inputs, dtype)
        c = hip_results(inputs, dtype, "capi")
        for k in KEYS:
            assert th.equal(a[k], b[k]) and th.equal(a[k], c[k]), (key, dtype, k)
        for grads, k in ((("p",), "grad_p"), (("q",), "grad_q")):
            one = hip_results(inputs, dtype, "capi", grads=grads)
            assert set(one) == {"dist2", "idx", k} and th.equal(one[k], a[k]), (key, dtype, k)


def test_the_operator_requests_only_what_requires_grad():
    import drtk_amd
    from drtk_amd import capi

    p, q, g = (x.float().to(DEV) for x in O.case("runs_end_on_chunk_edges"))
    full = hip_results(O.case("runs_end_on_chunk_edges"), th.float32)
    for need in ((True, False), (False, True), (True, True), (False, False)):
        pp, qq = p.clone().requires_grad_(need[0]), q.clone().requires_grad_(need[1])
        th.cuda.synchronize()
        capi.kernel_timing_begin()
        d, i = drtk_amd.nearest_points(pp, qq)
        if d.requires_grad:
            d.backward(g)
        th.cuda.synchronize()
        rep = capi.kernel_timing_report()
        count = lambda name: sum(n for k, (n, _) in rep.items() if name in k)  # noqa: E731
        got = tuple(count(k) for k in ("nearest_forward_kernel", "nearest_grad_p_kernel", "nearest_grad_q_chunk_kernel", "nearest_grad_q_target_kernel"))
        assert got == (1, int(need[0]), int(need[1]), int(need[1])), (need, rep)
        assert (pp.grad is not None) == need[0] and (qq.grad is not None) == need[1] and not i.requires_grad
        if need[0]:
            assert th.equal(pp.grad.cpu(), full["grad_p"])
        if need[1]:
            assert th.equal(qq.grad.cpu(), full["grad_q"])


def test_the_sort_must_be_stable_and_the_shims_is():
    """The sum of a target's terms runs in sorted order, so `order` must be THE stable sort: the C ABI with the CPU's stable
    sort gives the operator's bits (above and here), and any stable order of the same keys is that one order.  An unstable
    order of equal keys is a different summation order: the result stays within rounding of the oracle, not bitwise."""
    inputs = O.case("all_one_target")
    a = hip_results(inputs, th.float32)
    idx = a["idx"]
    stable = th.sort(idx.int(), dim=1, stable=True).indices
    # equal keys in ascending i, every view: what stability means here
    keys = th.gather(idx, 1, stable)
    same = keys[:, 1:] == keys[:, :-1]
    assert bool((stable[:, 1:][same] > stable[:, :-1][same]).all()) and bool((keys[:, 1:] >= keys[:, :-1]).all())
    b = hip_results(inputs, th.float32, "capi", order=stable)
    assert th.equal(a["grad_q"], b["grad_q"])
    reverse = stable.flip(1)  # every key equal here: still sorted, not stable
    c = hip_results(inputs, th.float32, "capi", order=reverse)
    ref = O.reference("all_one_target", th.float32)
    assert_within_f64_distance(c["grad_q"], ref["grad_q_own"], ref["grad_q"], "reversed order")
    assert th.equal(c["grad_p"], a["grad_p"])


def test_empty_shapes():
    import drtk_amd

    for dtype in (th.float32, th.float64):
        p = th.randn(2, 5, 3, dtype=dtype, device=DEV, requires_grad=True)
        q0 = th.zeros(2, 0, 3, dtype=dtype, device=DEV, requires_grad=True)
        d, i = drtk_amd.nearest_points(p, q0)  # M = 0: no candidate
        assert d.shape == (2, 5) and bool(th.isinf(d).all()) and bool((i == -1).all()) and i.dtype == th.int64
        gp, gq = th.autograd.grad(d, (p, q0), th.ones_like(d))
        assert th.equal(gp, th.zeros_like(p)) and gq.shape == (2, 0, 3)
        p0 = th.zeros(2, 0, 3, dtype=dtype, device=DEV, requires_grad=True)
        q = th.randn(1, 7, 3, dtype=dtype, device=DEV, requires_grad=True)
        d, i = drtk_amd.nearest_points(p0, q)  # P = 0
        assert d.shape == (2, 0) and i.shape == (2, 0)
        gp, gq = th.autograd.grad(d, (p0, q), th.ones_like(d))
        assert gp.shape == (2, 0, 3) and th.equal(gq, th.zeros_like(q))
        pn = th.zeros(0, 4, 3, dtype=dtype, device=DEV, requires_grad=True)
        q1 = th.randn(7, 3, dtype=dtype, device=DEV, requires_grad=True)
        d, i = drtk_amd.nearest_points(pn, q1.expand(0, 7, 3))  # N = 0
        assert d.shape == (0, 4) and i.shape == (0, 4)
        gp, gq = th.autograd.grad(d, (pn, q1), th.ones_like(d))
        assert gp.shape == (0, 4, 3) and th.equal(gq, th.zeros_like(q1))


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_strided_inputs_are_read_in_place_and_match_the_contiguous_copy(dtype):
    """p the positions of an [N,P,6] positions-plus-normals tensor, q the positions of every second view of an [2N,M,4] one"""
    import drtk_amd

    gen = th.Generator().manual_seed(77)
    n, num_p, num_q = 2, O.QUERIES + 90, O.TILE + 333
    p6 = th.randn(n, num_p, 6, dtype=dtype, generator=gen).to(DEV).requires_grad_(True)
    q4 = th.randn(2 * n, num_q, 4, dtype=dtype, generator=gen).to(DEV).requires_grad_(True)
    g = th.randn(n, num_p, dtype=dtype, generator=gen).to(DEV)
    p, q = p6[..., :3], q4[::2, :, :3]
    assert not p.is_contiguous() and not q.is_contiguous()
    d, i = drtk_amd.nearest_points(p, q)
    gp6, gq4 = th.autograd.grad(d, (p6, q4), g)
    pc, qc = p.detach().contiguous().requires_grad_(True), q.detach().contiguous().requires_grad_(True)
    dc, ic = drtk_amd.nearest_points(pc, qc)
    gpc, gqc = th.autograd.grad(dc, (pc, qc), g)
    assert th.equal(d, dc) and th.equal(i, ic)
    assert th.equal(gp6[..., :3], gpc) and th.equal(gp6[..., 3:], th.zeros_like(gp6[..., 3:]))
    assert th.equal(gq4[::2, :, :3], gqc) and th.equal(gq4[1::2], th.zeros_like(gq4[1::2])) and float(gqc.abs().max()) > 0
    ref_d, ref_i = O.nearest(pc.detach().cpu(), qc.detach().cpu())
    assert th.equal(d.cpu(), ref_d) and th.equal(i.cpu(), ref_i)
    # a transposed tensor (points not 3 consecutive elements) is copied, with the same result
    pt = pc.detach().transpose(1, 2).contiguous().transpose(1, 2)
    assert not pt.is_contiguous()
    dt, it = drtk_amd.nearest_points(pt, qc.detach())
    assert th.equal(dt, dc) and th.equal(it, ic)


def test_errors():
    import drtk_amd

    p, q = th.zeros(2, 5, 3, device=DEV), th.zeros(2, 7, 3, device=DEV)
    for args in ((p[..., :2], q), (p, q[0, 0]), (p, th.zeros(3, 7, 3, device=DEV)), (p[None], q)):
        with pytest.raises(ValueError, match="expected"):
            drtk_amd.nearest_points(*args)
        with pytest.raises(RuntimeError, match="expected"):
            th.ops.drtk_amd_ext.nearest_points(*args)
    with pytest.raises(TypeError, match="dtype of p"):
        drtk_amd.nearest_points(p, q.double())
    with pytest.raises(RuntimeError, match="dtype of p"):
        th.ops.drtk_amd_ext.nearest_points(p, q.double())
    with pytest.raises(ValueError, match="on the device of p"):
        drtk_amd.nearest_points(p, q.cpu())
    with pytest.raises(RuntimeError):
        th.ops.drtk_amd_ext.nearest_points(p, q.cpu())
    with pytest.raises(RuntimeError, match="HIP"):
        th.ops.drtk_amd_ext.nearest_points(p.cpu(), q.cpu())
    with pytest.raises(RuntimeError, match="not implemented for"):
        th.ops.drtk_amd_ext.nearest_points(p.half(), q.half())
    pp, qq = th.randn(2, 50, 3, device=DEV, requires_grad=True), th.randn(2, 70, 3, device=DEV, requires_grad=True)
    for wrt in (pp, qq):
        d, _ = drtk_amd.nearest_points(pp, qq)
        with pytest.raises(RuntimeError, match="double backward"):
            th.autograd.grad(d.sum(), wrt, create_graph=True)
        (g,) = th.autograd.grad(drtk_amd.nearest_points(pp, qq)[0].sum(), wrt)  # a plain backward still works
        assert bool(th.isfinite(g).all())


def test_graph_capture_replays_the_eager_bits_on_changed_inputs():
    """Forward and backward to both inputs inside torch.cuda.graph (the sort included: no host read), replayed twice on
    changed inputs; S > 1 on this shape."""
    import drtk_amd

    gen = th.Generator().manual_seed(9)
    n, num_p, num_q = 2, 700, 2 * O.TILE + 50
    assert O.split(n, num_p, num_q)[0] > 1
    data = [(th.randn(n, num_p, 3, generator=gen), th.randn(n, num_q, 3, generator=gen), th.randn(n, num_p, generator=gen)) for _ in range(3)]
    data[2][0][:, :300] = data[2][1][:, 5:6] + 0.01 * data[2][0][:, :300]  # a long run on the last replay
    p = data[0][0].to(DEV).requires_grad_(True)
    q = data[0][1].to(DEV).requires_grad_(True)
    g = data[0][2].to(DEV)

    def step():
        d, i = drtk_amd.nearest_points(p, q)
        d.backward(g)
        return d, i

    cap = drtk_amd.capture_step(step, [p, q])  # warms the op up on a side stream, then captures there
    for pd, qd, gd in data[1:]:
        with th.no_grad():
            p.copy_(pd.to(DEV))
            q.copy_(qd.to(DEV))
            g.copy_(gd.to(DEV))
        cap()
        th.cuda.synchronize()
        got = [cap.outputs[0].detach().clone(), cap.outputs[1].clone(), p.grad.clone(), q.grad.clone()]
        p.grad = q.grad = None
        d, i = step()
        want = [d.detach(), i, p.grad, q.grad]
        for a, b in zip(got, want):
            assert th.equal(a, b) and bool(th.isfinite(a.double()).all()) and float(a.double().abs().max()) > 0
        ref_d, ref_i = O.nearest(pd, qd)
        assert th.equal(got[0].cpu(), ref_d) and th.equal(got[1].cpu(), ref_i)
        p.grad = q.grad = None


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_chamfer_distance_against_its_definition(dtype):
    import drtk_amd

    gen = th.Generator().manual_seed(13)
    x = th.randn(3, 500, 3, dtype=dtype, generator=gen)
    y = th.randn(3, O.TILE + 77, 3, dtype=dtype, generator=gen)
    x[1, 4] = float("nan")
    xw = th.rand(3, 500, dtype=dtype, generator=gen)
    xw[2] = 0
    yw = th.rand(3, y.shape[1], generator=gen) < 0.5
    # the distances are the oracle's bits; what differs is the order of the means' sums (about a thousand non-negative terms):
    # 1e-12 in float64, the project's 1e-5 of the result in float32
    tol = 1e-12 if dtype == th.float64 else 1e-5
    for kw in ({}, {"squared": False}, {"bidirectional": False}, {"x_weights": xw, "y_weights": yw}, {"x_weights": xw, "y_weights": yw, "squared": False}):
        want = O.chamfer(x.double(), y.double(), **kw) if dtype == th.float64 else O.chamfer(x, y, **kw).double()
        got = drtk_amd.chamfer_distance(x.to(DEV), y.to(DEV), **{k: (v.to(DEV) if th.is_tensor(v) else v) for k, v in kw.items()})
        assert got.dtype == dtype and got.shape == () and abs(float(got) - float(want)) <= tol * float(want), (kw, float(got), float(want))
    # differentiable on the device, finite with an all-zero weight row and a NaN point
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    drtk_amd.chamfer_distance(xd, yd, x_weights=xw.to(DEV), y_weights=yw.to(DEV), squared=False).backward()
    assert bool(th.isfinite(xd.grad).all()) and bool(th.isfinite(yd.grad).all()) and float(yd.grad.abs().max()) > 0
    assert th.equal(xd.grad[1, 4], th.zeros(3, dtype=dtype, device=DEV))
    # y shared by the views: the same on both routes as its copies
    a = drtk_amd.chamfer_distance(x.nan_to_num(0.0).to(DEV), y[0].to(DEV))
    b = drtk_amd.chamfer_distance(x.nan_to_num(0.0).to(DEV), y[:1].expand(3, -1, -1).contiguous().to(DEV))
    assert th.equal(a, b)


def test_c_abi_between_sentinels_in_a_child_process():
    env = dict(os.environ, DRTK_CAPI_GUARD="1", DRTK_CAPI_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_nearest.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cases passed" in r.stdout
