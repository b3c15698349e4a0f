"""GPU: drtk_amd.skin on the HIP route (csrc/skin.hip through drtk_amd_ext::skin and through the C ABI) -- forward and all
three gradients against the independent dense oracle (tests/skin_oracle.py) on its structural cases and 40 seeded shapes,
the C ABI, either index dtype, cold and warm cache bit for bit, the launches of each gradient combination, non-contiguous
inputs, errors, graph capture, and the C ABI between sentinel elements (tests/guarded_skin.py in a child process)."""
import importlib
import os
import subprocess
import sys

import pytest
import torch as th
from conftest import ROOT

import skin_oracle as O
from f64_distance import assert_within_f64_distance
from test_skin_host import assert_exact_zeros

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("out", "grad_v", "grad_w", "grad_t")
ALL = ("v", "weights", "transforms")


def hip_results(inputs, dtype, api="ops", grads=ALL, idx_dtype=th.int64):
    """O.results on the device: through the package (`ops`) or through the C ABI's two entry points (`capi`: int32 indices,
    the numpy incidence) the way csrc/torch_ops/skin.cpp calls them.  Tensors on the CPU; with `capi`, only `grads`."""
    import drtk_amd
    from drtk_amd import capi

    v, idx, w, t, grad = inputs
    if api == "ops":
        assert grads == ALL
        return O.results(drtk_amd.skin, v, idx.to(idx_dtype), w, t, grad, dtype, DEV)
    expanded = v.dim() == 3 and v.shape[0] > 1 and v.stride(0) == 0
    vd = (v[:1] if expanded else v).to(dtype).to(DEV)
    td = (t if t.is_contiguous() else t._base).to(dtype).to(DEV)
    tv = td if t.is_contiguous() else td[..., :3, :]
    idx32, wd, gd = idx.to(DEV).int(), w.to(dtype).to(DEV), grad.to(dtype).to(DEV)
    inc = capi.joint_incidence_numpy(idx.numpy(), t.shape[1])
    res = {"out": capi.skin_forward(vd, idx32, wd, tv)}
    # an expanded v gets one gradient row per view, which autograd's expand then sums
    gv, gw, gt = capi.skin_backward(gd, vd, idx32, wd, tv, inc, grads=grads, sum_views=False if expanded else None)
    if gv is not None:
        res["grad_v"] = (gv.sum(0, keepdim=True) if expanded else gv).view(vd.shape)
    if gw is not None:
        res["grad_w"] = gw
    if gt is not None:
        if not t.is_contiguous():
            full = th.zeros_like(td)
            full[..., :3, :] = gt
            gt = full
        res["grad_t"] = gt
    return {k: x.detach().cpu() for k, x in res.items()}


def compare(got, r64, r32, dtype, what):
    """float64: 1e-12 of each result's scale from the float64 oracle; float32: within the project's float64-distance bound,
    max(1e-5 max|f64|, 3 |oracle_f32 - f64|), the oracles run on the float32 inputs."""
    for k in KEYS:
        assert got[k].dtype == dtype and got[k].shape == r64[k].shape, (what, k, got[k].shape, r64[k].shape)
        scale = float(r64[k].abs().max())
        assert scale > 0, (what, k)
        err = float((got[k].double() - r64[k]).abs().max())
        print(f"{what} {k} {dtype}: |hip - f64| = {err:.3e}, max|f64| = {scale:.3e}")
        if dtype == th.float64:
            assert err <= 1e-12 * scale, (what, k, err)
        else:
            assert_within_f64_distance(got[k], r32[k], r64[k], f"{what} {k}")


def check_key(key, dtype, api="ops"):
    inputs = O.case(key) if isinstance(key, str) else O.build_case(key)
    got = hip_results(inputs, dtype, api)
    compare(got, O.reference(key, th.float64), O.reference(key, th.float32) if dtype == th.float32 else None, dtype, str(key))
    assert_exact_zeros(got, inputs[1], inputs[3], key)
    return got


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("key", list(O.CASES) + list(O.SEEDS))
def test_forward_and_all_gradients_match_the_oracle(key, dtype):
    check_key(key, dtype)


@pytest.mark.parametrize("key", list(O.CASES) + [3, 17, 29])
def test_c_abi_and_int32_indices_give_the_operators_results_bit_for_bit(key):
    inputs = O.case(key) if isinstance(key, str) else O.build_case(key)
    for dtype in (th.float32, th.float64):
        a = hip_results(inputs, dtype, "ops")
        b = hip_results(inputs, dtype, "capi")
        c = hip_results(inputs, dtype, "ops", idx_dtype=th.int32)
        for k in KEYS:
            assert th.equal(a[k], b[k]), (key, dtype, k, "capi")
            assert th.equal(a[k], c[k]), (key, dtype, k, "int32")


def test_no_views_and_no_vertices():
    import drtk_amd

    idx = th.tensor([[0, 1], [1, -1], [2, 2], [0, 0]], device=DEV)
    w = th.ones(4, 2, dtype=th.float64, device=DEV, requires_grad=True)
    v = th.randn(1, 4, 3, dtype=th.float64, device=DEV, requires_grad=True)
    t0 = th.zeros(0, 3, 4, 4, dtype=th.float64, device=DEV, requires_grad=True)
    out = drtk_amd.skin(v, idx, w, t0)
    assert out.shape == (0, 4, 3)
    out.sum().backward()
    assert th.equal(w.grad, th.zeros_like(w)) and th.equal(v.grad, th.zeros_like(v)) and t0.grad.shape == (0, 3, 4, 4)  # empty sums
    t = th.randn(2, 3, 3, 4, device=DEV, requires_grad=True)
    v0 = th.zeros(2, 0, 3, device=DEV, requires_grad=True)
    w0 = th.zeros(0, 2, device=DEV, requires_grad=True)
    out = drtk_amd.skin(v0, th.zeros(0, 2, dtype=th.int32, device=DEV), w0, t)
    assert out.shape == (2, 0, 3)
    out.sum().backward()
    assert th.equal(t.grad, th.zeros_like(t)) and v0.grad.shape == (2, 0, 3) and w0.grad.shape == (0, 2)


def test_bitwise_reproducible_cold_and_warm():
    S = importlib.import_module("drtk_amd.skin")
    for name in ("chunked", "k8_slots", "shared_v"):
        for dtype in (th.float32, th.float64):
            S.skin_cache_clear()
            a = hip_results(O.case(name), dtype)
            assert S.skin_cache_stats()[1] == 1  # one build per index tensor
            S.skin_cache_clear()
            b = hip_results(O.case(name), dtype)
            c = hip_results(O.case(name), dtype)
            for k in KEYS:
                assert th.equal(a[k], b[k]) and th.equal(a[k], c[k]), (name, dtype, k)
    # one index tensor, used twice: a hit; edited in place: a miss
    import drtk_amd

    v, idx, w, t, _ = (x.to(DEV) for x in O.case("block_edge"))
    S.skin_cache_clear()
    first = drtk_amd.skin(v, idx, w, t)
    assert th.equal(drtk_amd.skin(v, idx, w, t), first) and S.skin_cache_stats()[:2] == (1, 1)
    idx[0, 0] = 2
    drtk_amd.skin(v, idx, w, t)
    assert S.skin_cache_stats()[:2] == (1, 2)
    crow, entries = S.joint_incidence(idx, t.shape[1])
    assert crow.shape == (t.shape[1] + 1,) and int(crow[-1]) == idx.numel() and S.skin_cache_stats()[0] == 2


@pytest.mark.parametrize("need", [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                  (True, True, False), (True, False, True), (False, True, True), (True, True, True)])
def test_a_backward_launches_only_the_kernels_of_the_requested_gradients(need):
    """One launch forward; one vertex pass for grad_v and / or grad_weights; a chunk pass and a sum for grad_transforms."""
    import drtk_amd
    from drtk_amd import capi

    v, idx, w, t, grad = (x.float().to(DEV) if x.is_floating_point() else x.to(DEV) for x in O.case("chunked"))
    drtk_amd.skin(v, idx, w, t)  # (the incidence build is not a launch of the library, but keep it out of the collection)
    vv, ww, tt = (x.clone().requires_grad_(r) for x, r in zip((v, w, t), need))
    th.cuda.synchronize()
    capi.kernel_timing_begin()
    out = drtk_amd.skin(vv, idx, ww, tt)
    if out.requires_grad:
        out.backward(grad)
    th.cuda.synchronize()
    rep = capi.kernel_timing_report()
    assert all(k.startswith("skin_") for k in rep), rep
    count = lambda name: sum(n for k, (n, _) in rep.items() if k.split("<")[0] == name)  # noqa: E731
    got = tuple(count(k) for k in ("skin_forward_kernel", "skin_vertex_backward_kernel", "skin_joint_chunk_kernel", "skin_joint_sum_kernel"))
    assert got == (1, int(need[0] or need[1]), int(need[2]), int(need[2])), (need, rep)
    if need[0] or need[1]:
        (name,) = [k for k in rep if k.startswith("skin_vertex_backward_kernel")]
        flags = [a.strip() for a in name.split("<")[1].rstrip(">").split(",")]
        assert flags[2:] == [str(need[0]).lower(), str(need[1]).lower()], name
    for x, r in zip((vv, ww, tt), need):
        assert (x.grad is not None) == r


def _weighted_sum(o):
    return (o * th.cos(th.arange(o.numel(), dtype=o.dtype, device=o.device) * 0.37).view_as(o)).sum()


@pytest.mark.parametrize("need", [(True, True, True), (True, False, False), (False, True, False), (False, False, True)])
def test_non_contiguous_inputs_get_the_requested_gradients(need):
    """v a transposed view, the weights a column slice, the indices a column slice, the transforms a [..., :3, :] view of a
    strided 4x4 tensor: the gradient reaches every leaf that requires it and no other, as the oracle's does on the CPU."""
    import drtk_amd

    gen = th.Generator().manual_seed(31)
    N, V, J, K = 3, 140, 6, 3
    leaves = (th.randn(N, 3, V, dtype=th.float64, generator=gen), th.rand(V, K + 2, dtype=th.float64, generator=gen),
              th.randn(N, J, 2, 4, 4, dtype=th.float64, generator=gen))
    idx5 = th.randint(-1, J, (V, K + 2), generator=gen)

    def grads(fn, dev):
        vt, w5, t5 = (x.to(dev).clone().requires_grad_(r) for x, r in zip(leaves, need))
        v, w, idx, t = vt.transpose(1, 2), w5[:, 1:K + 1], idx5.to(dev)[:, 1:K + 1], t5[:, :, 1, :3, :]
        assert not (v.is_contiguous() or w.is_contiguous() or idx.is_contiguous() or t.is_contiguous())
        loss = _weighted_sum(fn(v, idx, w, t))
        return [g.cpu() for g in th.autograd.grad(loss, [x for x in (vt, w5, t5) if x.requires_grad])]

    got, ref = grads(drtk_amd.skin, DEV), grads(O.skin, "cpu")
    assert len(got) == sum(need)
    for a, b in zip(got, ref):
        assert float(b.abs().max()) > 0 and a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_errors():
    import drtk_amd

    v, idx, w, t, grad = (x.to(DEV) for x in O.case("block_edge"))
    J = t.shape[1]
    one_bad = idx.clone()
    one_bad[7, 1] = J
    for bad in (one_bad, idx - 2, idx.int() + J):
        with pytest.raises(RuntimeError, match="outside"):
            drtk_amd.skin(v, bad, w, t)
    with pytest.raises((RuntimeError, ValueError), match="K = 9"):
        drtk_amd.skin(v, idx[:, :1].expand(-1, 9).contiguous(), w[:, :1].expand(-1, 9).contiguous(), t)
    with pytest.raises(RuntimeError, match="K = 9"):
        th.ops.drtk_amd_ext.skin(v, idx[:, :1].expand(-1, 9).contiguous(), w[:, :1].expand(-1, 9).contiguous(), t)
    for args in ((v, idx, w.float(), t), (v, idx, w, t.float()), (v.float(), idx, w, t)):
        with pytest.raises(TypeError, match="dtype of v"):
            drtk_amd.skin(*args)
        with pytest.raises(RuntimeError, match="dtype of v"):
            th.ops.drtk_amd_ext.skin(*args)
    for args in ((v, idx.cpu(), w, t), (v, idx, w.cpu(), t), (v, idx, w, t.cpu())):
        with pytest.raises(ValueError, match="on the device of v"):
            drtk_amd.skin(*args)
        with pytest.raises(RuntimeError):
            th.ops.drtk_amd_ext.skin(*args)
    with pytest.raises(RuntimeError, match="HIP"):
        th.ops.drtk_amd_ext.skin(v.cpu(), idx.cpu(), w.cpu(), t.cpu())
    for args in ((v[..., :2], idx, w, t), (v, idx[:-1], w[:-1], t), (v, idx, w[:, :2], t), (v, idx, w, t[0]), (v[:2], idx, w, t),
                 (v, idx, w, t[..., :3]), (v, idx.double(), w, t)):
        with pytest.raises((ValueError, TypeError), match="expected"):
            drtk_amd.skin(*args)
        with pytest.raises(RuntimeError, match="expected"):
            th.ops.drtk_amd_ext.skin(*args)
    vv, ww, tt = (x.clone().requires_grad_(True) for x in (v, w, t))
    for wrt in (vv, ww, tt):
        out = drtk_amd.skin(vv, idx, ww, tt)
        with pytest.raises(RuntimeError, match="double backward"):
            th.autograd.grad(out.square().sum(), wrt, create_graph=True)
        (g,) = th.autograd.grad(drtk_amd.skin(vv, idx, ww, tt).square().sum(), wrt)  # a plain backward still works
        assert bool(th.isfinite(g).all())


def test_a_capture_on_a_cold_cache_raises_and_a_captured_step_replays_the_eager_bits():
    import drtk_amd
    from drtk_amd.synthetic import ring_cameras, uv_sphere

    S = importlib.import_module("drtk_amd.skin")
    gen = th.Generator().manual_seed(41)
    v0, vi = uv_sphere(24, 32, device=DEV)
    V, N, J, K = v0.shape[-2], 2, 5, 4
    rest = v0.reshape(1, V, 3)
    idx = th.randint(0, J, (V, K), generator=gen).to(DEV)
    w = th.softmax(th.randn(V, K, generator=gen), 1).to(DEV).requires_grad_(True)
    t = (th.eye(4)[:3] + 0.05 * th.randn(N, J, 3, 4, generator=gen)).to(DEV).requires_grad_(True)
    vr = rest.clone().requires_grad_(True)
    cams = ring_cameras(N, 64, 64, device=DEV)

    S.skin_cache_clear()
    err = None
    g, s = th.cuda.CUDAGraph(), th.cuda.Stream()
    with th.cuda.stream(s), th.cuda.graph(g, stream=s):
        try:
            drtk_amd.skin(rest, idx, w.detach(), t.detach())
        except RuntimeError as e:
            err = str(e)
    th.cuda.synchronize()
    assert err is not None and "before the capture" in err, err

    def step():
        posed = drtk_amd.skin(vr, idx, w, t)
        normals = drtk_amd.vert_normals(posed, vi)
        v_pix = drtk_amd.transform(posed, *cams)
        loss = v_pix.square().mean() + (normals * posed).sum(-1).square().mean()
        loss.backward()
        return loss

    leaves = [vr, w, t]
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


def test_c_abi_between_sentinels_in_a_child_process():
    env = dict(os.environ, DRTK_CAPI_GUARD="1", DRTK_CAPI_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_skin.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cases passed" in r.stdout
