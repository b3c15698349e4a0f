"""GPU: drtk_amd.cotangent_weights and drtk_amd.mesh_laplacian on the HIP route (csrc/geometry.hip through the drtk_amd_ext
operators and through the C ABI) -- forward and all three gradients against the independent float64 oracle
(tests/laplacian_oracle.py) on its structural cases, the tutorial fixture, every layout of vi and weights, views and
non-contiguous inputs, which kernels a backward launches, errors, bitwise reproducibility, graph capture, the tutorial's
regulariser end to end, and the C ABI between sentinel elements (tests/guarded_laplacian.py in a child process)."""
import os
import subprocess
import sys

import pytest
import torch as th
from conftest import ROOT

import laplacian_oracle as O
from f64_distance import assert_within_f64_distance
from test_laplacian_host import assert_within_the_tutorial, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("weights", "out", "grad_x", "grad_w", "grad_v")


def hip_pipeline(v, x, grad, vi, api="ops"):
    """O.pipeline on the device: through the package (`ops`) or composed from the C ABI's entry points (`capi`: int32
    topology, the numpy incidence) the way csrc/torch_ops/geometry.cpp composes them.  Tensors on the CPU."""
    import drtk_amd
    from drtk_amd import capi

    v, x, grad, vi = v.to(DEV), x.to(DEV), grad.to(DEV), vi.to(DEV)
    if api == "ops":
        res = O.pipeline(drtk_amd.cotangent_weights, drtk_amd.mesh_laplacian, v, x, grad, vi)
    else:
        V = v.shape[1]
        vi32 = vi.to(th.int32)
        inc = capi.vertex_incidence_numpy(vi.cpu().numpy(), V)
        w = capi.geometry_cot_weights(v, vi32)
        gw = capi.geometry_laplacian_grad_weights(grad, x, vi32)
        rows = capi.geometry_cot_weights_backward(v, vi32, gw)
        res = {"weights": w, "out": capi.geometry_laplacian(x, vi32, inc, w),
               "grad_x": capi.geometry_laplacian(grad, vi32, inc, w), "grad_w": gw,
               "grad_v": capi.geometry_vertex_gather(rows, inc, V, per_corner=True)[0]}
    return {k: t.detach().cpu() for k, t in res.items()}


def check_case(name, dtype, api="ops"):
    """float64: 1e-12 of each result's scale from the oracle; float32: within the project's float64-distance bound,
    max(1e-5 max|f64|, 3 |oracle_f32 - f64|), the oracles on the float32 inputs."""
    return check_inputs(*O.case(name), dtype, api, name, degenerate=name.startswith("degenerate"))


def check_inputs(v, x, grad, vi, dtype, api, name, degenerate=False):
    """check_case on any inputs of O.case / O.build_case (shared with tests/fuzz_added_ops.py)."""
    v, x, grad = v.to(dtype), x.to(dtype), grad.to(dtype)
    got = hip_pipeline(v, x, grad, vi, api)
    r64 = O.reference(v, x, grad, vi, th.float64)
    r32 = O.reference(v, x, grad, vi, th.float32) if dtype == th.float32 else None
    compare(got, r64, r32, dtype, name)
    if degenerate:
        n = v.shape[0]
        assert th.equal(got["weights"][:, -2:], th.zeros(n, 2, 3, dtype=dtype))  # duplicate-corner and collinear face
        assert th.equal(got["grad_v"][:, -3:], th.zeros(n, 3, 3, dtype=dtype))   # which give v no gradient
        assert th.equal(got["out"][:, -4], th.zeros(n, x.shape[2], dtype=dtype))  # the unreferenced vertex
    return got


def compare(got, r64, r32, dtype, name):
    """Every result the float64 oracle `r64` has, under the two bounds of check_case (`r32`: the float32 oracle, or None)."""
    for k in r64:
        assert got[k].dtype == dtype and got[k].shape == r64[k].shape, (name, k)
        assert float(r64[k].abs().max()) > 0, (name, k)
        err = float((got[k].double() - r64[k]).abs().max())
        print(f"{name} {k} {dtype}: |hip - f64| = {err:.3e}, max|f64| = {float(r64[k].abs().max()):.3e}")
        if dtype == th.float64:
            assert err <= 1e-12 * float(r64[k].abs().max()), (name, k, err)
        else:
            assert_within_f64_distance(got[k], r32[k], r64[k], f"{name} {k}")


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("name", list(O.CASES))
def test_forward_and_all_gradients_match_the_oracle(name, dtype):
    check_case(name, dtype)


@pytest.mark.parametrize("name", ["soup257_c5_n3", "degenerate_per_view", "fan600_shared", "fan300_per_view"])
def test_c_abi_gives_the_operators_results_bit_for_bit(name):
    for dtype in (th.float32, th.float64):
        a, b = check_case(name, dtype, "ops"), check_case(name, dtype, "capi")
        for k in KEYS:
            assert th.equal(a[k], b[k]), (name, dtype, k)


def test_the_tutorial_fixture_on_float64():
    import drtk_amd

    d = load_fixture()
    v, x, vi = d["v"][None].to(DEV), d["x"][None].to(DEV), d["vi"].to(DEV)
    w = drtk_amd.cotangent_weights(v, vi)
    assert th.equal(w[0, -2:], th.zeros(2, 3, dtype=th.float64, device=DEV))
    assert_within_the_tutorial(drtk_amd.mesh_laplacian(x, vi, w)[0], d)


def test_no_faces_and_no_views():
    import drtk_amd

    e = th.zeros(0, 3, dtype=th.int32, device=DEV)
    x = th.randn(2, 5, 3, device=DEV).requires_grad_(True)
    w = drtk_amd.cotangent_weights(x, e)
    assert w.shape == (2, 0, 3)
    out = drtk_amd.mesh_laplacian(x, e, w)
    assert th.equal(out, th.zeros(2, 5, 3, device=DEV))
    out.sum().backward()
    assert th.equal(x.grad, th.zeros_like(x))
    assert th.equal(drtk_amd.mesh_laplacian(x.detach(), e), th.zeros(2, 5, 3, device=DEV))
    vi = th.tensor([[0, 1, 2], [2, 1, 3]], device=DEV)
    x0 = th.zeros(0, 4, 3, device=DEV, dtype=th.float64).requires_grad_(True)
    w0 = drtk_amd.cotangent_weights(x0, vi)
    assert w0.shape == (0, 2, 3)
    shared = th.ones(2, 3, device=DEV, dtype=th.float64, requires_grad=True)
    for weights in (w0, shared, None):
        out = drtk_amd.mesh_laplacian(x0, vi, weights)
        assert out.shape == (0, 4, 3)
        out.sum().backward()
    assert x0.grad.shape == (0, 4, 3) and th.equal(shared.grad, th.zeros_like(shared))  # the empty sum over no views


VI_LAYOUTS = ("F3", "1F3", "NF3")
W_LAYOUTS = ("none", "F3", "1F3", "NF3", "NF3_expand")


@pytest.mark.parametrize("w_layout", W_LAYOUTS)
@pytest.mark.parametrize("vi_layout", VI_LAYOUTS)
def test_every_layout_of_vi_and_weights_through_ops_and_capi(vi_layout, w_layout):
    """Every layout, either index dtype and both precisions: the output and the gradients against the oracle (1e-12 in
    float64, the float64-distance bound in float32), int32 and int64 indices bitwise equal, the C ABI bitwise equal to the
    operators; the weights' gradient has the shape of the weights as they were passed (shared: summed over the views)."""
    import drtk_amd
    from drtk_amd import capi

    v, x, grad, vi = O.case("degenerate_shared")
    N, V = x.shape[:2]
    w_all = O.cot_weights(v, vi)
    vi_l = {"F3": vi, "1F3": vi[None], "NF3": vi[None].repeat(N, 1, 1)}[vi_layout]
    # (applied where the weights live: a copy to the device would make an expanded tensor contiguous)
    w_of = {"none": lambda w: None, "F3": lambda w: w[0], "1F3": lambda w: w[:1], "NF3": lambda w: w,
            "NF3_expand": lambda w: w[:1].expand(N, -1, -1)}[w_layout]
    for dtype in (th.float32, th.float64):
        xs, gs = x.to(dtype), grad.to(dtype)
        ws = w_all.to(dtype)

        def run(lap, dt, dev, vi_x):
            xx = xs.to(dt).to(dev).clone().requires_grad_(True)
            ww = w_of(ws.to(dt).to(dev))
            if ww is not None:
                ww = ww.detach().requires_grad_(True)
                assert (ww.stride(0) == 0) == (w_layout == "NF3_expand")
            out = lap(xx, vi_x.to(dev), ww)
            out.backward(gs.to(dt).to(dev))
            return [out.detach().cpu(), xx.grad.cpu()] + ([] if ww is None else [ww.grad.cpu()])

        got = run(drtk_amd.mesh_laplacian, dtype, DEV, vi_l)
        assert all(th.equal(a, b) for a, b in zip(got, run(drtk_amd.mesh_laplacian, dtype, DEV, vi_l.int())))
        r64 = run(O.mesh_laplacian, th.float64, "cpu", vi_l)
        r32 = run(O.mesh_laplacian, th.float32, "cpu", vi_l)
        for what, a, b32, b64 in zip(("out", "grad_x", "grad_w"), got, r32, r64):
            assert a.shape == b64.shape and a.dtype == dtype, (what, a.shape, b64.shape)
            if dtype == th.float64:
                assert float((a - b64).abs().max()) <= 1e-12 * float(b64.abs().max()), what
            else:
                assert_within_f64_distance(a, b32, b64, f"{vi_layout} {w_layout} {what}")
        # the C ABI on the same data: shared weights are [1,F,3] there, an expanded tensor is N rows like any other
        xd, gd = xs.to(DEV), gs.to(DEV)
        vi32 = vi_l.to(DEV).int()
        inc = capi.vertex_incidence_numpy(vi_l.numpy(), V)
        wd = w_of(ws.to(DEV))
        assert th.equal(capi.geometry_laplacian(xd, vi32, inc, wd).cpu(), got[0])
        assert th.equal(capi.geometry_laplacian(gd, vi32, inc, wd).cpu(), got[1])
        if wd is not None:
            gw = capi.geometry_laplacian_grad_weights(gd, xd, vi32, shared_weights=w_layout in ("F3", "1F3"))
            assert th.equal(gw.cpu().reshape(got[2].shape), got[2])
        assert capi.check_guards() >= 0


def _weighted_sum(o):
    return (o * th.cos(th.arange(o.numel(), dtype=o.dtype, device=o.device) * 0.37).view_as(o)).sum()


@pytest.mark.parametrize("need", [(True, True, True), (True, False, False), (False, True, False), (False, False, True)])
def test_views_and_non_contiguous_inputs_get_the_requested_gradients(need):
    """x a transposed view, v an expanded view of one shared mesh, the weights a column slice: the gradient reaches every
    leaf that requires it and no other, equal in float64 to the PyTorch formulation's on the CPU."""
    import drtk_amd

    v0, _, _, vi = O.case("degenerate_shared")
    N, V, F = 3, v0.shape[1], vi.shape[0]
    gen = th.Generator().manual_seed(17)
    leaves = (th.randn(N, 5, V, dtype=th.float64, generator=gen), v0[0].clone(), th.rand(N, F, 5, dtype=th.float64, generator=gen))

    def grads(dev):
        xt, vs, w5 = (t.to(dev).clone().requires_grad_(r) for t, r in zip(leaves, need))
        x, v, w = xt.transpose(1, 2), vs[None].expand(N, -1, -1), w5[..., 1:4]
        assert not (x.is_contiguous() or v.is_contiguous() or w.is_contiguous())
        loss = _weighted_sum(drtk_amd.mesh_laplacian(x, vi.to(dev), w))
        loss = loss + _weighted_sum(drtk_amd.mesh_laplacian(x.detach(), vi.to(dev), drtk_amd.cotangent_weights(v, vi.to(dev))))
        want = [t for t in (xt, vs, w5) if t.requires_grad]
        return [g.cpu() for g in th.autograd.grad(loss, want)]

    got, ref = grads(DEV), grads("cpu")
    assert len(got) == sum(need)
    for a, b in zip(got, ref):
        assert float(b.abs().max()) > 0 and a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())


def test_a_backward_launches_only_the_kernels_of_the_requested_gradients():
    """The timing report lists the library's launches: the vertex kernel runs again in the backward only for grad_x, the
    weights' face pass only for grad_weights, and the cotangent backward (face pass + vertex gather) only for grad_v."""
    import drtk_amd
    from drtk_amd import capi

    v, x, grad, vi = (t.to(DEV) for t in O.case("degenerate_shared"))

    def launches(need_x, need_w, need_v):
        xx, vv = x.clone().requires_grad_(need_x), v.clone().requires_grad_(need_v)
        w = drtk_amd.cotangent_weights(vv, vi)
        if need_w:
            w = w.detach().requires_grad_(True)
        th.cuda.synchronize()
        capi.kernel_timing_begin()
        out = drtk_amd.mesh_laplacian(xx, vi, w)
        if out.requires_grad:
            out.backward(grad)
        th.cuda.synchronize()
        rep = capi.kernel_timing_report()
        count = lambda name: sum(n for k, (n, _) in rep.items() if k.split("<")[0] == name)  # noqa: E731
        return tuple(count(k) for k in ("laplacian_vertex_kernel", "laplacian_grad_weights_kernel",
                                        "cot_weights_face_backward_kernel", "geom_vertex_gather_kernel"))

    assert launches(False, False, False) == (1, 0, 0, 0)
    assert launches(True, False, False) == (2, 0, 0, 0)
    assert launches(False, True, False) == (1, 1, 0, 0)
    assert launches(False, False, True) == (1, 1, 1, 1)
    assert launches(True, True, False) == (2, 1, 0, 0)


def test_errors_out_of_range_index_double_backward_and_shapes():
    import drtk_amd

    v, x, _, vi = (t.to(DEV) for t in O.case("degenerate_shared"))
    V = v.shape[1]
    bad = vi.clone()
    bad[3, 1] = V
    for fn in (lambda: drtk_amd.mesh_laplacian(x, bad), lambda: drtk_amd.cotangent_weights(v, bad),
               lambda: drtk_amd.mesh_laplacian(x, -1 - vi)):
        with pytest.raises(RuntimeError, match="outside"):
            fn()
    with pytest.raises(RuntimeError, match="weights of shape"):
        drtk_amd.mesh_laplacian(x, vi, th.ones(2, vi.shape[0], 3, dtype=x.dtype, device=DEV))
    with pytest.raises(RuntimeError, match=r"\[N, V, C\]"):
        drtk_amd.mesh_laplacian(x[0], vi)
    vv, xx = v.clone().requires_grad_(True), x.clone().requires_grad_(True)
    w = drtk_amd.cotangent_weights(vv, vi)
    ww = w.detach().requires_grad_(True)
    for out, wrt in ((w, vv), (drtk_amd.mesh_laplacian(xx, vi, ww), xx), (drtk_amd.mesh_laplacian(xx, vi, ww), ww),
                     (drtk_amd.mesh_laplacian(xx, vi), xx)):
        with pytest.raises(RuntimeError, match="double backward"):
            th.autograd.grad(out.square().sum(), wrt, create_graph=True)
        (g,) = th.autograd.grad(out.square().sum(), wrt)  # a plain backward still works
        assert bool(th.isfinite(g).all())


def test_bitwise_reproducible_cold_and_warm_and_grad_x_is_the_operator():
    import drtk_amd
    import drtk_amd.geometry as G

    for name in ("fan600_shared", "fan600_per_view", "soup257_c5_n3"):
        v, x, grad, vi = (t.float().to(DEV) if t.is_floating_point() else t.to(DEV) for t in O.case(name))

        def run():
            return hip_pipeline(v, x, grad, vi)

        G.geometry_cache_clear()
        a = run()
        assert G.geometry_cache_stats()[1] == 1
        G.geometry_cache_clear()
        b = run()
        c = run()
        for k in KEYS:
            assert th.equal(a[k], b[k]) and th.equal(a[k], c[k]), (name, k)
        w = a["weights"].to(DEV)
        assert th.equal(drtk_amd.mesh_laplacian(grad, vi, w).cpu(), a["grad_x"]), name
        xx = x.clone().requires_grad_(True)
        drtk_amd.mesh_laplacian(xx, vi).backward(grad)
        assert th.equal(xx.grad, drtk_amd.mesh_laplacian(grad, vi)), name


def test_graph_capture_replay_equals_eager_and_a_cold_cache_raises():
    import drtk_amd
    import drtk_amd.geometry as G

    v0, x0, _, vi = (t.float().to(DEV) if t.is_floating_point() else t.to(DEV) for t in O.case("fan300_shared"))
    v = v0.clone().requires_grad_(True)

    def step():
        w = drtk_amd.cotangent_weights(v, vi)
        out = drtk_amd.mesh_laplacian(v - v0 + x0[..., :3], vi, w)
        (out.square().mean((1, 2)).sum() + drtk_amd.mesh_laplacian(v, vi).square().sum()).backward()
        return out

    G.geometry_cache_clear()
    err = None
    g, s = th.cuda.CUDAGraph(), th.cuda.Stream()
    with th.cuda.stream(s), th.cuda.graph(g, stream=s):
        try:
            drtk_amd.mesh_laplacian(x0, vi)
        except RuntimeError as e:
            err = str(e)
    th.cuda.synchronize()
    assert err is not None and "before the capture" in err, err
    cap = drtk_amd.capture_step(step, [v])
    cap()
    th.cuda.synchronize()
    got = (cap.outputs.detach().clone(), v.grad.clone())
    v.grad = None
    want = step()
    assert bool(th.isfinite(got[1]).all()) and float(got[1].abs().max()) > 0
    assert th.equal(got[0], want.detach()) and th.equal(got[1], v.grad)


def test_the_tutorials_regulariser_end_to_end_on_a_sphere():
    """loss = l_w * mesh_laplacian(v - v0, vi, cotangent_weights(v0, vi).detach()).square().mean((1, 2)) on a 32 x 32
    sphere, 2 views, backward to v: loss and gradient against the oracle."""
    import drtk_amd

    s0, vi = O.sphere_mesh(32, 32)
    gen = th.Generator().manual_seed(23)
    v0 = th.stack([s0, 1.3 * s0 + 0.1]) + 0.003 * th.randn(2, *s0.shape, dtype=th.float64, generator=gen)
    v = v0 + 0.02 * th.randn(v0.shape, dtype=th.float64, generator=gen)
    l_w = 40.0

    def run(cot, lap, dtype, dev):
        a, b = v.to(dtype).to(dev).clone().requires_grad_(True), v0.to(dtype).to(dev)
        w = cot(b, vi.to(dev)).detach()
        loss = l_w * lap(a - b, vi.to(dev), w).square().mean((1, 2))
        loss.sum().backward()
        return loss.detach().cpu(), a.grad.cpu()

    v, v0 = v.float().double(), v0.float().double()  # one set of inputs, exact in either precision
    r64, r32 = run(O.cot_weights, O.mesh_laplacian, th.float64, "cpu"), run(O.cot_weights, O.mesh_laplacian, th.float32, "cpu")
    got64 = run(drtk_amd.cotangent_weights, drtk_amd.mesh_laplacian, th.float64, DEV)
    got32 = run(drtk_amd.cotangent_weights, drtk_amd.mesh_laplacian, th.float32, DEV)
    for what, a64, a32, b32, b64 in zip(("loss", "grad_v"), got64, got32, r32, r64):
        assert float(b64.abs().max()) > 0
        assert float((a64 - b64).abs().max()) <= 1e-12 * float(b64.abs().max()), what
        assert_within_f64_distance(a32, b32, b64, what)


def test_c_abi_between_sentinels_in_a_child_process():
    env = dict(os.environ, DRTK_CAPI_GUARD="1", DRTK_CAPI_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guarded_laplacian.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "cases passed" in r.stdout
