"""CPU: drtk_amd.cotangent_weights and drtk_amd.mesh_laplacian -- names and signatures, the PyTorch formulation against the
independent oracle (tests/laplacian_oracle.py) and against what the reference's hand-fitting tutorial computes
(tests/golden/laplacian_tutorial.npz, written by tests/gen_golden_laplacian.py), the operator's algebra, and the C ABI's
argument checks."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch as th
from conftest import ROOT

import laplacian_oracle as O

U32 = 2.0 ** -24


def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "laplacian_tutorial.npz"))
    return {k: th.from_numpy(z[k]) for k in z.files}


def assert_within_the_tutorial(got, d):
    """16 * 2^-24 * acc per element -- one float32 rounding for each term of the fixture's longest row (the tutorial
    stores its weights, sums of up to 14 float64 values each, in float32) -- and exactly 0 where nothing was summed."""
    got = got.detach().cpu().double()
    assert got.shape == d["lx"].shape
    err, acc = (got - d["lx"]).abs(), d["acc"]
    ratio = float((err[acc > 0] / (U32 * acc[acc > 0])).max())
    print(f"|got - tutorial| / (2^-24 acc): max {ratio:.3f}")
    assert bool((err <= 16 * U32 * acc).all()), ratio
    assert bool((acc == 0).any()) and bool((got[acc == 0] == 0).all())


def test_names_are_exported_and_stay_out_of_the_drop_in():
    import drtk
    import drtk_amd

    for n in ("cotangent_weights", "mesh_laplacian"):
        assert n in drtk_amd.__all__ and callable(getattr(drtk_amd, n))
        assert getattr(drtk_amd, n) is getattr(drtk_amd.geometry, n)
        with pytest.raises(AttributeError):
            getattr(drtk, n)


def test_signatures():
    import drtk_amd

    want = {
        drtk_amd.cotangent_weights: [("v", inspect._empty), ("vi", inspect._empty)],
        drtk_amd.mesh_laplacian: [("x", inspect._empty), ("vi", inspect._empty), ("weights", None)],
    }
    for fn, params in want.items():
        got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
        assert got == params, (fn.__name__, got)
    ops = th.ops.drtk_amd_ext
    assert str(ops.cotangent_weights.default._schema) == "drtk_amd_ext::cotangent_weights(Tensor v, Tensor vi) -> Tensor"
    assert str(ops.mesh_laplacian.default._schema) == "drtk_amd_ext::mesh_laplacian(Tensor x, Tensor vi, Tensor? weights=None) -> Tensor"
    with pytest.raises(RuntimeError, match="HIP"):
        ops.mesh_laplacian(th.zeros(1, 3, 1), th.tensor([[0, 1, 2]]), None)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.cotangent_weights(th.zeros(1, 3, 3), th.tensor([[0, 1, 2]]))


def test_a_right_isosceles_triangle():
    import drtk_amd

    v = th.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]], dtype=th.float64)
    w = drtk_amd.cotangent_weights(v, th.tensor([[0, 1, 2]]))
    assert th.equal(w, th.tensor([[[0.0, 0.5, 0.5]]], dtype=th.float64))
    w32 = drtk_amd.cotangent_weights(v.float(), th.tensor([[0, 1, 2]], dtype=th.int32))
    assert th.equal(w32, th.tensor([[[0.0, 0.5, 0.5]]]))


def test_the_formulation_matches_the_tutorial_fixture():
    import drtk_amd

    d = load_fixture()
    v, x = d["v"][None], d["x"][None]
    w = drtk_amd.cotangent_weights(v, d["vi"])
    assert th.equal(w[0, -2:], th.zeros(2, 3, dtype=th.float64))  # the duplicate-corner and the collinear face
    assert th.equal(drtk_amd.cotangent_weights(v.float(), d["vi"])[0, -2:], th.zeros(2, 3))
    assert_within_the_tutorial(drtk_amd.mesh_laplacian(x, d["vi"], w)[0], d)


def _case(n, c, seed, per_view_vi=False, degenerate=True):
    """(v [n,V,3], x [n,V,c], vi) float64: a jittered 5 x 7 grid per view, with the degenerate additions"""
    v0, vi = O.grid_mesh(5, 7, seed)
    if degenerate:
        v0, vi = O.with_degenerates(v0, vi)
    g = th.Generator().manual_seed(seed)
    v = v0[None] + 0.05 * th.randn(n, *v0.shape, dtype=th.float64, generator=g)
    if degenerate:
        v[:, -3:] = v0[-3:]  # the collinear face keeps its integer coordinates
    x = th.randn(n, v0.shape[0], c, dtype=th.float64, generator=g)
    if per_view_vi:  # the same faces, listed in another order and from another corner (the degenerate ones stay last)
        k = vi.shape[0] - (2 if degenerate else 0)
        vi = th.stack([th.cat([vi[:k].roll(i, 0).roll(i, 1), vi[k:]]) for i in range(n)])
    return v, x, vi


@pytest.mark.parametrize("idx_dtype", [th.int32, th.int64])
@pytest.mark.parametrize("n,c,per_view_vi", [(1, 1, False), (3, 3, False), (2, 4, True), (3, 5, True)])
def test_the_formulation_matches_the_oracle_with_its_gradients(n, c, per_view_vi, idx_dtype):
    import drtk_amd

    v, x, vi = _case(n, c, 11 + n + c, per_view_vi)
    g = th.randn(x.shape, dtype=th.float64, generator=th.Generator().manual_seed(5))

    def run(cot, lap, vi):
        vv, xx = v.clone().requires_grad_(True), x.clone().requires_grad_(True)
        w = cot(vv, vi)
        w.retain_grad()
        out = lap(xx, vi, w)
        (out * g).sum().backward()
        return w.detach(), out.detach(), xx.grad, w.grad, vv.grad, lap(x, vi, None)

    got = run(drtk_amd.cotangent_weights, drtk_amd.mesh_laplacian, vi.to(idx_dtype))
    want = run(O.cot_weights, O.mesh_laplacian, vi)
    for name, a, b in zip(("weights", "out", "grad_x", "grad_w", "grad_v", "uniform"), got, want):
        assert a.shape == b.shape and float(b.abs().max()) > 0
        err = float((a - b).abs().max())
        assert err <= 1e-12 * max(1.0, float(b.abs().max())), (name, err)
    assert th.equal(got[0][:, -2:], th.zeros(n, 2, 3, dtype=th.float64))
    assert th.equal(got[4][:, -3:], th.zeros(n, 3, 3, dtype=th.float64))  # a degenerate face gives v no gradient
    assert th.equal(got[1][:, -4], th.zeros(n, c, dtype=th.float64))      # the unreferenced vertex


def test_shared_and_per_view_weights_broadcast_independently_of_vi():
    import drtk_amd

    v, x, vi = _case(3, 3, 21)
    w = O.cot_weights(v, vi)
    for vi_l in (vi, vi[None], vi[None].expand(3, -1, -1), vi[None].repeat(3, 1, 1)):
        for w_l, w_ref in ((w[0], w[:1]), (w[:1], w[:1]), (w, w)):
            wl = w_l.clone().requires_grad_(True)
            wr = w_ref.clone().requires_grad_(True)
            a, b = drtk_amd.mesh_laplacian(x, vi_l, wl), O.mesh_laplacian(x, vi, wr)
            assert float((a - b).detach().abs().max()) <= 1e-12 * float(b.detach().abs().max())
            a.square().sum().backward()
            b.square().sum().backward()
            assert wl.grad.shape == w_l.shape
            assert float((wl.grad.reshape(wr.shape) - wr.grad).abs().max()) <= 1e-12 * float(wr.grad.abs().max())


def test_symmetric_and_constants_map_to_zero():
    import drtk_amd

    v, x, vi = _case(2, 3, 31)
    w = drtk_amd.cotangent_weights(v, vi)
    g = th.randn(x.shape, dtype=th.float64, generator=th.Generator().manual_seed(6))
    for weights in (w, None):
        a = (g * drtk_amd.mesh_laplacian(x, vi, weights)).sum((1, 2))
        b = (drtk_amd.mesh_laplacian(g, vi, weights) * x).sum((1, 2))
        scale = (g.abs() * O.accumulated(x, vi, weights)).sum((1, 2))
        assert bool(((a - b).abs() <= 1e-14 * scale).all())
        # constants: every bracket is w * (c - c) + w * (c - c), exactly 0 for any finite weights
        const = th.full_like(x, 1.7)
        assert th.equal(drtk_amd.mesh_laplacian(const, vi, weights), th.zeros_like(x))
    # the uniform weights make an interior manifold edge total 1: an interior grid vertex of valence 6 has row sum 6
    v0, vi0 = O.grid_mesh(5, 7, 0)
    onehot = th.zeros(1, v0.shape[0], 1, dtype=th.float64)
    onehot[0, 8] = 1
    col = drtk_amd.mesh_laplacian(onehot, vi0)[0, :, 0]
    assert float(col[8]) == -6.0 and sorted(col[col > 0].tolist()) == [1.0] * 6 and float(col.sum()) == 0.0


def test_other_dtypes_take_the_formulation():
    import drtk_amd

    v, x, vi = _case(1, 3, 41)
    w = drtk_amd.cotangent_weights(v.half(), vi)
    assert w.dtype == th.float16 and bool(th.isfinite(w).all())
    assert drtk_amd.mesh_laplacian(x.bfloat16(), vi).dtype == th.bfloat16


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    z, nz = ctypes.c_void_p(0), ctypes.c_void_p(16)
    i64 = ctypes.c_int64
    out = ctypes.c_size_t(0)
    wsb = L.drtk_amd_geometry_laplacian_workspace_bytes
    assert wsb(ctypes.c_int(0), i64(8), i64(1), i64(5), i64(3), ctypes.byref(out)) == 0 and out.value == 8 * 5 * 3 * 4
    assert wsb(ctypes.c_int(1), i64(8), i64(8), i64(5), i64(2), ctypes.byref(out)) == 0 and out.value == 5 * 2 * 8
    assert wsb(ctypes.c_int(0), i64(8), i64(3), i64(5), i64(3), ctypes.byref(out)) == -1  # B is 1 or N
    assert wsb(ctypes.c_int(2), i64(8), i64(1), i64(5), i64(3), ctypes.byref(out)) == -1  # dtype
    assert wsb(ctypes.c_int(0), i64(8), i64(1), i64(5), i64(0), ctypes.byref(out)) == -1  # C >= 1

    def cot(fn=L.drtk_amd_geometry_cot_weights, dtype=0, N=1, V=3, F=1, v_sN=9, vi_sN=0, v=nz, out=nz, extra=()):
        return fn(ctypes.c_int(dtype), v, i64(v_sN), nz, i64(vi_sN), i64(N), i64(V), i64(F), *extra, out, z)
    for kw in ({}, {"fn": L.drtk_amd_geometry_cot_weights_backward, "extra": (nz,)}):
        assert cot(dtype=2, **kw) == -1 and cot(dtype=-1, **kw) == -1
        assert cot(N=-1, **kw) == -1 and cot(V=-1, **kw) == -1 and cot(F=-1, **kw) == -1
        assert cot(v_sN=7, **kw) == -1 and cot(vi_sN=5, **kw) == -1
        assert cot(v=z, **kw) == -1 and cot(out=z, **kw) == -1 and cot(V=0, v_sN=0, **kw) == -1
        assert cot(N=0, **kw) == 0 and cot(F=0, out=z, **kw) == 0  # nothing to do: no launch, NULL output allowed
    assert cot(fn=L.drtk_amd_geometry_cot_weights_backward, extra=(z,)) == -1  # no upstream gradient

    def lap(dtype=0, C=3, vi_sN=0, w=z, w_sN=0, nch=0, B=1, N=1, V=3, F=1, x=nz, out=nz, ws=z, wsb=0):
        return L.drtk_amd_geometry_laplacian(ctypes.c_int(dtype), x, i64(C), nz, i64(vi_sN), w, i64(w_sN), nz, nz, nz, nz, nz,
                                             i64(nch), i64(B), i64(N), i64(V), i64(F), out, ws, ctypes.c_size_t(wsb), z)
    assert lap(dtype=2) == -1 and lap(C=0) == -1
    assert lap(N=-1) == -1 and lap(V=-1) == -1 and lap(F=-1) == -1 and lap(nch=-1) == -1
    assert lap(vi_sN=5) == -1 and lap(w=nz, w_sN=2) == -1 and lap(w_sN=3) == -1  # weight stride without weights
    assert lap(N=2, B=3) == -1                        # B is 1 or N
    assert lap(N=2, B=2, vi_sN=0) == -1 and lap(N=2, B=1, vi_sN=3) == -1  # vi is the incidence's topology
    assert lap(x=z) == -1 and lap(out=z) == -1
    assert lap(nch=2) == -2                           # chunks need a workspace ...
    assert lap(nch=2, ws=nz, wsb=2 * 3 * 4 - 1) == -2  # ... of the full size
    assert lap(N=0, out=z) == 0 and lap(V=0, out=z) == 0  # N * V == 0: nothing to do

    def gw(dtype=0, C=3, vi_sN=0, N=1, V=3, F=1, wB=1, g=nz, out=nz):
        return L.drtk_amd_geometry_laplacian_grad_weights(ctypes.c_int(dtype), g, nz, i64(C), nz, i64(vi_sN), i64(N), i64(V),
                                                          i64(F), i64(wB), out, z)
    assert gw(dtype=2) == -1 and gw(C=0) == -1 and gw(N=-1) == -1 and gw(F=-1) == -1 and gw(vi_sN=4) == -1
    assert gw(N=3, wB=2) == -1 and gw(g=z) == -1 and gw(out=z) == -1 and gw(V=0) == -1
    assert gw(F=0, out=z) == 0 and gw(N=0, wB=0, out=z) == 0
