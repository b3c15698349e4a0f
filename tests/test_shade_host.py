"""CPU: drtk_amd.shade without a GPU -- the public surface (signature, export, operator schema, dispatch keys), every
ValueError before anything else happens, CPU tensors failing loudly, the C ABI's argument / workspace statuses with null or
dummy pointers and its workspace size against the kernel's constants, and the oracle's own checks (tests/shade_oracle.py):
it equals the tutorial's literal formulation, passes gradcheck, its cases keep their margins and shares, and a view left
out of a many-slot case is far outside the tolerance the GPU test uses."""
import ctypes
import inspect
import os
import re

import pytest
import torch as th

import shade_oracle as O
from f64_distance import f64_distance_bound

ARGS = ["normal_img", "light_dir", "albedo", "ambient", "index_img", "pos_img", "specular", "shininess", "background", "gamma"]


def test_python_signature_export_and_docstring():
    import drtk_amd

    E = inspect.Parameter.empty
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.shade).parameters.values()]
    assert got == [(a, E if i < 4 else None) for i, a in enumerate(ARGS)]
    assert "shade" in drtk_amd.__all__ and drtk_amd.shade.__module__ == "drtk_amd.shade"
    doc = drtk_amd.shade.__doc__
    for word in ("-(n . L) > 0", "-(h . n) > 1e-8", "exactly 0", "1e-12", "Double backward is not"):
        assert word in doc, word
    import drtk

    assert not hasattr(drtk, "shade")  # the drop-in keeps the reference's surface


def test_operator_schema_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    schema = ("drtk_amd_ext::shade(Tensor normal_img, Tensor light_dir, Tensor albedo, Tensor ambient, Tensor? index_img, "
              "Tensor? pos_img, Tensor? specular, Tensor? shininess, Tensor? background, float? gamma) -> Tensor")
    assert str(th.ops.drtk_amd_ext.shade.default._schema) == schema
    for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
        assert th._C._dispatch_has_kernel_for_dispatch_key("drtk_amd_ext::shade", key), key


def test_c_abi_names_are_declared_and_bound():
    from conftest import ROOT
    from drtk_amd import capi

    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    for name in ("drtk_amd_shade_workspace_bytes", "drtk_amd_shade_forward", "drtk_amd_shade_backward"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    assert callable(capi.shade_forward) and callable(capi.shade_backward)


def _cpu_args(N=2, C=3, H=4, W=5, dtype=th.float32):
    return dict(normal_img=th.randn(N, 3, H, W, dtype=dtype), light_dir=th.randn(3, dtype=dtype), albedo=th.rand(C, dtype=dtype),
                ambient=th.rand(C, dtype=dtype), index_img=th.zeros(N, H, W, dtype=th.int32), pos_img=th.randn(N, 3, H, W, dtype=dtype),
                specular=th.rand(N, C, dtype=dtype), shininess=th.rand(1, dtype=dtype) + 1, background=th.rand(N, C, H, W, dtype=dtype),
                gamma=2.2)


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    a = _cpu_args()
    for drop in ((), ("specular", "shininess", "pos_img"), ("index_img", "background", "gamma")):
        kw = {k: v for k, v in a.items() if k not in drop}
        with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
            drtk_amd.shade(**kw)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        drtk_amd.shade(**{k: (v.double() if th.is_tensor(v) and v.is_floating_point() else v) for k, v in a.items()})
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.shade_forward(**a)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.shade_backward(th.zeros(2, 3, 4, 5), **a)


BAD_CALLS = {
    "specular without pos_img": dict(pos_img=None),
    "specular without shininess": dict(shininess=None),
    "C = 0": dict(ambient=th.rand(0), albedo=th.rand(0), specular=None),
    "C = 5": dict(ambient=th.rand(5), albedo=th.rand(5), specular=None, background=None),
    "ambient [1, 1, C]": dict(ambient=th.rand(1, 1, 3)),
    "normal_img with 4 channels": dict(normal_img=th.randn(2, 4, 4, 5)),
    "pos_img of another N": dict(pos_img=th.randn(3, 3, 4, 5)),
    "pos_img of another H": dict(pos_img=th.randn(2, 3, 5, 5)),
    "background of another C": dict(background=th.rand(2, 4, 4, 5)),
    "background of another W": dict(background=th.rand(2, 3, 4, 6)),
    "albedo image of another C": dict(albedo=th.rand(2, 2, 4, 5)),
    "albedo of another C": dict(albedo=th.rand(4)),
    "albedo of another N": dict(albedo=th.rand(3, 3)),
    "light_dir [2]": dict(light_dir=th.randn(2)),
    "light_dir [N, 3, 1]": dict(light_dir=th.randn(2, 3, 1)),
    "specular [N + 1, C]": dict(specular=th.rand(3, 3)),
    "shininess [2]": dict(shininess=th.rand(2)),
    "shininess scalar": dict(shininess=th.rand(())),
    "index_img int64": dict(index_img=th.zeros(2, 4, 5, dtype=th.int64)),
    "index_img of another W": dict(index_img=th.zeros(2, 4, 6, dtype=th.int32)),
    "gamma 0": dict(gamma=0.0),
    "gamma negative": dict(gamma=-2.2),
    "gamma inf": dict(gamma=float("inf")),
    "gamma nan": dict(gamma=float("nan")),
}


@pytest.mark.parametrize("what", list(BAD_CALLS))
def test_value_errors_on_cpu_tensors_before_anything_else(what):
    """A bad call is a ValueError from drtk_amd/shade.py -- on CPU tensors too, so it is raised before the operator (which
    would refuse CPU tensors with a RuntimeError) is reached, let alone a launch."""
    import drtk_amd

    with pytest.raises(ValueError, match=r"shade\(\)"):
        drtk_amd.shade(**dict(_cpu_args(), **BAD_CALLS[what]))


def test_c_abi_statuses_with_null_and_dummy_pointers():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci, cd = ctypes.c_int64, ctypes.c_int, ctypes.c_double
    z, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    s3 = (ctypes.c_int64 * 3)(60, 20, 5)
    neg = (ctypes.c_int64 * 3)(60, -20, 5)

    def inputs(dtype=0, normal=p, normal_s=s3, pos=p, albedo_img=z, bg=p, index=p, light=p, l_sN=0, albedo=p, al_sN=0, ambient=p, am_sN=3,
               specular=p, sp_sN=0, shininess=p, sh_sN=0, gamma=2.2, N=2, C=3, H=4, W=5):
        return (ci(dtype), normal, normal_s, pos, s3, albedo_img, s3, bg, s3, index, s3, light, i64(l_sN), albedo, i64(al_sN), ambient,
                i64(am_sN), specular, i64(sp_sN), shininess, i64(sh_sN), cd(gamma), i64(N), i64(C), i64(H), i64(W))

    def fwd(out=p, **kw):
        return lib.drtk_amd_shade_forward(*inputs(**kw), out, z)

    def bwd(grad_out=p, gn=p, gl=p, gl_sN=0, ws=p, nbytes=1 << 30, **kw):
        a = inputs(**kw)
        return lib.drtk_amd_shade_backward(a[0], grad_out, *a[1:], gn, z, z, z, gl, i64(gl_sN), z, i64(0), z, i64(0), z, i64(0), z, i64(0),
                                           ws, ctypes.c_size_t(nbytes), z)

    # judged before any pointer is looked at (every pointer here is a dummy: a status other than these would be a fault)
    for f in (fwd, bwd):
        assert f(dtype=2) == -1 and f(dtype=-1) == -1
        assert f(C=0) == -1 and f(C=5) == -1
        assert f(N=-1) == -1 and f(H=-1) == -1 and f(H=1 << 16, W=1 << 15) == -1
        assert f(gamma=-1.0) == -1 and f(gamma=float("nan")) == -1 and f(gamma=float("inf")) == -1
        assert f(N=0) == 0 and f(H=0) == 0  # nothing to do, nothing launched
        assert f(normal=z) == -1 and f(light=z) == -1 and f(ambient=z) == -1
        assert f(normal_s=neg) == -1
        assert f(albedo=z) == -1 and f(albedo_img=p) == -1  # neither, and both
        assert f(pos=z) == -1 and f(shininess=z) == -1  # specular needs them
        assert f(l_sN=2) == -1 and f(am_sN=2) == -1 and f(al_sN=1) == -1 and f(sp_sN=4) == -1 and f(sh_sN=3) == -1
    assert fwd(out=z) == -1
    assert bwd(grad_out=z) == -1
    assert bwd(gl_sN=2) == -1
    # the workspace: alignment before size, both before the first launch
    assert bwd(ws=z) == -1
    assert bwd(ws=odd, nbytes=1 << 30) == -1 and bwd(ws=odd, nbytes=0) == -1
    assert bwd(ws=p, nbytes=0) == -2
    need = capi.shade_workspace_bytes(th.float32, 2, 4, 5)
    assert bwd(ws=p, nbytes=need - 1) == -2
    # a gradient of something that was not given
    a = inputs(specular=z, pos=z, shininess=z)
    assert lib.drtk_amd_shade_backward(a[0], p, *a[1:], z, p, z, z, z, i64(0), z, i64(0), z, i64(0), z, i64(0), z, i64(0), z,
                                       ctypes.c_size_t(0), z) == -1
    # nothing wanted: nothing launched
    assert bwd(gn=z, gl=z, ws=z, nbytes=0) == 0
    o = ctypes.c_size_t(0)
    assert lib.drtk_amd_shade_workspace_bytes(ci(0), i64(2), i64(4), i64(5), None) == -1
    assert lib.drtk_amd_shade_workspace_bytes(ci(3), i64(2), i64(4), i64(5), ctypes.byref(o)) == -1
    assert lib.drtk_amd_shade_workspace_bytes(ci(0), i64(-2), i64(4), i64(5), ctypes.byref(o)) == -1


def test_workspace_bytes_is_the_slot_count_of_the_kernels_constants():
    from drtk_amd import capi

    P, B, S, terms = O.kernel_constants()
    assert terms == 16 and S >= 2 and all(B[dt] == 256 * P[dt] for dt in P) and P[th.float32] * 4 == 16 == P[th.float64] * 8
    for dt in P:
        for N, H, W in ((1, 1, 1), (2, 1, B[dt]), (3, B[dt] + 1, 1), (2, 7, 293), (5, 33, 31), (65537, 1, 2)):
            rows = -(-H * W // B[dt])
            assert capi.shade_workspace_bytes(dt, N, H, W) == N * (rows + 1) * terms * 8, (dt, N, H, W)
    # the slot cases hold the row counts they are named after, in the precision they are named after
    for dt, tag in ((th.float32, "f32"), (th.float64, "f64")):
        for name, rows in (("S", S), ("S+1", S + 1), ("2S+1", 2 * S + 1)):
            c = O.CASES[f"rows_{name}_{tag}"]
            assert -(-c["H"] * c["W"] // B[dt]) == rows and c["W"] % 2 == 1
    sizes = {O.CASES[k]["H"] * O.CASES[k]["W"] for k in O.CASES if k.startswith("plane")}
    for dt in P:
        assert {1, P[dt] - 1, P[dt], P[dt] + 1, B[dt] - 1, B[dt], B[dt] + 1, 2 * B[dt] + 3} <= sizes
    assert all(O.CASES[k]["W"] % 2 == 1 for k in O.CASES)
    assert {O.CASES[k]["N"] for k in O.CASES} >= {1, 2, 3} and {O.CASES[k]["C"] for k in O.CASES} >= {1, 3, 4}
    for key in ("index", "specular", "background", "albedo_img"):
        assert {bool(O.CASES[k][key]) for k in O.CASES} == {False, True}, key
    assert {O.CASES[k]["gamma"] for k in O.CASES} == {None, 2.2}
    for param in O.PARAMS:
        assert {param in O.CASES[k]["per_view"] for k in O.CASES} == {False, True}, param


def test_oracle_equals_the_tutorials_literal_formulation():
    """On a margin case (finite inputs, nothing at a clamp) the select and the blend, and the where-clamps and clamp(), agree."""
    inp, _ = O.case("per_view_all")
    gloss = inp["shininess"] / 40
    want = O.tutorial_shade(inp["normal_img"], inp["light_dir"], inp["albedo"], inp["ambient"], inp["index_img"], inp["pos_img"],
                            inp["specular"], gloss, inp["background"])
    got = O.shade(**dict(inp, shininess=gloss * 40))
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


def test_oracle_passes_gradcheck_on_3_x_3():
    g = th.Generator().manual_seed(5)
    r = lambda *s: th.rand(*s, generator=g, dtype=th.float64)  # noqa: E731
    n = (r(2, 3, 3, 3) - 0.5).requires_grad_(True)
    pos = (r(2, 3, 3, 3) - 0.5).requires_grad_(True)
    light = th.tensor([0.3, -0.5, 0.8], dtype=th.float64, requires_grad=True)
    alb, amb, spec = ((0.1 + r(*s)).requires_grad_(True) for s in ((2, 3, 3, 3), (2, 3), (3,)))
    shin = th.tensor([[3.0], [7.5]], dtype=th.float64, requires_grad=True)
    bg = (0.1 + r(2, 3, 3, 3)).requires_grad_(True)
    idx = th.tensor([[[0, -1, 2], [3, 4, -1], [-1, 7, 8]], [[1, 1, -1], [-1, 2, 2], [5, -1, 0]]], dtype=th.int32)
    cat = O.categories(dict(normal_img=n.detach(), light_dir=light.detach(), pos_img=pos.detach(), specular=spec, index_img=idx))
    assert float(cat["ndl"].abs().min()) > 1e-3 and float(cat["hn"].abs().min()) > 1e-3  # away from the kinks
    f = lambda n, light, alb, amb, pos, spec, shin, bg: O.shade(n, light, alb, amb, idx, pos, spec, shin, bg, 2.2)  # noqa: E731
    assert th.autograd.gradcheck(f, (n, light, alb, amb, pos, spec, shin, bg), eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", list(O.CASES))
def test_every_case_keeps_its_margins_and_shares(name):
    inp, grad_out = O.case(name)
    again, _ = O.case(name)
    c = O.CASES[name]
    for k, t in inp.items():
        if th.is_tensor(t):
            assert th.equal(t, again[k]), k  # deterministic
            if t.is_floating_point():
                assert t.dtype == th.float64 and th.equal(t, t.float().double()), k  # float32 numbers
    cat = O.categories(inp)
    assert float(cat["ndl"].abs().min()) >= O.MARGIN
    assert float(inp["normal_img"].norm(dim=1).min()) >= 0.1 and float(inp["light_dir"].norm(dim=-1).min()) >= 0.1
    for k in ("albedo", "ambient", "background", "specular"):
        if inp[k] is not None:
            assert float(inp[k].min()) >= 0.05, k
    if c["specular"]:
        assert float(cat["hn"].abs().min()) >= O.MARGIN and float(cat["hv"].min()) >= 0.1
        assert float(inp["pos_img"].norm(dim=1).min()) >= 0.1
    value = O.shade(**dict(inp, gamma=None))
    assert float(value[(cat["fg"][:, None]).expand_as(value)].min()) >= 1e-3
    if c["N"] * c["H"] * c["W"] >= 64:
        for k, share in O.shares(inp).items():
            assert share >= 0.1, (k, share)
    assert grad_out.shape == (c["N"], c["C"], c["H"], c["W"]) and float(grad_out.abs().max()) > 0.5
    for param in O.PARAMS:
        if inp[param] is not None and inp[param].ndim < 4:
            assert inp[param].ndim == (2 if param in c["per_view"] else 1), param


def test_a_view_left_out_of_a_many_slot_case_moves_each_parameter_gradient_by_100_tolerances():
    """What the GPU test's float32 bound (tests/f64_distance.py with the accumulated magnitude) can see: in a case whose
    views fill more than one pass of the finalize kernel, the last view's share of every shared parameter's gradient is
    more than 100 bounds."""
    inp, grad_out = O.case("rows_S_f64")
    assert O.CASES["rows_S_f64"]["per_view"] == () and O.CASES["rows_S_f64"]["N"] == 2
    r64, r32 = O.reference(inp, grad_out, th.float64), O.reference(inp, grad_out, th.float32)
    first = {k: (v[:1] if th.is_tensor(v) and v.ndim >= 3 else v) for k, v in inp.items()}
    part = O.reference(first, grad_out[:1], th.float64)
    for param in O.PARAMS:
        k = "grad_" + param
        bound, _ = f64_distance_bound(r32[k], r64[k], acc_magnitude=r64["mag_" + param])
        moved = float((r64[k] - part[k]).abs().min())
        assert moved > 100 * bound, (param, moved, bound)
