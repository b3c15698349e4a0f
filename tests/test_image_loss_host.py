"""CPU: `ssim` and `photometric_loss` without a GPU -- the feature is present at every layer of the interface (Python export,
operator schemas and dispatch keys, the loud failure on CPU tensors, the argument errors, the C ABI's argument validation),
and the closed-form gradient its backward kernel evaluates is autograd of the definition (tests/image_loss_oracle.py)."""
import ctypes
import inspect

import pytest
import torch as th

import image_loss_oracle as O


def test_python_signatures_and_export():
    import drtk_amd

    E = inspect.Parameter.empty
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.ssim).parameters.values()]
    assert got == [("img", E), ("target", E), ("weight", None), ("window_size", 11), ("sigma", 1.5), ("data_range", 1.0),
                   ("padding", "same"), ("reduction", "mean")]
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.photometric_loss).parameters.values()]
    assert got == [("img", E), ("target", E), ("weight", None), ("l1_weight", 0.8), ("ssim_weight", 0.2), ("window_size", 11),
                   ("sigma", 1.5), ("data_range", 1.0), ("padding", "same")]
    assert "ssim" in drtk_amd.__all__ and "photometric_loss" in drtk_amd.__all__
    import drtk

    assert not hasattr(drtk, "ssim") and not hasattr(drtk, "photometric_loss")  # the drop-in keeps the reference's surface


def test_operator_schemas_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    want = {
        "ssim": "drtk_amd_ext::ssim(Tensor img, Tensor target, Tensor? weight, int window_size, float sigma, float data_range, bool valid) -> Tensor",
        "ssim_map": "drtk_amd_ext::ssim_map(Tensor img, Tensor target, int window_size, float sigma, float data_range, bool valid) -> Tensor",
        "photometric_loss": "drtk_amd_ext::photometric_loss(Tensor img, Tensor target, Tensor? weight, float l1_weight, float ssim_weight, "
                            "int window_size, float sigma, float data_range, bool valid) -> Tensor",
    }
    for name, schema in want.items():
        assert str(getattr(th.ops.drtk_amd_ext, name).default._schema) == schema, name
        for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
            assert th._C._dispatch_has_kernel_for_dispatch_key("drtk_amd_ext::" + name, key), (name, key)


def test_c_abi_names_are_declared_and_bound():
    """tests/test_host_logic.py holds the header's declarations against `nm -D`; here: the three names are among them."""
    import os
    import re

    from conftest import ROOT
    from drtk_amd import capi

    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    for name in ("drtk_amd_image_loss_workspace_bytes", "drtk_amd_image_loss_forward", "drtk_amd_image_loss_backward"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    x, y = th.rand(2, 3, 16, 20), th.rand(2, 3, 16, 20)
    w = th.ones(2, 16, 20, dtype=th.bool)
    for a, b in ((x, y), (x.double(), y.double()), (x.clone().requires_grad_(True), y)):
        for kwargs in ({}, {"weight": w}, {"padding": "valid"}, {"window_size": 7, "sigma": 1.0}):
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                drtk_amd.ssim(a, b, **kwargs)
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                drtk_amd.photometric_loss(a, b, **kwargs)
        with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
            drtk_amd.ssim(a, b, reduction="none")
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.drtk_amd_ext.ssim(x, y, None, 11, 1.5, 1.0, False)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.image_loss_forward(x, y)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.image_loss_backward(x, y, None, th.zeros(3, 2, 3, 16, 20), th.ones(()), th.zeros(4, dtype=th.float64))


def test_value_errors_before_any_launch():
    import drtk_amd

    x, y = th.rand(1, 2, 12, 14), th.rand(1, 2, 12, 14)
    bad = [
        dict(window_size=4), dict(window_size=1), dict(window_size=17), dict(window_size=-3), dict(window_size=11.0),
        dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
        dict(data_range=0.0), dict(data_range=-2.0),
        dict(padding="reflect"), dict(padding="SAME"), dict(padding=None),
        dict(padding="valid", window_size=13),  # H = 12 < 13
        dict(padding="valid", window_size=15),  # W = 14 < 15
    ]
    for kwargs in bad:
        for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
            with pytest.raises(ValueError):
                fn(x, y, **kwargs)
    for kwargs in (dict(reduction="sum"), dict(reduction=None), dict(reduction="none", weight=th.ones(1, 12, 14))):
        with pytest.raises(ValueError):
            drtk_amd.ssim(x, y, **kwargs)
    # the operators judge the same numbers (a caller that goes past the wrappers)
    for args in ((4, 1.5, 1.0, False), (17, 1.5, 1.0, False), (11, 0.0, 1.0, False), (11, 1.5, 0.0, False), (13, 1.5, 1.0, True)):
        with pytest.raises(ValueError):
            th.ops.drtk_amd_ext.ssim(x, y, None, *args)
        with pytest.raises(ValueError):
            th.ops.drtk_amd_ext.ssim_map(x, y, *args)
        with pytest.raises(ValueError):
            th.ops.drtk_amd_ext.photometric_loss(x, y, None, 0.8, 0.2, *args)
    # "valid" at exactly the window's size passes the checks (and then fails as CPU tensors)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        drtk_amd.ssim(th.rand(1, 1, 11, 11), th.rand(1, 1, 11, 11), padding="valid")


def test_shape_and_dtype_errors():
    import drtk_amd

    x = th.rand(2, 3, 16, 20)
    for a, b, kwargs, message in [
        (x[0], x[0], {}, r"expected img.ndim == 4"),
        (x, x[:, :2], {}, "same sizes"),
        (x, x.double(), {}, "same dtype"),
        (x.int(), x.int(), {}, "not implemented for 'Int'"),
        (x.half(), x.half(), {}, "not implemented for 'Half'"),
        (x, x, {"weight": th.ones(2, 3, 16, 20)}, r"expected weight to be \[N, H, W\] or \[N, 1, H, W\]"),
        (x, x, {"weight": th.ones(2, 16, 20, dtype=th.float64)}, "expected weight to be bool or"),
        (th.zeros(0, 3, 16, 20), th.zeros(0, 3, 16, 20), {}, "non-empty"),
    ]:
        for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
            with pytest.raises(RuntimeError, match=message):
                fn(a, b, **kwargs)


def test_target_requiring_a_gradient_names_the_workaround():
    import drtk_amd

    x, y = th.rand(1, 1, 16, 16), th.rand(1, 1, 16, 16).requires_grad_(True)
    for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
        with pytest.raises(RuntimeError, match="arguments exchanged"):
            fn(x, y)
        with th.no_grad(), pytest.raises(RuntimeError, match=r"\(HIP\) path only"):  # without autograd it is no error
            fn(x, y)


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci, cd = ctypes.c_int64, ctypes.c_int, ctypes.c_double
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    s3, s2 = (i64 * 3)(6000, 2000, 50), (i64 * 2)(2000, 50)

    def ws(N=2, H=40, W=50, k=11, valid=0, out="out"):
        o = ctypes.c_size_t(0)
        return lib.drtk_amd_image_loss_workspace_bytes(i64(N), i64(H), i64(W), ci(k), ci(valid), ctypes.byref(o) if out == "out" else None), o.value

    assert ws() == (0, 2 * 2 * 2 * 4 * 8)  # 2 views x (2 x 2 tiles of 32 x 32) x 4 doubles
    assert ws(valid=1) == (0, 2 * 1 * 2 * 4 * 8)  # the map is 30 x 40
    assert ws(out=None)[0] == -1 and ws(k=4)[0] == -1 and ws(k=17)[0] == -1 and ws(k=1)[0] == -1 and ws(N=0)[0] == -1
    assert ws(H=10, valid=1)[0] == -1 and ws(H=11, valid=1)[0] == 0 and ws(H=1 << 16, W=1 << 15)[0] == -1

    def head(dtype=0, x=p, xs=s3, y=p, ys=s3, w=z, kind=0, wst=s2, N=2, C=3, H=40, W=50, k=11, sigma=1.5, dr=1.0, valid=0, mode=1, l1=0.8, ss=0.2):
        return (ci(dtype), x, xs, y, ys, w, ci(kind), wst, i64(N), i64(C), i64(H), i64(W), ci(k), cd(sigma), cd(dr), ci(valid), ci(mode), cd(l1), cd(ss))

    def fwd(out=p, maps=z, scalars=p, wsp=p, nbytes=1 << 20, **kw):
        return lib.drtk_amd_image_loss_forward(*head(**kw), out, maps, scalars, wsp, ctypes.c_size_t(nbytes), z)

    def bwd(maps=p, gout=p, scalars=p, gimg=p, **kw):
        return lib.drtk_amd_image_loss_backward(*head(**kw), maps, gout, scalars, gimg, z)

    for f in (fwd, bwd):  # judged before any pointer is looked at (all of them are junk here)
        assert f(dtype=2) == -1 and f(dtype=7) == -1
        assert f(mode=3) == -1 and f(mode=-1) == -1 and f(kind=3) == -1
        assert f(mode=0, kind=2, w=p) == -1  # the map takes no weight
        assert f(k=4) == -1 and f(k=1) == -1 and f(k=17) == -1
        assert f(sigma=0.0) == -1 and f(sigma=float("nan")) == -1 and f(dr=0.0) == -1 and f(dr=float("inf")) == -1
        assert f(N=0) == -1 and f(C=0) == -1 and f(H=0) == -1 and f(W=-1) == -1
        assert f(H=10, valid=1) == -1
        assert f(x=z) == -1 and f(y=z) == -1 and f(xs=None) == -1 and f(ys=None) == -1
        assert f(kind=1, w=z) == -1 and f(kind=2, w=p, wst=None) == -1
        assert f(xs=(i64 * 3)(6000, -1, 50)) == -1
    assert fwd(out=z) == -1 and fwd(scalars=z) == -1 and fwd(wsp=z) == -1
    assert fwd(nbytes=8) == -2  # workspace too small
    assert bwd(maps=z) == -1 and bwd(gout=z) == -1 and bwd(gimg=z) == -1 and bwd(scalars=z) == -1


CASES = [((2, 3, 37, 53), 11, 1.5, 1.0), ((1, 2, 20, 17), 7, 1.0, 255.0), ((1, 1, 7, 9), 11, 1.5, 1.0), ((1, 1, 15, 15), 15, 2.5, 1.0)]
# "valid" needs H, W >= window_size
GRADIENT_CASES = [(*c, padding) for c in CASES for padding in ("same", "valid") if padding == "same" or min(c[0][2:]) >= c[1]]


@pytest.mark.parametrize(
    "shape,k,sigma,data_range,padding", GRADIENT_CASES, ids=[f"{'x'.join(map(str, c[0]))}-w{c[1]}-{c[4]}" for c in GRADIENT_CASES])
def test_closed_form_gradient_is_autograd_of_the_definition(shape, k, sigma, data_range, padding):
    """float64; at most 1e-12 (of max(1, max|autograd|)) for a random upstream map, for the weighted mean and for the
    photometric loss."""
    x, y = O.make_images(shape, seed=3, data_range=data_range)
    gen = th.Generator().manual_seed(5)
    kw = dict(window_size=k, sigma=sigma, data_range=data_range, padding=padding)

    def close(a, b):
        err, top = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
        assert err <= 1e-12 * top, (err, top)

    leaf = x.clone().requires_grad_(True)
    S = O.ssim(leaf, y, reduction="none", **kw)
    h = th.rand(S.shape, generator=gen, dtype=th.float64) * 2 - 1
    (S * h).sum().backward()
    close(O.gradient(x, y, h, **kw), leaf.grad)
    for weight in (None, O.make_mask(shape, seed=1), th.rand(shape[0], 1, *shape[2:], generator=gen, dtype=th.float64)):
        leaf = x.clone().requires_grad_(True)
        O.ssim(leaf, y, weight, **kw).backward()
        close(O.gradient(x, y, O.mean_upstream(weight, x, k, padding), **kw), leaf.grad)
        leaf = x.clone().requires_grad_(True)
        O.photometric_loss(leaf, y, weight, 0.7, 0.3, **kw).backward()
        close(O.photometric_gradient(x, y, weight, 0.7, 0.3, **kw), leaf.grad)


def test_oracle_fixed_points():
    """ssim(x, x) == 1 everywhere and in the mean; the losses of a zero weight are 0 with a zero gradient, all finite."""
    x, _ = O.make_images((2, 3, 24, 31), seed=1)
    for padding in ("same", "valid"):
        S = O.ssim(x, x, padding=padding, reduction="none")
        assert float((S - 1).abs().max()) <= 1e-12
        assert abs(float(O.ssim(x, x, padding=padding)) - 1) <= 1e-12
        assert abs(float(O.photometric_loss(x, x, padding=padding))) <= 1e-12
        zero = th.zeros(2, 24, 31, dtype=th.bool)
        y = (x * 0.5).requires_grad_(True)
        s, loss = O.ssim(y, x, zero, padding=padding), O.photometric_loss(y, x, zero, padding=padding)
        assert float(s.detach()) == 0.0 and float(loss.detach()) == 0.2 * (1 - 0.0)
        (s + loss).backward()
        assert bool(th.isfinite(y.grad).all()) and not bool(y.grad.any())
