"""CPU: `composite_layers` without a GPU -- the feature is present at every layer of the interface (Python export, operator
schema and dispatch keys, the loud failure on CPU tensors, the operator's argument errors, the C ABI's argument
validation), and the back-to-front recurrence its backward kernel evaluates is the derivative of the definition."""
import ctypes
import inspect

import pytest
import torch as th


def test_python_signature_and_export():
    import drtk_amd

    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.composite_layers).parameters.values()]
    assert got == [("color", inspect.Parameter.empty), ("alpha", None), ("index_img", None), ("background", None)]
    assert "composite_layers" in drtk_amd.__all__
    import drtk

    assert not hasattr(drtk, "composite_layers")  # the drop-in keeps the reference's surface


def test_operator_schema_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    got = str(th.ops.drtk_amd_ext.composite_layers.default._schema)
    want = "drtk_amd_ext::composite_layers(Tensor color, Tensor? alpha, Tensor? index_img, Tensor? background) -> (Tensor, Tensor)"
    assert got == want, got
    for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
        assert th._C._dispatch_has_kernel_for_dispatch_key("drtk_amd_ext::composite_layers", key), key


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    color, alpha = th.zeros(1, 2, 3, 4, 5), th.zeros(1, 2, 4, 5)
    for c in (color, color.double(), color.clone().requires_grad_(True)):
        with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
            drtk_amd.composite_layers(c, alpha.to(c.dtype))
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.drtk_amd_ext.composite_layers(color, None, None, None)  # rgba
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.composite_layers(color, alpha)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.composite_layers_backward(th.zeros(1, 3, 4, 5), None, color, alpha)


def test_argument_errors():
    import drtk_amd

    N, K, C, H, W = 2, 3, 3, 4, 5
    color, alpha = th.zeros(N, K, C, H, W), th.zeros(N, K, H, W)
    index, bg = th.zeros(N, K, H, W, dtype=th.int32), th.zeros(N, C, H, W)
    bad = [
        (dict(color=color[0]), r"expected color.ndim == 5"),
        (dict(color=color.int()), "expected color to have floating point type"),
        (dict(alpha=alpha[0]), r"expected alpha to be \[N, K, H, W\] or \[N, K, 1, H, W\]"),
        (dict(alpha=th.zeros(N, K, 2, H, W)), r"expected alpha to be \[N, K, H, W\] or \[N, K, 1, H, W\]"),
        (dict(alpha=th.zeros(N, K, H, W + 1)), "expected alpha to match color in N, K, H and W"),
        (dict(alpha=alpha.double()), "expected alpha to have the type of color"),
        (dict(color=th.zeros(N, K, 1, H, W), alpha=None), "without alpha, color must be rgba"),
        (dict(color=th.zeros(N, 9, C, H, W), alpha=th.zeros(N, 9, H, W)), r"the number of layers must be in \[1, 8\], but got 9"),
        (dict(color=th.zeros(N, 0, C, H, W), alpha=th.zeros(N, 0, H, W)), r"the number of layers must be in \[1, 8\], but got 0"),
        (dict(color=th.zeros(N, K, 0, H, W)), "expected at least one colour channel"),
        (dict(index_img=index.long()), "expected index_img to have int32 type"),
        (dict(index_img=index[:, :2]), r"expected index_img to be \[N, K, H, W\]"),
        (dict(index_img=index[0]), r"expected index_img to be \[N, K, H, W\]"),
        (dict(background=bg[:, :2]), r"expected background to be \[N, C, H, W\]"),
        (dict(background=bg[:1]), r"expected background to be \[N, C, H, W\]"),
        (dict(background=bg.double()), "expected background to have the type of color"),
    ]
    for kw, message in bad:
        args = dict(color=color, alpha=alpha, index_img=index, background=bg)
        args.update(kw)
        with pytest.raises(RuntimeError, match=message):
            drtk_amd.composite_layers(**args)
    # [N,K,1,H,W] alpha and the rgba form pass the checks (and then fail as CPU tensors)
    for args in (dict(color=color, alpha=alpha[:, :, None]), dict(color=th.zeros(N, K, C + 1, H, W), index_img=index, background=bg)):
        with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
            drtk_amd.composite_layers(**args)


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    z, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)
    s3, s2 = (i64 * 3)(60, 20, 4), (i64 * 2)(8, 4)
    neg3 = (i64 * 3)(60, -20, 4)

    def fwd(dtype=0, color=a16, cs=s3, alpha=a16, as_=s2, index=a16, bg=a16, bg_sN=12, N=2, K=3, C=3, H=2, W=2, img=a16, trans=a16):
        return lib.drtk_amd_composite_layers(
            ci(dtype), color, cs, alpha, as_, index, bg, i64(bg_sN), i64(N), i64(K), i64(C), i64(H), i64(W), img, trans, z)

    def bwd(dtype=0, gi=a16, gt=a16, color=a16, cs=s3, alpha=a16, as_=s2, index=a16, bg=a16, bg_sN=12, N=2, K=3, C=3, H=2, W=2,
            gc=a16, gcs=s3, ga=a16, gas=s2, gb=a16):
        return lib.drtk_amd_composite_layers_backward(
            ci(dtype), gi, gt, color, cs, alpha, as_, index, bg, i64(bg_sN), i64(N), i64(K), i64(C), i64(H), i64(W), gc, gcs, ga,
            gas, gb, z)

    for f in (fwd, bwd):
        assert f(K=0) == -1 and f(K=9) == -1 and f(K=-1) == -1
        assert f(K=0, N=0) == -1 and f(K=9, H=0) == -1  # judged before the problem is found empty
        assert f(N=-1) == -1 and f(C=-1) == -1 and f(H=-1) == -1 and f(W=-1) == -1
        assert f(dtype=2) == -1 and f(dtype=7) == -1  # float16 is not one of this operator's types
        assert f(C=0) == -1  # elements, but no channel
        assert f(H=1 << 16, W=1 << 15) == -1  # H * W < 2^31
        assert f(color=z) == -1 and f(alpha=z) == -1 and f(cs=None) == -1 and f(as_=None) == -1
        assert f(cs=neg3) == -1 and f(bg_sN=-1) == -1
        # empty problems: nothing is looked at
        for empty in (dict(N=0), dict(H=0), dict(W=0), dict(N=0, C=0)):
            assert f(color=z, alpha=z, index=z, bg=z, cs=None, as_=None, **empty) == 0
    assert fwd(img=z) == -1 and fwd(trans=z) == -1
    assert bwd(gcs=None) == -1 and bwd(gas=None) == -1 and bwd(gcs=neg3) == -1
    assert bwd(bg=z) == -1  # a background gradient without a background
    assert bwd(gc=z, ga=z, gb=z, gcs=None, gas=None) == 0  # nothing wanted: nothing launched


def _loop(color, alpha, index, background):
    N, K, C, H, W = color.shape
    img, T = color.new_zeros(N, C, H, W), color.new_ones(N, 1, H, W)
    for k in range(K):
        a = alpha[:, k:k + 1]
        if index is not None:
            a = a * (index[:, k:k + 1] != -1)
        img = img + (T * a) * color[:, k]
        T = T * (1 - a)
    if background is not None:
        img = img + T * background
    return img, T


@pytest.mark.parametrize("K,C", [(1, 1), (3, 3), (5, 4), (8, 7)])
def test_the_recurrence_of_the_backward_is_autograd_of_the_definition(K, C):
    """float64, alphas of exactly 0 and 1, index holes: the division-free recurrence of csrc/composite.hip, restated in
    PyTorch, against autograd of the loop."""
    g = th.Generator().manual_seed(K * 31 + C)
    N, H, W = 2, 5, 7
    color = (th.rand(N, K, C, H, W, generator=g, dtype=th.float64) * 2 - 1).requires_grad_(True)
    alpha = th.rand(N, K, H, W, generator=g, dtype=th.float64)
    r = th.rand(N, K, H, W, generator=g)
    alpha[r < 0.15], alpha[r > 0.85] = 0.0, 1.0
    alpha.requires_grad_(True)
    bg = (th.rand(N, C, H, W, generator=g, dtype=th.float64) * 2 - 1).requires_grad_(True)
    index = th.where(th.rand(N, K, H, W, generator=g) < 0.3, -1, 5).int()
    g_img, g_T = th.rand(N, C, H, W, generator=g, dtype=th.float64) * 6 - 3, th.rand(N, 1, H, W, generator=g, dtype=th.float64) * 6 - 3
    img, T = _loop(color, alpha, index, bg)
    ((img * g_img).sum() + (T * g_T).sum()).backward()

    with th.no_grad():
        m = index != -1
        a = alpha * m
        Tk = [th.ones(N, H, W, dtype=th.float64)]
        for k in range(K):
            Tk.append(Tk[-1] * (1 - a[:, k]))
        d = (color * g_img[:, None]).sum(2) * m
        R = g_T[:, 0] + (bg * g_img).sum(1)
        ga, gc = th.zeros_like(alpha), th.zeros_like(color)
        for k in range(K - 1, -1, -1):
            ga[:, k] = Tk[k] * (d[:, k] - R) * m[:, k]
            gc[:, k] = (Tk[k] * a[:, k])[:, None] * g_img
            R = a[:, k] * d[:, k] + (1 - a[:, k]) * R
        gb = Tk[K][:, None] * g_img
    assert float((ga - alpha.grad).abs().max()) <= 1e-13
    assert float((gc - color.grad).abs().max()) <= 1e-13
    assert float((gb - bg.grad).abs().max()) <= 1e-13
