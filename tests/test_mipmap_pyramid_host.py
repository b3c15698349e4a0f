"""CPU: `mipmap_pyramid` without a GPU -- the feature is present at every layer of the interface (Python export, operator
schema and dispatch keys, the loud failure on CPU tensors, the argument errors, the C ABI's argument validation), and the
definition and the backward recurrence its kernels evaluate are the `avg_pool2d` chain and its autograd."""
import ctypes
import inspect

import pytest
import torch as th
import torch.nn.functional as thf


def test_python_signature_and_export():
    import drtk_amd

    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.mipmap_pyramid).parameters.values()]
    assert got == [("input", inspect.Parameter.empty), ("levels", None)]
    assert "mipmap_pyramid" in drtk_amd.__all__
    import drtk

    assert not hasattr(drtk, "mipmap_pyramid")  # the drop-in keeps the reference's surface


def test_operator_schema_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    got = str(th.ops.drtk_amd_ext.mipmap_pyramid.default._schema)
    assert got == "drtk_amd_ext::mipmap_pyramid(Tensor input, int levels) -> Tensor[]", got
    for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
        assert th._C._dispatch_has_kernel_for_dispatch_key("drtk_amd_ext::mipmap_pyramid", key), key


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    x = th.zeros(2, 3, 8, 12)
    for t in (x, x.double(), x.clone().requires_grad_(True), x[:1].expand(4, -1, -1, -1)):
        for levels in (None, 2):
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                drtk_amd.mipmap_pyramid(t, levels)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.drtk_amd_ext.mipmap_pyramid(x, 3)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.mipmap_pyramid(x, 3)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.mipmap_pyramid_backward([x, None, th.zeros(2, 3, 2, 3)])


def test_argument_errors():
    import drtk_amd

    x = th.zeros(2, 3, 70, 130)
    for bad, message in [
        (x[0], r"expected input.ndim == 4"),
        (x.int(), "expected input to have floating point type"),
        (x.half(), "not implemented for 'Half'"),  # the sampler takes no float16 either
        (th.zeros(2, 3, 0, 8), "non-empty spatial dimensions"),
        (th.zeros(2, 3, 8, 0), "non-empty spatial dimensions"),
    ]:
        for levels in (None, 1):
            with pytest.raises(RuntimeError, match=message):
                drtk_amd.mipmap_pyramid(bad, levels)
        with pytest.raises(RuntimeError, match=message):
            th.ops.drtk_amd_ext.mipmap_pyramid(bad, 1)
    # levels: [1, min(11, 1 + floor(log2(min(H, W))))], the maximum named in the message
    for t, most in ((x, 7), (th.zeros(1, 1, 4096, 4096), 11), (th.zeros(1, 1, 1, 9), 1), (th.zeros(1, 1, 64, 64), 7), (th.zeros(1, 1, 63, 64), 6)):
        for levels in (0, -1, most + 1):
            with pytest.raises(ValueError, match=rf"levels must be in \[1, {most}\]"):
                drtk_amd.mipmap_pyramid(t, levels)
            with pytest.raises(ValueError, match=rf"levels must be in \[1, {most}\]"):
                th.ops.drtk_amd_ext.mipmap_pyramid(t, levels)
        for levels in (None, 1, most):  # these pass the checks (and then fail as CPU tensors)
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                drtk_amd.mipmap_pyramid(t, levels)


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    z, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def table(levels, holes=()):
        return (ctypes.c_void_p * 16)(*[0 if l in holes else 16 for l in range(16)]), (i64 * 16)(*[64] * 16)

    def fwd(dtype=0, inp=a16, sN=100000, sC=10000, N=2, C=3, H=70, W=130, levels=7, out="table", out_sN="table", holes=(0,)):
        ptrs, sn = table(levels, holes)
        return lib.drtk_amd_mipmap_pyramid(
            ci(dtype), inp, i64(sN), i64(sC), i64(N), i64(C), i64(H), i64(W), ci(levels), ptrs if out == "table" else out,
            sn if out_sN == "table" else out_sN, z)

    def bwd(dtype=0, N=2, C=3, H=70, W=130, levels=7, g="table", g_sN="table", holes=(1, 3), gi=a16):
        ptrs, sn = table(levels, holes)
        return lib.drtk_amd_mipmap_pyramid_backward(
            ci(dtype), ptrs if g == "table" else g, sn if g_sN == "table" else g_sN, i64(N), i64(C), i64(H), i64(W), ci(levels), gi, z)

    for f in (fwd, bwd):
        assert f(levels=0) == -1 and f(levels=-1) == -1 and f(levels=8) == -1 and f(levels=12) == -1  # 70 x 130: at most 7
        assert f(H=4096, W=4096, levels=12) == -1
        assert f(levels=0, N=0) == -1 and f(levels=12, H=0) == -1  # judged before the problem is found empty
        assert f(N=-1) == -1 and f(C=-1) == -1 and f(H=-1) == -1 and f(W=-1) == -1
        assert f(dtype=2) == -1 and f(dtype=7) == -1  # float16 is not one of this operator's types
        assert f(C=0) == -1  # elements, but no channel
        assert f(H=1 << 16, W=1 << 15, levels=1) == -1  # H * W < 2^31
        for empty in (dict(N=0), dict(H=0), dict(W=0), dict(N=0, C=0)):  # nothing is looked at
            assert f(**empty, levels=1) == 0
    assert fwd(inp=z) == -1 and fwd(out=None) == -1 and fwd(out_sN=None) == -1 and fwd(sN=-1) == -1 and fwd(sC=-1) == -1
    assert fwd(holes=(0, 3)) == -1  # a level without an output
    assert fwd(inp=z, out=None, out_sN=None, levels=1) == 0  # levels == 1: the input is the pyramid, nothing is launched
    assert fwd(N=0, inp=z, out=None, out_sN=None) == 0 and bwd(N=0, g=None, g_sN=None, gi=z) == 0
    assert bwd(g=None) == -1 and bwd(g_sN=None) == -1 and bwd(gi=z) == -1


def _next_level(x):
    h, w = x.shape[-2] // 2, x.shape[-1] // 2
    a, b = x[..., 0:2 * h:2, 0:2 * w:2], x[..., 0:2 * h:2, 1:2 * w:2]
    c, d = x[..., 1:2 * h:2, 0:2 * w:2], x[..., 1:2 * h:2, 1:2 * w:2]
    return (((a + b) + c) + d) * 0.25


def _recurrence(grads, shape):
    """G_{L-1} = g_{L-1}; G_l = g_l + 0.25 * up(G_{l+1}), a texel of a dropped row / column keeping g_l alone."""
    G = None
    for l in range(len(grads) - 1, -1, -1):
        h, w = shape[-2] >> l, shape[-1] >> l
        g = grads[l] if grads[l] is not None else th.zeros(*shape[:-2], h, w, dtype=th.float64)
        if G is not None:
            g = g.clone()
            g[..., :2 * G.shape[-2], :2 * G.shape[-1]] += 0.25 * G.repeat_interleave(2, -2).repeat_interleave(2, -1)
        G = g
    return G


@pytest.mark.parametrize("absent", [(), (0, 2), (1, 3, 5), (0, 1, 2, 3, 4)])
def test_definition_and_recurrence_are_the_avg_pool2d_chain_and_its_autograd(absent):
    """float64 on [2,3,35,70], six levels, with the odd drops 35 -> 17 and 17 -> 8; some g_l absent."""
    gen = th.Generator().manual_seed(7 + len(absent))
    x = (th.rand(2, 3, 35, 70, generator=gen, dtype=th.float64) * 2 - 1).requires_grad_(True)
    chain, mine = [x], [x.detach()]
    for _ in range(5):
        chain.append(thf.avg_pool2d(chain[-1], 2))
        mine.append(_next_level(mine[-1]))
    assert [tuple(t.shape[-2:]) for t in chain] == [(35, 70), (17, 35), (8, 17), (4, 8), (2, 4), (1, 2)]
    for a, b in zip(chain, mine):
        assert th.equal(a.detach(), b)
    grads = [None if l in absent else th.rand(t.shape, generator=gen, dtype=th.float64) * 6 - 3 for l, t in enumerate(chain)]
    sum((t * g).sum() for t, g in zip(chain, grads) if g is not None).backward()
    assert th.equal(_recurrence(grads, x.shape), x.grad)
