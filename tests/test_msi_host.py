"""CPU: `msi` without a GPU -- the oracle of tests/msi_oracle.py checks itself (float32 against float64 on the cases the GPU
suite runs, its backward against autograd of its own forward, the sigma-gradient identity, early termination), and the
feature is present at every layer of the interface: Python signature and export, operator schema and dispatch keys, the
operator's argument errors, the loud failure on CPU tensors, the C ABI's argument validation, and the pinned boundary of
the `drtk` drop-in package (msi_ext is not one of its extension names yet)."""
import ctypes
import inspect

import pytest
import torch as th

import msi_oracle as O

CASES, case = O.CASES, O.case


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_float32_agrees_with_float64_outside_the_fragile_rays(name):
    (o, d, tex, gout), args, fragile, r64, r32 = case(name)
    N = o.shape[0]
    assert int(fragile.sum()) <= O.FRAGILE_CAP * N, f"{int(fragile.sum())} of {N} rays are fragile"
    ok = ~fragile
    # 1e-5 of the output's scale: the bar every float32 result of this repository is held to (tests/f64_distance.py)
    err = float((r32.out.double() - r64.out)[ok].abs().max())
    print(f"{name}: fragile {int(fragile.sum())}, |out32 - out64| = {err:.3e}")
    assert err <= 1e-5 * float(r64.out[ok][:, :3].abs().max())
    assert th.equal(r32.out[ok][:, 3] == -1000, r64.out[ok][:, 3] == -1000) and th.equal(r32.stopped[ok], r64.stopped[ok])
    gerr = float((r32.grad_texture.double() - r64.grad_texture).abs().max())
    assert gerr <= 1e-5 * float(r64.grad_texture.abs().max()), gerr
    assert bool((r64.grad_texture.abs() <= r64.magnitudes * (1 + 1e-12)).all())


@pytest.mark.parametrize("name", list(CASES))
def test_each_case_exercises_what_it_is_named_for(name):
    _, _, fragile, r64, _ = case(name)
    N = fragile.numel()
    if name == "outside_skip":
        assert int(r64.skipped.sum()) >= N / 10
    if name == "early_stop":
        assert N / 10 <= int(r64.stopped.sum()) <= N - N / 10
    if name == "one_layer":
        assert int(r64.taken.sum()) == N  # one sphere, every ray inside it
    # samples with sigma <= 0 (not composited) or a colour that is clamped
    assert int(r64.edge.sum()) >= int(r64.taken.sum()) / 10


def _small(seed=5, N=48, stop=1e-7, sigma=(-0.5, 2.5), radius=1.5):
    o, d, tex, gout = O.make_case(seed, N, 3, 4, 6, sigma, radius, th.float64)
    return o, d, tex, gout, (2, 1.0, 0.05, stop)


def test_oracle_colour_gradient_is_autograd_of_its_forward_and_sigma_obeys_the_identity():
    """rays of every kind (inside, outside, skipping spheres, stopping early): the colour planes of the oracle's backward
    are what autograd makes of the forward; the sigma plane is NOT -- it is the reference's expression -- but the
    identity  analytic = s (ref + sum_ch max(rgb, 0) g T (1 - exp(-sigma)))  turns it into autograd's to 1e-10."""
    for stop, sigma in ((1e-7, (-0.5, 2.5)), (1e-2, (0.0, 12.0))):
        o, d, tex, gout, args = _small(stop=stop, sigma=sigma)
        fragile = O.march(o, d, tex, *args).margin < O.FRAGILE_MARGIN
        gout[fragile] = 0
        t = tex.clone().requires_grad_(True)
        out = O.forward_autograd(o, d, t, *args)
        (out[:, :3] * gout[:, :3]).sum().backward()
        ref = O.march(o, d, tex, *args, grad_out=gout)
        assert float((out.detach() - ref.out).abs().max()) <= 1e-13
        scale = float(t.grad.abs().max())
        assert float((ref.grad_texture[:, :3] - t.grad[:, :3]).abs().max()) <= 1e-10 * scale
        analytic = O.march(o, d, tex, *args, grad_out=gout, analytic_sigma=True)
        assert float((analytic.grad_texture - t.grad).abs().max()) <= 1e-10 * scale
        # the difference is real: the reference's sigma plane is not a rounding of the derivative
        assert float((ref.grad_texture[:, 3] - t.grad[:, 3]).abs().max()) > 1e-2 * float(t.grad[:, 3].abs().max())
        assert bool(ref.stopped.any()) == (stop == 1e-2)


def test_oracle_early_stop_writes_minus_1000_and_grad_out_column_3_is_ignored():
    o, d, tex, gout, args = _small(stop=1e-2, sigma=(0.0, 12.0), radius=0.5)
    r = O.march(o, d, tex, *args, grad_out=gout)
    assert bool(r.stopped.any()) and not bool(r.stopped.all())
    assert th.equal(r.out[:, 3] == -1000, r.stopped) and bool((r.out[~r.stopped, 3] > -1000).all())
    g2 = gout.clone()
    g2[:, 3] = 7.0
    assert th.equal(O.march(o, d, tex, *args, grad_out=g2).grad_texture, r.grad_texture)


def test_python_signature_and_export():
    import drtk_amd

    E = inspect.Parameter.empty
    got = [(p.name, p.default) for p in inspect.signature(drtk_amd.msi).parameters.values()]
    assert got == [("ray_o", E), ("ray_d", E), ("texture", E), ("sub_step_count", 2), ("min_inv_r", 1.0), ("max_inv_r", 0.0),
                   ("stop_thresh", 1e-7)]  # drtk/msi.py:15-23
    assert "msi" in drtk_amd.__all__ and "not the derivative" in drtk_amd.msi.__doc__.lower()


def test_operator_schema_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    got = str(th.ops.msi_ext.msi.default._schema)
    want = "msi_ext::msi(Tensor ray_o, Tensor ray_d, Tensor texture, int sub_step_count, float min_inv_r, float max_inv_r, float stop_thresh) -> Tensor"
    assert got == want, got
    for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
        assert th._C._dispatch_has_kernel_for_dispatch_key("msi_ext::msi", key), key


def test_operator_argument_errors():
    import drtk_amd

    o, d, tex = th.zeros(5, 3), th.ones(5, 3), th.zeros(2, 4, 3, 3)
    bad = [
        (dict(sub_step_count=0), "expected step_size > 0"),
        (dict(stop_thresh=0.0), "expected 0 < stop_thresh < 1"),
        (dict(stop_thresh=1.0), "expected 0 < stop_thresh < 1"),
        (dict(min_inv_r=0.5, max_inv_r=0.5), "expected min_inv_r to be greater than max_inv_r"),
        (dict(texture=tex.to(th.int32)), "expected texture to be of type Double, Float or Half"),
        (dict(ray_o=o.double()), "expected ray_o and ray_d to be of type Float"),
        (dict(ray_d=d.half()), "expected ray_o and ray_d to be of type Float"),
        (dict(ray_o=o[:, None]), "expected ray_o and ray_d to have 2 dimensions"),
        (dict(texture=tex[0]), "texture to have 4 dimension"),
        (dict(ray_d=th.ones(5, 2)), "expected ray_o, ray_d to have size 3 along the dimension 1"),
        (dict(texture=th.zeros(2, 3, 3, 3)), "texture to have size 4 along the dimension 1"),
        (dict(ray_d=th.ones(4, 3)), "to have the same size along the dimension 0"),
    ]
    for kw, message in bad:
        args = dict(ray_o=o, ray_d=d, texture=tex)
        args.update(kw)
        with pytest.raises(RuntimeError, match=message):
            drtk_amd.msi(**args)


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    o, d, tex = th.zeros(5, 3), th.ones(5, 3), th.zeros(2, 4, 3, 3)
    for t in (tex, tex.double(), tex.clone().requires_grad_(True)):
        with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
            drtk_amd.msi(o, d, t)
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.msi_ext.msi(o, d, tex, 2, 1.0, 0.0, 1e-7)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.msi_forward(o, d, tex)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.msi_backward(th.zeros(5, 4), th.zeros(5, 4), o, d, tex)


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci, cd = ctypes.c_int64, ctypes.c_int, ctypes.c_double
    z, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def fwd(dtype=0, o=a16, d=a16, tex=a16, N=4, L=2, H=3, W=3, sub=2, mn=1.0, mx=0.0, stop=1e-7, out=a16):
        return lib.drtk_amd_msi_forward(ci(dtype), o, d, tex, i64(N), i64(L), i64(H), i64(W), ci(sub), cd(mn), cd(mx), cd(stop), out, z)

    def bwd(dtype=0, go=a16, out=a16, o=a16, d=a16, tex=a16, N=4, L=2, H=3, W=3, sub=2, mn=1.0, mx=0.0, stop=1e-7, gt=a16):
        return lib.drtk_amd_msi_backward(ci(dtype), go, out, o, d, tex, i64(N), i64(L), i64(H), i64(W), ci(sub), cd(mn), cd(mx),
                                         cd(stop), gt, z)

    for f in (fwd, bwd):
        assert f(dtype=7) == -1
        assert f(N=-1) == -1 and f(L=-1) == -1 and f(H=-1) == -1 and f(W=-1) == -1
        assert f(N=1 << 31) == -1
        assert f(L=0) == -1 and f(H=0) == -1 and f(W=0) == -1  # rays, but nothing to sample
        assert f(L=1 << 10, H=1 << 10, W=1 << 9) == -1  # L * 4 * H * W < 2^31
        assert f(sub=0) == -1 and f(sub=-2) == -1
        assert f(mn=0.5, mx=0.5) == -1 and f(mn=0.0, mx=1.0) == -1 and f(mn=float("nan")) == -1
        assert f(stop=0.0) == -1 and f(stop=1.0) == -1 and f(stop=-1e-3) == -1 and f(stop=float("nan")) == -1
        assert f(o=z) == -1 and f(d=z) == -1 and f(tex=z) == -1 and f(out=z) == -1
    assert bwd(go=z) == -1 and bwd(gt=z) == -1
    # no rays: the forward looks at no pointer
    assert fwd(N=0, o=z, d=z, tex=z, out=z) == 0 and fwd(N=0, L=0, o=z, d=z, tex=z, out=z) == 0
    assert bwd(N=0, L=0, go=z, out=z, o=z, d=z, tex=z, gt=z) == 0
    assert bwd(N=0, gt=z) == -1  # the gradient of a texture is zero-filled even without rays


def test_the_drop_in_package_does_not_lift_msi_yet():
    from drtk_amd.utils import load_torch_ops

    for name in ("drtk.msi_ext", "drtk_amd.msi_ext"):
        with pytest.raises(ImportError):
            load_torch_ops(name)
    import drtk

    with pytest.raises(AttributeError, match="not provided"):
        drtk.msi
