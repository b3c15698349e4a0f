"""GPU (-m gpu): `msi` -- multi-sphere-image ray marching -- through the C ABI and through `drtk_amd.msi` under autograd,
against the CPU oracle of tests/msi_oracle.py (the reference has no CPU kernel and no `*_ref` model to record from).

Rays whose float64 decision margin is below 1e-5 (msi_oracle: a sphere grazed, sigma or a colour next to 0, transmittance
next to stop_thresh, the seam of atan2) are FRAGILE: float32 and float64 may take different branches there.  They are left
out of the comparison of `out`, and their grad_out rows are zero for the kernel and the oracle alike; a case may lose at
most 1e-3 of its rays this way; that, and that every case shows what it is named for, is asserted with each case.

Bounds (nothing hand-picked):
  float32   assert_within_f64_distance (tests/f64_distance.py) with its defaults -- oracle_f32 the oracle on the float32
            inputs, oracle_f64 the same inputs cast up; for grad_texture with the largest magnitude the oracle accumulates
            into a texel (the backward run on absolute values);
  float64   1e-12 * max|ref|;
  out[:, 3] exactly -1000 on every non-fragile ray the oracle stops early, and on no other."""
import pytest
import torch as th

import msi_oracle as O
from f64_distance import assert_within_f64_distance

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def hip(o, d, tex, gout, args, api):
    """(out, grad_texture) of the kernels as CPU tensors.  api: `python` (drtk_amd.msi under autograd) | `capi`."""
    import drtk_amd
    from drtk_amd import capi

    o, d, tex, gout = (t.to(DEV) for t in (o, d, tex, gout))
    if api == "capi":
        out = capi.msi_forward(o, d, tex, *args)
        grad = capi.msi_backward(gout, out, o, d, tex, *args)
    else:
        o.requires_grad_(True), d.requires_grad_(True), tex.requires_grad_(True)
        out = drtk_amd.msi(o, d, tex, *args)
        out.backward(gout)
        assert o.grad is None and d.grad is None  # the rays get no gradient
        grad = tex.grad
    return out.detach().cpu(), grad.cpu()


@pytest.mark.parametrize("api", ["capi", "python"])
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(O.CASES))
def test_cases_against_the_oracle(name, dtype, api):
    (o, d, tex, gout), args, fragile, r64, r32 = O.case(name)
    N = o.shape[0]
    assert int(fragile.sum()) <= O.FRAGILE_CAP * N, f"{int(fragile.sum())} of {N} rays are fragile"
    assert name != "outside_skip" or int(r64.skipped.sum()) >= N / 10
    assert name != "early_stop" or N / 10 <= int(r64.stopped.sum()) <= N - N / 10
    assert int(r64.edge.sum()) >= int(r64.taken.sum()) / 10  # samples with sigma <= 0 or a clamped colour
    check_against_the_oracle(O.case(name), dtype, api, name)


def check_against_the_oracle(case, dtype, api, name):
    """A case of O.case / O.build_case through `api` under the bounds of this file's docstring -> (out, grad_texture).
    Shared with tests/fuzz_added_ops.py."""
    (o, d, tex, gout), args, fragile, r64, r32 = case
    ok = ~fragile
    out, grad = hip(o, d, tex.to(dtype), gout.to(dtype), args, api)
    assert out.dtype == dtype and out.shape == (o.shape[0], 4) and grad.dtype == dtype and grad.shape == tex.shape
    assert th.equal(out[ok][:, 3] == -1000, r64.stopped[ok])
    live = ok & ~r64.stopped  # log_transmit of a stopped ray is the -1000 marker, checked exactly above: kept out of the scale
    if dtype == th.float32:
        e = assert_within_f64_distance(out[ok][:, :3], r32.out[ok][:, :3], r64.out[ok][:, :3], f"{name} out rgb")
        assert_within_f64_distance(out[live][:, 3], r32.out[live][:, 3], r64.out[live][:, 3], f"{name} out log_transmit")
        eg = assert_within_f64_distance(grad, r32.grad_texture, r64.grad_texture, f"{name} grad_texture",
                                        acc_magnitude=float(r64.magnitudes.max()))
        print(f"{name} {api}: |out - f64| = {e[0]:.3e} (oracle f32 {e[1]:.3e}), |grad - f64| = {eg[0]:.3e} (oracle f32 {eg[1]:.3e})")
    else:
        e = float((out[ok][:, :3] - r64.out[ok][:, :3]).abs().max())
        eg = float((grad - r64.grad_texture).abs().max())
        print(f"{name} {api} f64: |out - ref| = {e:.3e}, |grad - ref| = {eg:.3e}")
        assert e <= 1e-12 * float(r64.out[ok][:, :3].abs().max())
        if bool(live.any()):  # (a case of a few rays may stop them all: nothing to take a maximum of)
            assert float((out[live][:, 3] - r64.out[live][:, 3]).abs().max()) <= 1e-12 * float(r64.out[live][:, 3].abs().max())
        assert eg <= 1e-12 * float(r64.grad_texture.abs().max())
    return out, grad


def test_one_ray_and_no_ray():
    import drtk_amd
    from drtk_amd import capi

    (o, d, tex, gout), args, fragile, r64, r32 = O.case("outside_skip")
    k = int((~fragile & r64.skipped).nonzero()[0])
    one = O.march(o[k:k + 1], d[k:k + 1], tex.double(), *args, grad_out=gout[k:k + 1].double())
    one32 = O.march(o[k:k + 1], d[k:k + 1], tex, *args, grad_out=gout[k:k + 1])
    out, grad = hip(o[k:k + 1], d[k:k + 1], tex, gout[k:k + 1], args, "python")
    assert_within_f64_distance(out[:, :3], one32.out[:, :3], one.out[:, :3], "N = 1 out")
    assert_within_f64_distance(grad, one32.grad_texture, one.grad_texture, "N = 1 grad_texture", acc_magnitude=float(one.magnitudes.max()))
    for dtype in (th.float32, th.float64):
        t = tex.to(DEV, dtype).requires_grad_(True)
        empty = drtk_amd.msi(o[:0].to(DEV), d[:0].to(DEV), t, *args)
        assert empty.shape == (0, 4) and empty.dtype == dtype
        empty.sum().backward()
        assert t.grad.shape == tex.shape and not bool(t.grad.any())
        assert capi.msi_forward(o[:0].to(DEV), d[:0].to(DEV), t.detach(), *args).shape == (0, 4)
        g = capi.msi_backward(empty.detach(), empty.detach(), o[:0].to(DEV), d[:0].to(DEV), t.detach(), *args)
        assert not bool(g.any())  # zero-filled (the binding poisons what it allocates)


def test_texture_gradient_ignores_grad_out_column_3():
    (o, d, tex, gout), args, _, r64, _ = O.case("early_stop")
    other = gout.clone()
    other[:, 3] = th.linspace(-50, 50, gout.shape[0])
    a = hip(o, d, tex.double(), gout.double(), args, "python")[1]
    b = hip(o, d, tex.double(), other.double(), args, "python")[1]
    # the same terms in another atomic order: the float64 bound
    assert float((a - b).abs().max()) <= 1e-12 * float(r64.grad_texture.abs().max())


def test_no_backward_output_when_the_texture_needs_no_gradient():
    import drtk_amd

    (o, d, tex, gout), args, _, _, _ = O.case("one_layer")
    o, d, tex = o.to(DEV), d.to(DEV), tex.to(DEV)
    assert not drtk_amd.msi(o, d, tex, *args).requires_grad
    # a ray that asks for a gradient gets an undefined one; nothing is computed for the texture
    o.requires_grad_(True)
    out = drtk_amd.msi(o, d, tex, *args)
    assert out.requires_grad
    assert th.autograd.grad(out.sum(), o, allow_unused=True)[0] is None


def test_non_contiguous_ray_d_gives_the_same_result():
    import drtk_amd

    (o, d, tex, gout), args, _, _, _ = O.case("inside")
    both = th.cat([o, d], 1).to(DEV)  # [N,6]
    sliced = both[:, 3:]
    assert not sliced.is_contiguous()
    tex = tex.to(DEV)
    assert th.equal(drtk_amd.msi(o.to(DEV), sliced, tex, *args), drtk_amd.msi(o.to(DEV), d.to(DEV), tex, *args))
    assert th.equal(drtk_amd.msi(both[:, :3], sliced, tex, *args), drtk_amd.msi(o.to(DEV), d.to(DEV), tex, *args))


def test_autocast_casts_a_half_texture_to_float32():
    import drtk_amd

    (o, d, tex, gout), args, _, _, _ = O.case("one_layer")
    half = tex.to(DEV).half()
    with th.autocast("cuda", dtype=th.float16):
        out = drtk_amd.msi(o.to(DEV), d.to(DEV), half, *args)
    assert out.dtype == th.float32
    assert th.equal(out, drtk_amd.msi(o.to(DEV), d.to(DEV), half.float(), *args))
    with pytest.raises(RuntimeError, match="not implemented for 'Half'"):  # outside autocast there is no half kernel
        drtk_amd.msi(o.to(DEV), d.to(DEV), half, *args)
