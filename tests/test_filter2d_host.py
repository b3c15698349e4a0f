"""CPU: `filter2d` without a GPU -- the filter design against the reference's recorded weights, the oracle of
tests/filter2d_oracle.py against the fixtures recorded from the reference's pure-PyTorch model (tests/gen_golden_filter2d.py)
and against its own structure (the `backward`-flag call is the derivative of the forward under zeros padding, and under
reflection exactly as far from the border as `gradient_reach` says), and the feature at every layer of the interface: C ABI
(output size, argument validation), operator schemas, dispatch keys and argument errors, the loud failure on CPU images, the
Python signatures, and the pinned boundary of the `drtk` drop-in package."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch as th
from conftest import ROOT

import filter2d_oracle as O

GOLDEN = os.path.join(ROOT, "tests", "golden")
U32 = 2.0 ** -24


def fixture(name):
    z = np.load(os.path.join(GOLDEN, "filter2d_" + name + ".npz"))
    return {k: (th.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


# ---- filter design ---------------------------------------------------------------------------------------------------------
def _options(n_taps, filter_type, guard):
    import drtk_amd

    return drtk_amd.FilterOptions(int(n_taps), drtk_amd.FilterType(int(filter_type)), float(guard))


def test_make_resampling_kernel_matches_the_recorded_weights_of_the_reference():
    """Per weight 4 * 2^-24 * |gain|: the float32 rounding of either side (weights are below |gain| ... 2 |gain| in
    magnitude: 2 * 2^-24 |gain| together, generously 3) plus the 2^-24 |gain| by which the reference's own two
    implementations differ (sqrt(2) evaluated in float in one, in double in the other)."""
    import drtk_amd

    z = np.load(os.path.join(GOLDEN, "filter2d_weights.npz"))
    params, weights, offsets = z["params"], z["weights"], z["offsets"]
    assert len(params) == 2 * 5 * (1 + 2 + 2 + 2) * 2 * 3
    worst = 0.0
    for r, (n_taps, m, freq_div, gain, guard, filter_type) in enumerate(params):
        want = th.from_numpy(weights[offsets[r]:offsets[r + 1]])
        got = drtk_amd.make_resampling_kernel(_options(n_taps, filter_type, guard), int(m), float(freq_div), float(gain), device="cpu")
        k = int(n_taps * m)
        assert got.dtype == th.float32 and got.shape == (k,) and got.device.type == "cpu"
        err = float((got.double() - want.double()).abs().max())
        worst = max(worst, err / abs(gain))
        assert err <= 4 * U32 * abs(gain), (params[r], err)
        assert abs(float(got.double().sum()) - gain) <= k * U32 * abs(gain), params[r]
        assert th.equal(got, got.flip(0)), params[r]  # symmetric: the taps sit symmetrically around 0
        # the oracle's own design (the case table's filters) is held to the same
        mine = O.design(int(n_taps), int(m), float(freq_div), float(gain), float(guard), int(filter_type))
        assert float((mine.double() - want.double()).abs().max()) <= 4 * U32 * abs(gain), params[r]
    print(f"largest |w - ref| / |gain| = {worst:.3e} (bound {4 * U32:.3e})")


def test_make_resampling_kernel_caches_per_key_and_checks_its_arguments():
    import drtk_amd

    opt = drtk_amd.FilterOptions(5, drtk_amd.FilterType.Lanczos, 0.25)
    a = drtk_amd.make_resampling_kernel(opt, 3, 1.5, 3.0)
    assert drtk_amd.make_resampling_kernel(opt, 3, 1.5, 3.0, device=th.device("cpu")) is a
    assert drtk_amd.make_resampling_kernel(opt, 3, 1.5, 2.0) is not a
    assert th.ops.filter2d_ext.make_resampling_kernel(5, 3, 1.5, 3.0, 0.25, 1, th.device("cpu")) is a
    mk = th.ops.filter2d_ext.make_resampling_kernel
    cpu = th.device("cpu")
    nan, inf = float("nan"), float("inf")
    bad = [
        ((0, 1, 1.0, 1.0, 0.0, 0), "n must be at least 1"),
        ((6, 0, 1.0, 1.0, 0.0, 0), "m must be at least 1"),
        ((6, 1, 0.0, 1.0, 0.0, 0), "freq_div must be finite and greater than 0"),
        ((6, 1, -1.0, 1.0, 0.0, 0), "freq_div must be finite and greater than 0"),
        ((6, 1, nan, 1.0, 0.0, 0), "freq_div must be finite and greater than 0"),
        ((6, 1, inf, 1.0, 0.0, 0), "freq_div must be finite and greater than 0"),
        ((6, 1, 1.0, inf, 0.0, 0), "gain must be finite"),
        ((6, 1, 1.0, nan, 0.0, 0), "gain must be finite"),
        ((6, 1, 1.0, 1.0, -0.5, 0), "alias_guard_band must be finite and non-negative"),
        ((6, 1, 1.0, 1.0, nan, 0), "alias_guard_band must be finite and non-negative"),
        ((6, 1, 1.0, 1.0, 0.0, 2), "filter_type must be Kaiser"),
        ((6, 1, 1.0, 1.0, 0.0, -1), "filter_type must be Kaiser"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            mk(*args, cpu)


# ---- the oracle against the reference's model, and against itself --------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CASES))
def test_oracle_agrees_with_the_recorded_reference_model_in_float64(name):
    fx = fixture(name)
    x, f, gout, up, down = O.make_case(name)
    P = fx["in_x"].shape[1]
    x, gout = x.reshape(1, -1, *x.shape[2:])[:, :P], gout.reshape(1, -1, *gout.shape[2:])[:, :P]
    assert th.equal(fx["in_x"], x) and th.equal(fx["in_f"], f) and th.equal(fx["in_grad_out"], gout)
    assert (fx["in_up"], fx["in_down"]) == (up, down)
    for padding in O.CASES[name][4]:
        ref = fx["out_" + padding]
        got = O.apply(x.double(), f, up, down, padding == "reflection")
        assert got.shape == ref.shape and ref.dtype == th.float64
        err = float((got - ref).abs().max())
        print(f"{name} {padding}: |oracle - model| = {err:.3e}, max|model| = {float(ref.abs().max()):.3e}")
        assert err <= 1e-12 * float(ref.abs().max())
    if "zeros" in O.CASES[name][4]:
        ref = fx["grad_zeros"]
        got = O.gradient(gout.double(), f, up, down, False, x.shape)
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


STRUCTURE = [(3, 2, 12), (2, 3, 10), (2, 1, 7), (1, 2, 7), (3, 1, 9), (1, 1, 1), (1, 1, 5), (2, 1, 12), (1, 2, 12), (4, 1, 16),
             (1, 4, 16), (1, 1, 8)]


@pytest.mark.parametrize("up,down,k", STRUCTURE)
def test_oracle_backward_flag_is_the_derivative_under_zeros_and_beyond_the_reach_under_reflection(up, down, k):
    g = th.Generator().manual_seed(7 * k + up)
    H, W = 12 * down, 16 * down  # multiples of down: the backward has the input's shape
    x = th.rand(1, 2, H, W, generator=g, dtype=th.float64)
    f = th.rand(k, generator=g) - 0.3
    gout = th.rand(1, 2, O.output_size(H, k, up, down), O.output_size(W, k, up, down), generator=g, dtype=th.float64)
    exact = O.autograd_gradient(x, gout, f, up, down, False)
    flag = O.gradient(gout, f, up, down, False, x.shape)
    assert float((flag - exact).abs().max()) <= 1e-12 * float(exact.abs().max())
    if not (O.reflect_ok(H, k, up, down) and O.reflect_ok(gout.shape[2], k, down, up, True)):
        return
    exact = O.autograd_gradient(x, gout, f, up, down, True)
    flag = O.gradient(gout, f, up, down, True, x.shape)
    r = O.gradient_reach(k, up, down)
    diff = (flag - exact).abs()
    scale = float(exact.abs().max())
    if 2 * r < H and 2 * r < W:
        assert float(diff[:, :, r:H - r, r:W - r].max()) <= 1e-12 * scale
    if k > 1:  # nearer the border it is another function, not a rounding of the derivative
        assert float(diff.max()) > 1e-3 * scale
    else:
        assert float(diff.max()) <= 1e-12 * scale


def test_oracle_refuses_what_the_operator_does_not_admit():
    f = th.ones(2)
    for up, down in ((1, 4), (4, 1), (8, 1), (1, 8)):
        with pytest.raises(ValueError, match="too short"):
            O.geometry(16, 2, up, down)
    with pytest.raises(ValueError, match="reflection"):
        O.axis_matrix(3, th.ones(9), 1, 1, True)
    with pytest.raises(ValueError, match="backward"):
        O.gradient(th.zeros(1, 1, 6, 8), th.ones(12), 1, 2, False, (1, 1, 13, 17))
    assert O.apply(th.zeros(1, 1, 13, 17), th.ones(12), 1, 2).shape == (1, 1, 6, 8)


# ---- the tuned families ------------------------------------------------------------------------------------------------------------
def tuned_families_of_the_source():
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "filter2d.hip")).read()
    bodies = re.findall(r"#define F2D_TUNED\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", src)
    assert len(bodies) == 1, bodies
    entries = re.findall(r"\bX\(([^)]*)\)", bodies[0])
    triples = [tuple(int(t) for t in e.split(",")) for e in entries]
    assert all(len(t) == 3 for t in triples), entries
    return triples


def test_families_is_exactly_the_tuned_set_of_the_source():
    """A family added to F2D_TUNED without an entry in FAMILIES would be compiled and never launched against the oracle
    (tests/test_gpu_filter2d.py runs FAMILIES)."""
    tuned = tuned_families_of_the_source()
    assert len(tuned) >= 29 and len(set(tuned)) == len(tuned), tuned
    assert len(set(O.FAMILIES)) == len(O.FAMILIES)
    assert set(O.FAMILIES) == set(tuned), (sorted(set(tuned) - set(O.FAMILIES)), sorted(set(O.FAMILIES) - set(tuned)))
    # forward and gradient of every entry launch every family with both settings of the `backward` flag
    assert {(d, u, k) for u, d, k in O.FAMILIES} == set(O.FAMILIES)
    # ... and every tuned family is one the kernel's static_assert admits: up == 1, or down == 1 and k a multiple of up
    assert all(u == 1 or (d == 1 and k % u == 0) for u, d, k in O.FAMILIES)


def test_the_family_cases_reach_every_tile_shape_and_admit_gradient_and_reflection():
    OH, OW = O.FAMILY_OUT
    # two tiles per axis at the widest and the tallest tile; a ragged last column tile at every tile width, a ragged last row
    # tile at the heights 32 and 16 (the lower heights divide every multiple of 8)
    assert OW > max(O.TILE_WIDTHS) and OH > max(O.TILE_HEIGHTS)
    assert all(OW % w != 0 for w in O.TILE_WIDTHS)
    assert all(OH % h != 0 for h in O.TILE_HEIGHTS[:2]) and all(OH % h == 0 for h in O.TILE_HEIGHTS[2:])
    for up, down, k in O.FAMILIES:
        x, f, gout = O.family_case(up, down, k)
        assert f.shape == (k,) and x.shape[:2] == gout.shape[:2] == O.FAMILY_PLANES
        assert tuple(gout.shape[2:]) == O.FAMILY_OUT, (up, down, k)
        for n, o in zip(x.shape[2:], gout.shape[2:]):
            assert n * up == o * down and n % down == 0
            assert O.geometry(n, k, up, down)[2] == o
            assert O.geometry(o, k, down, up, backward=True)[2] == n  # the gradient call exists
            assert O.reflect_ok(n, k, up, down) and O.reflect_ok(o, k, down, up, backward=True), (up, down, k, n)
    # the generic configuration the guarded driver adds (tests/guarded_added_ops.py): a gradient exists there too
    x, f, gout = O.family_case(3, 2, 12)
    assert tuple(x.shape[2:]) == (28, 48) and tuple(gout.shape[2:]) == (42, 72)
    assert O.gradient(gout.double(), f, 3, 2, True, x.shape).shape == x.shape


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_output_size_for_the_case_table():
    from drtk_amd import capi

    for name, (up, down, _, shape, _) in O.CASES.items():
        k = O.make_case(name)[1].shape[0]
        for n in shape[2:]:
            assert capi.filter2d_output_size(n, k, up, down) == O.output_size(n, k, up, down), name
    for n in range(1, 40):
        for up, down, k in STRUCTURE:
            try:
                want = O.output_size(n, k, up, down)
            except ValueError:  # an output smaller than 1: both refuse
                with pytest.raises(capi.DrtkAmdError):
                    capi.filter2d_output_size(n, k, up, down)
                continue
            assert capi.filter2d_output_size(n, k, up, down) == want
    assert O.output_size(4, 16, 1, 4) == 1 and O.output_size(13, 12, 1, 2) == 6 and O.output_size(19, 12, 2, 1) == 38
    out = ctypes.c_int64(0)
    i64 = ctypes.c_int64
    L = capi.lib()
    assert L.drtk_amd_filter2d_output_size(i64(8), i64(5), i64(1), i64(1), None) == -1
    for args in ((0, 5, 1, 1), (8, 0, 1, 1), (8, 5, 0, 1), (8, 5, 1, 0), (-3, 5, 1, 1), (8, 2, 1, 4), (8, 2, 8, 1), (1 << 31, 5, 1, 1),
                 (1 << 30, 5, 4, 1)):
        assert L.drtk_amd_filter2d_output_size(*map(i64, args), ctypes.byref(out)) == -1, args


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    lib = capi.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    z, a16 = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def call(dtype=0, x=a16, f=a16, planes=2, H=20, W=24, k=5, up=1, down=1, reflect=0, backward=0, generic=0, y=a16):
        return lib.drtk_amd_filter2d(ci(dtype), x, f, i64(planes), i64(H), i64(W), i64(k), i64(up), i64(down), ci(reflect), ci(backward),
                                     ci(generic), y, z)

    assert call(dtype=7) == -1 and call(dtype=-1) == -1 and call(dtype=3) == -1
    assert call(planes=-1) == -1
    assert call(H=0) == -1 and call(W=0) == -1 and call(H=-2) == -1  # an empty image
    assert call(k=0) == -1 and call(up=0) == -1 and call(down=0) == -1 and call(up=-1) == -1
    assert call(k=2, down=4) == -1 and call(k=2, up=4) == -1  # filter too short for the sampling factors
    assert call(k=2, down=4, backward=1) == -1 and call(k=2, up=4, backward=1) == -1
    assert call(H=1 << 16, W=1 << 16) == -1  # a plane is indexed with int
    assert call(H=1 << 31) == -1 and call(H=1 << 28, W=1, up=16, k=16) == -1
    assert call(H=3, W=24, k=9, reflect=1) == -1 and call(H=20, W=4, k=9, reflect=1) == -1  # torch's rule for reflect padding
    assert call(H=4, W=4, k=16, down=4, reflect=1) == -1
    assert call(x=z) == -1 and call(f=z) == -1 and call(y=z) == -1
    # all of it is judged before any pointer is looked at, in every dtype -- DRTK_F16 = 2 is accepted here
    for dtype in (0, 1, 2):
        assert call(dtype=dtype, planes=0, x=z, f=z, y=z) == 0
        assert call(dtype=dtype, planes=0, x=z, f=z, y=z, H=4, W=4, k=16, down=4) == 0
        assert call(dtype=dtype, planes=0, x=z, f=z, y=z, k=2, down=4) == -1
        assert call(dtype=dtype, x=z) == -1
    # no other entry point takes DRTK_F16
    assert lib.drtk_amd_msi_forward(ci(2), a16, a16, a16, i64(4), i64(2), i64(3), i64(3), ci(2), ctypes.c_double(1.0),
                                    ctypes.c_double(0.0), ctypes.c_double(1e-7), a16, z) == -1


# ---- operators -----------------------------------------------------------------------------------------------------------------
def test_operator_schemas_and_dispatch_keys():
    import drtk_amd  # noqa: F401  (loads the library)

    want = {
        "resample_filter": "filter2d_ext::resample_filter(Tensor x, Tensor f, int up, int down, bool reflect) -> Tensor",
        "low_pass_filter": "filter2d_ext::low_pass_filter(Tensor x, int n, float freq_div, float alias_guard_band, int filter_type, bool reflect) -> Tensor",
        "downsample": "filter2d_ext::downsample(Tensor x, int n, int m, float alias_guard_band, int filter_type, bool reflect) -> Tensor",
        "upsample": "filter2d_ext::upsample(Tensor x, int n, int m, float alias_guard_band, int filter_type, bool reflect) -> Tensor",
        "make_resampling_kernel": "filter2d_ext::make_resampling_kernel(int n, int m, float freq_div, float gain, float alias_guard_band, int filter_type, Device d) -> Tensor",
    }
    for name, schema in want.items():
        assert str(getattr(th.ops.filter2d_ext, name).default._schema) == schema, name
        if name != "make_resampling_kernel":
            for key in ("CUDA", "CPU", "Autograd"):
                assert th._C._dispatch_has_kernel_for_dispatch_key("filter2d_ext::" + name, key), (name, key)
            assert not th._C._dispatch_has_kernel_for_dispatch_key("filter2d_ext::" + name, "AutocastCUDA"), name


def test_operator_argument_errors():
    import drtk_amd

    x, f = th.zeros(1, 2, 12, 16), th.ones(6)
    bad = [
        (dict(f=f.double()), "f must be float32"),
        (dict(f=f[None]), "f must be rank 1"),
        (dict(x=x[0]), "x must be rank 4"),
        (dict(x=x.to(th.int32)), "x dtype must be float16, float32, or float64"),
        (dict(x=x.to(th.bfloat16)), "x dtype must be float16, float32, or float64"),
        (dict(x=x[:, :, :0]), "x dimensions must be non-empty"),
        (dict(f=f[:0]), "f must have at least one tap"),
        (dict(up=0), r"upsampling factor \(up\) must be at least 1"),
        (dict(down=0), r"downsampling factor \(down\) must be at least 1"),
        (dict(f=f[:2], down=4), "filter too short for the sampling factors: f has 2 taps"),
        (dict(f=f[:2], up=8), "filter too short for the sampling factors: f has 2 taps"),
        (dict(x=x[:, :, :4, :4], f=th.ones(16), down=4, padding_mode="reflection"), "reflection padding of"),
        (dict(x=x[:, :, :3], f=th.ones(9), padding_mode="reflection"), "reflection padding of"),
    ]
    for kw, message in bad:
        args = dict(x=x, f=f, up=1, down=1, padding_mode="zeros")
        args.update(kw)
        with pytest.raises(RuntimeError, match=message):
            drtk_amd.resample_filter(**args)
    opt = drtk_amd.FilterOptions()
    with pytest.raises(RuntimeError, match="upsampling factor must be at least 1"):
        drtk_amd.upsample(x, opt, 0)
    with pytest.raises(RuntimeError, match="downsampling factor must be at least 1"):
        drtk_amd.downsample(x, opt, 0)
    with pytest.raises(RuntimeError, match="freq_div must be finite and greater than 0"):
        drtk_amd.low_pass_filter(x, opt, 0.0)
    with pytest.raises(RuntimeError, match="n must be at least 1"):
        drtk_amd.upsample(x, drtk_amd.FilterOptions(0))


def test_cpu_images_fail_loudly_no_fallback():
    import drtk_amd
    from drtk_amd import capi

    opt = drtk_amd.FilterOptions()
    for x in (th.zeros(1, 2, 12, 16), th.zeros(1, 2, 12, 16, dtype=th.float64), th.zeros(1, 2, 12, 16).half(),
              th.zeros(1, 2, 12, 16, requires_grad=True)):
        for call in (lambda: drtk_amd.upsample(x, opt), lambda: drtk_amd.downsample(x, opt), lambda: drtk_amd.low_pass_filter(x, opt),
                     lambda: drtk_amd.filter(x, th.ones(3)), lambda: drtk_amd.resample_filter(x, th.ones(4), 2, 1, "zeros")):
            with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
                call()
    with pytest.raises(RuntimeError, match=r"\(HIP\) path only"):
        th.ops.filter2d_ext.resample_filter(th.zeros(1, 1, 8, 8), th.ones(3), 1, 1, False)
    with pytest.raises(capi.DrtkAmdError, match="HIP"):
        capi.filter2d(th.zeros(1, 1, 8, 8), th.ones(3))


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_python_signatures_exports_and_options():
    import drtk_amd

    want = {  # drtk/filter2d.py
        "resample_filter": "(x: torch.Tensor, f: torch.Tensor, up: int = 1, down: int = 1, padding_mode: str = 'reflection') -> torch.Tensor",
        "filter": "(x: torch.Tensor, f: torch.Tensor, padding_mode: str = 'reflection') -> torch.Tensor",
        "upsample": "(x: torch.Tensor, filter_options: drtk_amd.filter2d.FilterOptions, upsample_factor: int = 2, padding_mode: str = 'reflection') -> torch.Tensor",
        "downsample": "(x: torch.Tensor, filter_options: drtk_amd.filter2d.FilterOptions, downsample_factor: int = 2, padding_mode: str = 'reflection') -> torch.Tensor",
        "low_pass_filter": "(x: torch.Tensor, filter_options: drtk_amd.filter2d.FilterOptions, freq_div: float = 1.0, padding_mode: str = 'reflection') -> torch.Tensor",
        "make_resampling_kernel": "(filter_options: drtk_amd.filter2d.FilterOptions, m: int = 1, freq_div: float = 1.0, gain: float = 1.0, device: Optional[torch.device] = None) -> torch.Tensor",
        "FilterOptions": "(n_taps: int = 6, filter_type: drtk_amd.filter2d.FilterType = <FilterType.Kaiser: 0>, alias_guard_band: Optional[float] = None, alias_suppression_level: Optional[float] = None) -> None",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(drtk_amd, name))) == sig, (name, str(inspect.signature(getattr(drtk_amd, name))))
        assert name in drtk_amd.__all__
    assert "FilterType" in drtk_amd.__all__
    assert [(t.name, t.value) for t in drtk_amd.FilterType] == [("Kaiser", 0), ("Lanczos", 1)]
    assert "not the derivative" in drtk_amd.resample_filter.__doc__.lower()
    # the alias and its conflict error
    o = drtk_amd.FilterOptions()
    assert (o.n_taps, o.filter_type, o.alias_guard_band, o.alias_suppression_level) == (6, drtk_amd.FilterType.Kaiser, 0.0, 0.0)
    assert drtk_amd.FilterOptions(alias_suppression_level=0.5).alias_guard_band == 0.5
    assert drtk_amd.FilterOptions(alias_guard_band=0.25, alias_suppression_level=0.25).alias_guard_band == 0.25
    with pytest.raises(ValueError, match="specify only one of alias_guard_band and alias_suppression_level"):
        drtk_amd.FilterOptions(alias_guard_band=0.25, alias_suppression_level=0.5)
    o.alias_suppression_level = 0.75
    assert o.alias_guard_band == 0.75
    with pytest.raises(TypeError, match="FilterType"):
        drtk_amd.FilterOptions(filter_type=0)
    with pytest.raises(AttributeError):
        o.other = 1  # __slots__
    x = th.zeros(1, 1, 8, 8)
    for call in (lambda m: drtk_amd.upsample(x, o, 2, m), lambda m: drtk_amd.downsample(x, o, 2, m), lambda m: drtk_amd.low_pass_filter(x, o, 1.0, m),
                 lambda m: drtk_amd.filter(x, th.ones(3), m), lambda m: drtk_amd.resample_filter(x, th.ones(3), 1, 1, m)):
        for mode in ("border", "reflect", ""):
            with pytest.raises(NotImplementedError, match="'zeros' or 'reflection'"):
                call(mode)


def test_the_drop_in_package_does_not_lift_filter2d_yet():
    from drtk_amd.utils import load_torch_ops

    for name in ("drtk.filter2d_ext", "drtk_amd.filter2d_ext"):
        with pytest.raises(ImportError):
            load_torch_ops(name)
    import drtk

    for name in ("upsample", "downsample", "low_pass_filter", "resample_filter", "FilterOptions"):
        with pytest.raises(AttributeError, match="not provided"):
            getattr(drtk, name)
