"""GPU (-m gpu): `drtk_amd.ssim` / `drtk_amd.photometric_loss` and the C ABI binding against tests/image_loss_oracle.py run on
the device -- float64 to 1e-12 on every shape (index, halo and tile mistakes), float32 within 4 x the error of the float32
PyTorch formulation itself, weights, layouts, reproducibility, autocast, poisoned outputs, graph capture, errors.  The shapes
include interior tiles in both axes under both paddings and 256, 257, 297 and 513 partial sums (the finalize kernel takes 256
a pass); random shapes are in tests/test_gpu_fuzz_image_ops.py."""
import functools
import os
import re

import pytest
import torch as th

import image_loss_oracle as O
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tile():
    """(kIlTileW, kIlTileH) as csrc/image_loss.hip spells them."""
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "image_loss.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("kIlTileW", "kIlTileH"))


TW, TH = _tile()
# (shape, window_size, data_range)
CASES = [
    ((2, 3, 37, 53), 11, 1.0),    # several tiles with ragged tails
    ((1, 1, 7, 9), 11, 1.0),      # "same" only: the image is smaller than the window
    ((1, 1, 11, 11), 11, 1.0),    # "valid": a one-pixel map
    ((1, 2, 70, 45), 7, 1.0),
    ((1, 2, 70, 45), 7, 255.0),   # inputs scaled to match
    ((1, 1, TH, TW), 11, 1.0), ((1, 1, TH - 1, TW - 1), 11, 1.0), ((1, 1, TH + 1, TW + 1), 11, 1.0),  # the image against the tile
    ((1, 1, TH + 10, TW + 10), 11, 1.0), ((1, 1, TH + 9, TW + 9), 11, 1.0), ((1, 1, TH + 11, TW + 11), 11, 1.0),  # the "valid" map against it
    ((1, 2, 40, 40), 3, 1.0), ((1, 2, 40, 40), 5, 1.0), ((1, 2, 40, 40), 15, 1.0),
]
PARAMS = [(*c, p, w) for c in CASES for p in ("same", "valid") if p == "same" or min(c[0][2:]) >= c[1] for w in (False, True)]
# Past a 2 x 2 tile grid and past the 256 slots one pass of the finalize kernel takes (image_loss_oracle.STRUCTURAL_CASES;
# tests/test_image_loss_host.py proves the tile grids and slot counts, and that one view left out of a many-slot case moves
# each scalar by more than 100 x the float32 tolerance below)
STRUCTURAL = {name: [(shape, k, 1.0, p, w) for p in paddings for w in (False, True)] for name, (shape, k, paddings, _) in O.STRUCTURAL_CASES.items()}
PARAMS += [q for params in STRUCTURAL.values() for q in params]
IDS = [f"{'x'.join(map(str, s))}-w{k}-r{int(dr)}-{p}-{'weighted' if w else 'plain'}" for s, k, dr, p, w in PARAMS]
L1W, SSW = 0.7, 0.3


@functools.lru_cache(maxsize=None)
def problem(shape, k, data_range, padding, weighted):
    """Inputs (float32 values, so that both precisions see the same numbers) and the float64 oracle's results on the device,
    computed once and never modified: the map, an upstream gradient for it, its gradient, the two scalars, their gradients."""
    x32, y32 = O.case_inputs(shape, k, dtype=th.float32, data_range=data_range, device=DEV)
    w = O.make_mask(shape, seed=k, device=DEV) if weighted else None
    kw = dict(window_size=k, sigma=1.5 * k / 11, data_range=data_range, padding=padding)
    x, y = x32.double(), y32.double()
    ref = reference(x, y, w, kw, th.float64)
    return dict(x32=x32, y32=y32, x=x, y=y, w=w, kw=kw, ref=ref, h=ref["h"])


def reference(x, y, w, kw, dtype, h=None):
    """The oracle in `dtype`: map, grad of sum(h map), ssim, photometric loss and their gradients (autograd of the oracle)."""
    x, y = x.to(dtype), y.to(dtype)
    leaf = x.clone().requires_grad_(True)
    S = O.ssim(leaf, y, reduction="none", **kw)
    if h is None:
        gen = th.Generator().manual_seed(S.numel())
        h = (th.rand(S.shape, generator=gen, dtype=th.float64) * 2 - 1).to(DEV)
    (S * h.to(dtype)).sum().backward()
    out = dict(map=S.detach(), h=h, grad_map=leaf.grad)
    for name, fn in (("ssim", lambda a: O.ssim(a, y, w, **kw)), ("photo", lambda a: O.photometric_loss(a, y, w, L1W, SSW, **kw))):
        leaf = x.clone().requires_grad_(True)
        v = fn(leaf)
        v.backward()
        out[name], out["grad_" + name] = v.detach(), leaf.grad
    return out


def ours(x, y, w, kw, h):
    """The same quantities from drtk_amd."""
    import drtk_amd

    leaf = x.clone().requires_grad_(True)
    S = drtk_amd.ssim(leaf, y, reduction="none", **kw)
    (S * h.to(x.dtype)).sum().backward()
    out = dict(map=S.detach(), grad_map=leaf.grad)
    for name, fn in (("ssim", lambda a: drtk_amd.ssim(a, y, w, **kw)), ("photo", lambda a: drtk_amd.photometric_loss(a, y, w, L1W, SSW, **kw))):
        leaf = x.clone().requires_grad_(True)
        v = fn(leaf)
        assert v.ndim == 0 and v.dtype == x.dtype
        v.backward()
        out[name], out["grad_" + name] = v.detach(), leaf.grad
    return out


def ours_c_abi(x, y, w, kw, h):
    """The same quantities through the ctypes binding of the C ABI (poisoned outputs, and guards around them where asked for),
    with the scalars the forward leaves in device memory: `scalars_ssim`, `scalars_photo`."""
    from drtk_amd import capi

    cw = dict(window_size=kw["window_size"], sigma=kw["sigma"], data_range=kw["data_range"], valid=kw["padding"] == "valid")
    S, maps, scalars = capi.image_loss_forward(x, y, None, mode="map", with_maps=True, **cw)
    assert scalars is None
    out = dict(map=S, grad_map=capi.image_loss_backward(x, y, None, maps, h.to(x.dtype), None, mode="map", **cw))
    one = th.ones((), dtype=x.dtype, device=x.device)
    for name, mode in (("ssim", "ssim"), ("photo", "photometric")):
        cm = dict(cw, mode=mode, l1_weight=L1W, ssim_weight=SSW)
        v, maps, scalars = capi.image_loss_forward(x, y, w, with_maps=True, **cm)
        assert v.ndim == 0 and v.dtype == x.dtype and scalars.dtype == th.float64
        out[name], out["grad_" + name], out["scalars_" + name] = v, capi.image_loss_backward(x, y, w, maps, one, scalars, **cm), scalars
    return out


def err(a, b):
    return float((a.double() - b.double()).abs().max())


QUANTITIES = ("map", "ssim", "photo", "grad_map", "grad_ssim", "grad_photo")


def check_float64(got, ref):
    for name in QUANTITIES:
        assert got[name].shape == ref[name].shape, name
        e, top = err(got[name], ref[name]), max(1.0, float(ref[name].abs().max()))
        print(f"float64 {name}: max abs err {e:.3e}, max |ref| {top:.3e}")
        assert e <= 1e-12 * top, (name, e, top)


def check_float32(got, ref, form, data_range):
    for name in ("map", "grad_map", "grad_ssim", "grad_photo"):
        assert got[name].shape == ref[name].shape, name
        bar, e = err(form[name], ref[name]), err(got[name], ref[name])
        print(f"float32 {name}: kernel {e:.3e}, formulation {bar:.3e}, ratio {e / bar if bar else float('inf'):.2f}")
        assert e <= 4 * bar, (name, e, bar)
    eps, map_bar = th.finfo(th.float32).eps, err(form["map"], ref["map"])
    for name, tol in (("ssim", 4 * map_bar), ("photo", SSW * 4 * map_bar + L1W * 4 * eps * data_range)):
        e = err(got[name], ref[name])
        print(f"float32 {name}: kernel {e:.3e}, formulation {err(form[name], ref[name]):.3e}, bound {tol:.3e}")
        assert e <= tol, (name, e, tol)


def check_case(shape, k, data_range, padding, weighted, dtype, api=ours):
    """One case in one precision through `api` (`ours`, `ours_c_abi`) under this file's two bounds; -> what `api` returned."""
    p = problem(shape, k, data_range, padding, weighted)
    if dtype == th.float64:
        got = api(p["x"], p["y"], p["w"], p["kw"], p["h"])
        check_float64(got, p["ref"])
    else:
        form = reference(p["x32"], p["y32"], p["w"], p["kw"], th.float32, h=p["h"])
        got = api(p["x32"], p["y32"], p["w"], p["kw"], p["h"])
        check_float32(got, p["ref"], form, data_range)
    return got


@pytest.mark.parametrize("shape,k,data_range,padding,weighted", PARAMS, ids=IDS)
def test_float64_against_the_oracle(shape, k, data_range, padding, weighted):
    """Map, both scalars and every gradient within 1e-12 * max(1, max|ref|): the two differ by summation order only."""
    check_case(shape, k, data_range, padding, weighted, th.float64)


@pytest.mark.parametrize("shape,k,data_range,padding,weighted", PARAMS, ids=IDS)
def test_float32_within_four_times_the_formulations_own_error(shape, k, data_range, padding, weighted):
    """The bar per case: the error of the float32 PyTorch formulation (the oracle in float32 on this device) against the
    float64 oracle, maxima over elements, maps and gradients separately; the kernels stay within 4 x that (another
    summation order, fused multiply-adds).  The scalars are means of the map's elements (sums in double) and of |x - y|: no
    further off than 4 x the formulation's worst map element, plus 4 eps of the data range for the L1 term."""
    check_case(shape, k, data_range, padding, weighted, th.float32)


BASE = ((2, 3, 37, 53), 11, 1.0)


def _weights(shape):
    """name -> weight for the weights test, on the device."""
    N, _, H, W = shape
    mask = O.make_mask(shape, seed=3, device=DEV)
    gen = th.Generator().manual_seed(9)
    soft = th.rand(N, H, W, generator=gen, dtype=th.float64).to(DEV)
    one_view = mask.clone()
    one_view[0] = False
    return {
        "bool_NHW": mask, "bool_N1HW": mask[:, None], "float_NHW": soft, "float_N1HW": soft[:, None],
        "float_mask_with_holes": mask.double(), "zero_on_one_view": one_view, "zero_on_one_view_float": one_view.double() * soft,
    }


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_weights(padding):
    import drtk_amd

    shape, k, _ = BASE
    p = problem(shape, k, 1.0, padding, False)
    x, y, kw = p["x"], p["y"], p["kw"]
    for name, w in _weights(shape).items():
        wd = w if w.dtype == th.bool else w.double()
        ref, got = reference(x, y, wd, kw, th.float64, h=p["h"]), ours(x, y, wd, kw, p["h"])
        for q in ("ssim", "photo", "grad_ssim", "grad_photo"):
            e, top = err(got[q], ref[q]), max(1.0, float(ref[q].abs().max()))
            assert e <= 1e-12 * top, (name, q, e)
    # a bool mask and the same mask as numbers are the same call
    m = _weights(shape)["bool_NHW"]
    assert th.equal(drtk_amd.ssim(x, y, m, **kw), drtk_amd.ssim(x, y, m.double(), **kw))
    assert th.equal(drtk_amd.photometric_loss(p["x32"], p["y32"], m, **kw), drtk_amd.photometric_loss(p["x32"], p["y32"], m.float(), **kw))


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_all_zero_weight_gives_zero_without_nan(padding, dtype):
    """Both means are exactly 0 (photometric_loss is then the constant ssim_weight) and the gradient is exactly 0, all finite
    -- also with 257 partial sums, where the finalize kernel takes a second pass.  There, with a weight in the last view
    alone, the one live slot is the one that pass reaches: the results are those of the last view by itself, bit for bit
    (every other slot adds an exact zero), and they are not zero."""
    import drtk_amd

    many, k3, _, _ = O.STRUCTURAL_CASES["slots257"]
    for shape, k in (BASE[:2], (many, k3)):
        p = problem(shape, k, 1.0, padding, False)
        x, y = p["x"].to(dtype), p["y"].to(dtype)
        for zero in (th.zeros(shape[0], *shape[2:], dtype=th.bool, device=DEV), th.zeros(shape[0], 1, *shape[2:], dtype=dtype, device=DEV)):
            for fn, want in ((lambda a: drtk_amd.ssim(a, y, zero, **p["kw"]), 0.0),
                             (lambda a: drtk_amd.photometric_loss(a, y, zero, 1.0, 0.0, **p["kw"]), 0.0),
                             (lambda a: drtk_amd.photometric_loss(a, y, zero, 0.8, 0.25, **p["kw"]), 0.25)):
                leaf = x.clone().requires_grad_(True)
                v = fn(leaf)
                v.backward()
                assert float(v.detach()) == want
                assert bool(th.isfinite(leaf.grad).all()) and not bool(leaf.grad.any())
    last = many[0] - 1
    assert last == 256
    for live in (O.make_mask((1, *many[1:]), seed=5, device=DEV), th.rand(1, 1, *many[2:], generator=th.Generator().manual_seed(4), dtype=th.float64).to(dtype).to(DEV) + 0.25):
        w = th.zeros(many[0], *live.shape[1:], dtype=live.dtype, device=DEV)
        w[last] = live[0]
        for fn in (drtk_amd.ssim, lambda a, b, c, **kw: drtk_amd.photometric_loss(a, b, c, L1W, SSW, **kw)):
            leaf, alone = x.clone().requires_grad_(True), x[last:].clone().requires_grad_(True)
            v, v1 = fn(leaf, y, w, **p["kw"]), fn(alone, y[last:], live, **p["kw"])
            v.backward(), v1.backward()
            assert th.equal(v.detach(), v1.detach()) and float(v.detach()) != 0.0 and bool(th.isfinite(v.detach()))
            assert th.equal(leaf.grad[last:], alone.grad) and bool(alone.grad.any()) and not bool(leaf.grad[:last].any())


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_strided_tensors_are_read_in_place_and_equal_the_contiguous_call_bit_for_bit(dtype):
    import drtk_amd

    shape, k, _ = BASE
    p = problem(shape, k, 1.0, "same", True)
    x, y, w, kw = p["x"].to(dtype), p["y"].to(dtype), p["w"], p["kw"]
    base = ours(x, y, w, kw, p["h"])
    N, C, H, W = shape
    # channel slices of an RGBA render; a view slice; a row slice of a taller image
    rgba = th.full((N, C + 1, H, W), float("nan"), dtype=dtype, device=DEV)
    rgba[:, :C] = x
    views = th.full((2 * N, C, H, W), float("nan"), dtype=dtype, device=DEV)
    views[::2] = y
    tall = th.full((N, C, H + 5, W + 3), float("nan"), dtype=dtype, device=DEV)
    tall[:, :, 2:2 + H, :W] = x
    wide_w = th.zeros(N, H, W + 7, dtype=th.bool, device=DEV)
    wide_w[:, :, :W] = w
    for xs, ys, ws in ((rgba[:, :C], y, w), (x, views[::2], w), (tall[:, :, 2:2 + H, :W], views[::2], wide_w[:, :, :W])):
        assert not xs.is_contiguous() or not ys.is_contiguous()
        got = ours(xs, ys, ws, kw, p["h"])
        for name in base:
            assert th.equal(got[name], base[name]), name
    # the gradient of a slice lands in the slice
    leaf = rgba.clone().requires_grad_(True)
    drtk_amd.photometric_loss(leaf[:, :C], y, w, L1W, SSW, **kw).backward()
    assert th.equal(leaf.grad[:, :C], base["grad_photo"]) and not bool(leaf.grad[:, C].any())
    # a permuted NHWC view has W stride C: copied once, same results
    nhwc_x, nhwc_y = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), y.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert nhwc_x.stride(3) == C and not nhwc_x.is_contiguous()
    got = ours(nhwc_x, nhwc_y, w.transpose(1, 2).contiguous().transpose(1, 2), kw, p["h"])
    for name in base:
        assert th.equal(got[name], base[name]), name


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
def test_two_calls_are_bitwise_equal(dtype):
    shape, k, _ = BASE
    for padding in ("same", "valid"):
        p = problem(shape, k, 1.0, padding, True)
        x, y = p["x"].to(dtype), p["y"].to(dtype)
        a, b = ours(x, y, p["w"], p["kw"], p["h"]), ours(x, y, p["w"], p["kw"], p["h"])
        for name in a:
            assert th.equal(a[name], b[name]), name


def test_autocast_casts_half_inputs_to_float32():
    import drtk_amd

    shape, k, _ = BASE
    p = problem(shape, k, 1.0, "same", True)
    xh, yh, w, kw = p["x32"].half(), p["y32"].half(), p["w"], p["kw"]
    with pytest.raises(RuntimeError, match="not implemented for 'Half'"):
        drtk_amd.ssim(xh, yh, **kw)
    for wt in (w, w.half()):
        leaf = xh.clone().requires_grad_(True)
        with th.autocast("cuda", dtype=th.float16):
            a = drtk_amd.photometric_loss(leaf, yh, wt, **kw)
            s = drtk_amd.ssim(leaf, yh, wt, **kw)
            m = drtk_amd.ssim(xh, yh, reduction="none", **kw)
        assert a.dtype == s.dtype == m.dtype == th.float32
        a.backward()
        up = xh.float().requires_grad_(True)
        b = drtk_amd.photometric_loss(up, yh.float(), wt if wt.dtype == th.bool else wt.float(), **kw)
        b.backward()
        assert th.equal(a, b) and leaf.grad.dtype == th.float16 and th.equal(leaf.grad, up.grad.half())
        assert th.equal(s, drtk_amd.ssim(xh.float(), yh.float(), wt if wt.dtype == th.bool else wt.float(), **kw))
        assert th.equal(m, drtk_amd.ssim(xh.float(), yh.float(), reduction="none", **kw))


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_c_abi_binding_writes_every_element_and_nothing_stray(padding, dtype):
    """Through capi, whose outputs start as NaN (conftest.py sets DRTK_CAPI_POISON=1): every element of the map, of the three
    gradient maps and of grad_img is written, a no-grad call leaves no NaN in its scalars, and the results are the operators'."""
    import drtk_amd
    from drtk_amd import capi

    assert os.environ.get("DRTK_CAPI_POISON") == "1" and capi._POISON
    for shape, k in ((2, 3, 37, 53), 11), ((1, 2, 70, 45), 7), ((1, 1, TH + 1, TW + 1), 11):
        p = problem(shape, k, 1.0, padding, True)
        x, y, w, kw = p["x"].to(dtype), p["y"].to(dtype), p["w"], p["kw"]
        cw = dict(window_size=k, sigma=kw["sigma"], data_range=1.0, valid=padding == "valid")
        S, maps, scalars = capi.image_loss_forward(x, y, None, mode="map", with_maps=True, **cw)
        assert scalars is None and bool(th.isfinite(S).all()) and bool(th.isfinite(maps).all())
        assert th.equal(S, drtk_amd.ssim(x, y, reduction="none", **kw))
        h = p["h"].to(dtype)
        g = capi.image_loss_backward(x, y, None, maps, h, None, mode="map", **cw)
        assert bool(th.isfinite(g).all())
        leaf = x.clone().requires_grad_(True)
        (drtk_amd.ssim(leaf, y, reduction="none", **kw) * h).sum().backward()
        assert th.equal(g, leaf.grad)
        # no-grad: the scalars only
        out, maps, scalars = capi.image_loss_forward(x, y, w, mode="photometric", l1_weight=L1W, ssim_weight=SSW, **cw)
        assert maps is None and bool(th.isfinite(scalars).all()) and bool(th.isfinite(out))
        assert th.equal(out, drtk_amd.photometric_loss(x, y, w, L1W, SSW, **kw))
        assert float(scalars[0]) == float(capi.image_loss_forward(x, y, w, mode="ssim", **cw)[2][0])
        out, maps, scalars = capi.image_loss_forward(x, y, w, mode="photometric", l1_weight=L1W, ssim_weight=SSW, with_maps=True, **cw)
        one = th.ones((), dtype=dtype, device=DEV)
        g = capi.image_loss_backward(x, y, w, maps, one, scalars, mode="photometric", l1_weight=L1W, ssim_weight=SSW, **cw)
        leaf = x.clone().requires_grad_(True)
        drtk_amd.photometric_loss(leaf, y, w, L1W, SSW, **kw).backward()
        assert bool(th.isfinite(g).all()) and th.equal(g, leaf.grad)


def check_c_abi_case(shape, k, padding, weighted, dtype):
    """A case through the binding under this file's bounds (shared with tests/guarded_added_ops.py); where the forward leaves
    scalars they are finite and those of the Python API: ssim, and the l1 that photometric_loss(1, 0) returns by itself."""
    import drtk_amd

    got = check_case(shape, k, 1.0, padding, weighted, dtype, api=ours_c_abi)
    p = problem(shape, k, 1.0, padding, weighted)
    x, y = (p["x"], p["y"]) if dtype == th.float64 else (p["x32"], p["y32"])
    py = ours(x, y, p["w"], p["kw"], p["h"])
    for name in QUANTITIES:
        assert bool(th.isfinite(got[name]).all()) and th.equal(got[name], py[name]), name
    ssim, l1 = drtk_amd.ssim(x, y, p["w"], **p["kw"]), drtk_amd.photometric_loss(x, y, p["w"], 1.0, 0.0, **p["kw"])
    for name in ("scalars_ssim", "scalars_photo"):
        s = got[name]
        assert s.shape == (4,) and bool(th.isfinite(s).all()), (name, s)
        assert th.equal(s[0].to(dtype), ssim) and bool(s[2] > 0), (name, s, ssim)
    s = got["scalars_photo"]
    assert th.equal(s[1].to(dtype), l1) and bool(s[3] > 0) and th.equal(s[0], got["scalars_ssim"][0]), (s, l1)


SLOT_PARAMS = [(name, p) for name in O.SLOT_CASES for p in O.STRUCTURAL_CASES[name][2]]


@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,padding", SLOT_PARAMS, ids=[f"{n}-{p}" for n, p in SLOT_PARAMS])
def test_c_abi_binding_with_more_slots_than_one_finalize_pass_takes(name, padding, dtype):
    """The many-slot cases through capi, weighted: the bounds of this file, bit for bit the Python API, scalars finite."""
    shape, k, _, _ = O.STRUCTURAL_CASES[name]
    check_c_abi_case(shape, k, padding, True, dtype)


def test_graph_capture_of_forward_and_backward():
    """photometric_loss with its backward pass under torch.cuda.graph; a replay on refreshed inputs equals eager bit for bit."""
    import drtk_amd

    shape, k, _ = BASE
    p = problem(shape, k, 1.0, "same", True)
    x = p["x32"].clone().requires_grad_(True)
    y, w = p["y32"].clone(), p["w"].clone()

    def step():
        loss = drtk_amd.photometric_loss(x, y, w, L1W, SSW, **p["kw"])
        loss.backward()
        return loss

    captured = drtk_amd.capture_step(step, [x])
    new_x, new_y, new_w = (p["x32"].flip(-1) * 0.75 + 0.125), p["y32"].flip(-2), p["w"].flip(-1)
    with th.no_grad():
        x.copy_(new_x), y.copy_(new_y), w.copy_(new_w)
    loss = captured()
    th.cuda.synchronize()
    leaf = new_x.clone().requires_grad_(True)
    want = drtk_amd.photometric_loss(leaf, new_y, new_w, L1W, SSW, **p["kw"])
    want.backward()
    assert th.equal(loss, want.detach()) and th.equal(x.grad, leaf.grad)


def test_errors_on_the_device():
    import drtk_amd

    shape, k, _ = BASE
    p = problem(shape, k, 1.0, "same", False)
    x, y = p["x"], p["y"]
    for fn in (drtk_amd.ssim, drtk_amd.photometric_loss):
        with pytest.raises(RuntimeError, match="arguments exchanged"):
            fn(x, y.clone().requires_grad_(True))
        leaf = x.clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="double backward"):
            th.autograd.grad(fn(leaf, y), leaf, create_graph=True)
    # the symmetric call gives the gradient of the other image
    leaf = y.clone().requires_grad_(True)
    drtk_amd.ssim(leaf, x).backward()
    ref = y.clone().requires_grad_(True)
    O.ssim(x, ref).backward()
    assert err(leaf.grad, ref.grad) <= 1e-12
    with pytest.raises(ValueError):
        drtk_amd.ssim(x, y, window_size=4)
    with pytest.raises(RuntimeError, match="same device"):
        drtk_amd.ssim(x, y.cpu())
    assert th.autograd.gradcheck(
        lambda t: drtk_amd.photometric_loss(t, y[:1, :1, :9, :10], None, L1W, SSW, window_size=5, sigma=1.0), (x[:1, :1, :9, :10].clone().requires_grad_(True),),
        eps=1e-6, atol=1e-8, rtol=1e-6)
