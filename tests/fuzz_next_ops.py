"""Randomised sweep of the 'next row' ops -- sparse interpolation operators (incl. the device-side A^T A pattern
builder), screen_space_uv_derivative, pinhole transform -- against the CPU oracle / the f64 PyTorch formulation (not
collected by pytest: `python tests/fuzz_next_ops.py --cases 200` on a GPU box; a fixed subset runs as
tests/test_gpu_mipmap.py::test_randomised_sparse_uv_and_transform_cases).  Awkward image sizes, f32 / f64, shared and
per-view topology, random foreground masks and upstream gradients."""
import argparse
import os

os.environ.setdefault("DRTK_CAPI_POISON", "1")  # outputs of the ctypes binding pre-filled with NaN / sentinels (drtk_amd/capi.py _out)
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

DEV = "cuda:0"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f64_distance import assert_normal_matrix_values_within  # noqa: E402

# screen_space_uv_derivative: quantiles of the per-pixel error against the double result, the kernel's within this factor
# of the reference composite's own (the same principle as tests/f64_distance.py, on a distribution instead of a maximum).
# Round 3's kernel inverted two matrices like the composite and scattered around it (log10 ratio of the two 90 % quantiles
# over 197 cases: 1 % / 99 % points -0.28 / +0.51, hence a factor 4); since round 4 it evaluates G^-1 A and is the more
# accurate of the two (545 cases: -1.27 / +0.06 for the 90 % quantiles, -0.40 / +0.07 for the medians;
# tests/diag_uv_derivative_accuracy.py): the factor is 2.
K_F64 = 2.0


def _close(a, ref, what, atol=1e-5, rtol=1e-5):
    a = a.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    tol = atol + rtol * float(ref.abs().max()) if ref.numel() else atol
    err = float((a - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol, f"{what}: max abs err {err:.3e} > tol {tol:.3e}"


def make_case(seed):
    from drtk_amd import synthetic as S
    from drtk_amd.transform import transform

    g = th.Generator().manual_seed(5000 + seed)
    r = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    N = r(1, 3)
    H = [1, 2, 7, 16, 17, 33, 64, 65, 100][r(0, 8)]
    W = [1, 3, 4, 5, 8, 63, 64, 66, 100, 127, 130][r(0, 10)]
    dtype = th.float64 if r(0, 2) == 0 else th.float32
    v_world, vi = S.uv_sphere(r(3, 14), r(3, 18), lobes=0.1 * r(0, 2), dtype=th.float64)
    cams = S.ring_cameras(N, W, H, dtype=th.float64)
    per_view_v = r(0, 2) == 0
    vN = v_world[None].repeat(N, 1, 1)
    if per_view_v:
        vN = vN + 0.02 * th.randn(N, 1, 3, generator=g, dtype=th.float64)
    batched_vi = r(0, 3) == 0
    if batched_vi:
        vi = vi[None].repeat(N, 1, 1)
        if N > 1:
            vi[1] = vi[1].flip(-1)
    V = v_world.shape[0]
    vt = th.rand(N, V, 2, generator=g, dtype=th.float64)
    return dict(N=N, H=H, W=W, V=V, dtype=dtype, vN=vN.to(dtype), vi=vi.contiguous(), cams=tuple(c.to(dtype) for c in cams),
                cams64=cams, vN64=vN, vt=vt.to(dtype), batched_vi=batched_vi, seed=seed,
                mask_keep=th.rand(N, H, W, generator=g) > 0.2, g=g)


def run_case(c):
    """One case; with DRTK_CAPI_GUARD=g in the environment also: nothing was written outside an output or a workspace."""
    from drtk_amd import capi

    out = _run_case(c)
    capi.check_guards()
    return out


def _run_case(c):
    import oracle as O
    import drtk_amd
    from drtk_amd import capi
    from drtk_amd.transform import transform, transform_with_v_cam

    d = lambda x: x.to(DEV)  # noqa: E731
    N, H, W, V, dtype, vi, g = c["N"], c["H"], c["W"], c["V"], c["dtype"], c["vi"], c["g"]
    f64 = dtype == th.float64

    # ---- transform (forward + gradient wrt v) against the PyTorch formulation in f64 on the CPU
    v64 = c["vN64"].clone().requires_grad_(True)
    ref, _ = transform_with_v_cam(v64, *c["cams64"])
    gout = th.rand(ref.shape, dtype=th.float64, generator=g) * 2 - 1
    (ref * gout).sum().backward()
    vd = d(c["vN"]).requires_grad_(True)
    out = transform(vd, *(d(t) for t in c["cams"]))
    (out * d(gout.to(dtype))).sum().backward()
    ttol = dict(atol=1e-9, rtol=1e-11) if f64 else dict(atol=2e-3, rtol=2e-6)  # pixel coordinates are O(W): ~1 ulp at 1e2..1e3
    _close(out, ref, "transform", **ttol)
    _close(vd.grad, v64.grad, "transform grad", **(dict(atol=1e-8, rtol=1e-10) if f64 else dict(atol=1e-2, rtol=2e-5)))

    # ---- a consistent rasterization of these views (oracle), shared by the remaining ops
    v_pix = out.detach().cpu()
    _, index = O.rasterize(v_pix, vi, H, W)
    _, bary = O.render(v_pix, vi, index)
    dvi, dindex, dbary = d(vi), d(index), d(bary)

    # ---- sparse operators
    crow_o, col_o, val_o, rows_o = O.interpolation_matrix(vi, index, bary)
    crow, col, values, rows = capi.interpolation_matrix(dvi, dindex, dbary)
    assert th.equal(crow.cpu(), crow_o) and th.equal(col.cpu(), col_o) and th.equal(rows.cpu(), rows_o), "interpolation matrix structure"
    assert th.equal(values.cpu(), val_o), "interpolation matrix values"
    gim = (th.rand(val_o.shape, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    assert th.equal(capi.interpolation_matrix_backward(d(gim), dvi, dindex, rows).cpu(), O.interpolation_matrix_backward(gim, vi, index, bary, rows_o)), "interpolation matrix backward"
    vi3 = vi if vi.ndim == 3 else vi[None].expand(N, -1, -1)  # the oracle's builder takes the expanded topology, like the reference
    ncrow_o, ncol_o, pair_o = O.normal_matrix_structure(vi3, V)
    nnz = ncol_o.numel()
    M = drtk_amd.interpolation_normal_matrix(dvi, dindex, dbary, V)  # pattern built on the device
    assert th.equal(M.crow_indices().cpu(), ncrow_o) and th.equal(M.col_indices().cpu(), ncol_o), "A^T A pattern"
    nv_o = O.normal_matrix_values(pair_o, index, bary, nnz)
    if f64:
        tol = dict(atol=1e-12, rtol=1e-10)
        _close(M.values(), nv_o, "A^T A values (python api)", **tol)
        _close(capi.interpolation_normal_matrix_values(d(pair_o), dindex, dbary, nnz), nv_o, "A^T A values", **tol)
    else:
        # An entry of A^T A sums one product per pixel of the triangles around a vertex pair -- up to N*H*W float32 terms,
        # and two float32 summations of that many terms in different orders (the oracle's loop, the kernel's atomics; the
        # reference's CUDA kernel is a third) differ by ~ sqrt(terms) * eps of the sum (seed 202311: 1.02e-5 of max|ref|).
        # So: against the same sums carried in double, as near as the oracle's own float32 loop up to a factor
        # (tests/f64_distance.py); every term is a product of non-negative barycentrics, so what was accumulated is the
        # entry itself.
        nv_64 = O.normal_matrix_values(pair_o, index, bary.double(), nnz)
        assert_normal_matrix_values_within(M.values(), nv_o, nv_64, "A^T A values (python api)")
        assert_normal_matrix_values_within(capi.interpolation_normal_matrix_values(d(pair_o), dindex, dbary, nnz), nv_o, nv_64, "A^T A values")
    tol = dict(atol=1e-12, rtol=1e-10) if f64 else dict(atol=1e-5, rtol=1e-5)
    gnm = (th.rand(nnz, generator=g, dtype=th.float64) * 2 - 1).to(dtype)
    _close(capi.interpolation_normal_matrix_values_backward(d(gnm), d(pair_o), dindex, dbary), O.normal_matrix_values_backward(gnm, pair_o, index, bary),
           "A^T A values backward", **tol)

    # ---- screen_space_uv_derivative (mask within the foreground: background pixels are a documented difference)
    if c["batched_vi"]:
        return  # the op takes one topology for all views, like the reference
    mask = (index != -1) & c["mask_keep"]
    campos, camrot, focal = c["cams"][0], c["cams"][1], c["cams"][2]
    got = capi.screen_space_uv_derivative(d(c["vN"]), d(c["vt"]), dvi, dvi, dindex, dbary, d(mask), d(campos), d(camrot), d(focal))
    try:
        want = O.screen_space_uv_derivative(c["vN"], c["vt"], vi, vi, index, bary, mask, campos, camrot, focal)
    except th.linalg.LinAlgError:
        # A face with zero UV area: the reference's face_dpdt (drtk/utils/geometry.py:71-82) inverts every face's UV
        # edge matrix with th.inverse, which RAISES for the whole call -- there is no reference output for this mesh.
        # The kernel is per pixel (include/drtk_amd.h): it must still run, and write 0 wherever index is -1 / mask is 0.
        assert bool((got.cpu()[~mask] == 0).all()), "screen_space_uv_derivative: background / masked pixels must be 0"
        return "reference undefined: a face with zero UV area makes the reference composite raise"
    if f64:
        # pins the formula -- per pixel, and aware of the conditioning of the REFERENCE's evaluation: the composite inverts
        # the UV edge matrix A and later the product A^-1 G again; on a face that is a sliver in UV space its own result
        # moves when an input moves by one ulp (seed 460768: one pixel at 6.8e13, median 0.046, moving by 10 %).  The
        # kernel evaluates G^-1 A and has no such error, so the distance between the two is the composite's: bounded by
        # what the composite does on inputs one ulp apart, and not compared at all where that exceeds 1e-3 of the value
        # (fewer than four digits left in the float64 reference).
        signs = 1.0 - 2.0 * (th.arange(c["vt"].numel(), dtype=th.float64) % 2).reshape(c["vt"].shape)  # +1, -1, +1, ...
        want_ulp = O.screen_space_uv_derivative(c["vN"], c["vt"] * (1 + 2.0 ** -52 * signs), vi, vi, index, bary, mask, campos, camrot, focal)
        moved = (want_ulp - want).abs()
        unstable = moved.amax((-1, -2)) > 1e-3 * want.abs().amax((-1, -2))
        err = (got.cpu() - want).abs()
        bound = 1e-11 + 1e-10 * want.abs() + 8 * moved
        worst = float((err - bound)[~unstable].max()) if bool((~unstable).any()) else 0.0
        assert worst <= 0, f"screen_space_uv_derivative (f64): a pixel is {worst:.3e} beyond its conditioning-aware bound"
        assert int(unstable.sum()) <= 0.05 * max(int(mask.sum()), 20), "screen_space_uv_derivative (f64): too many pixels set aside as unstable in the reference"
        return
    # f32: the result is large and ill-conditioned for triangles seen edge-on; there two f32 evaluations with different
    # operation orders (the reference's PyTorch composite: two LU inverses; the kernel: G^-1 A in closed form) scatter
    # around the exact value by up to 1e-1 and comparing them WITH EACH OTHER means nothing.  Both are measured against the
    # f64 result instead, and the bar is on the DISTRIBUTION of the per-pixel error: the kernel at least as accurate as the
    # reference formulation is in f32 (median, 90 % quantile; in fact about twice as accurate, see K_F64), plus a loose
    # bound on the single worst pixel -- heavy-tailed luck for either evaluation -- against gross errors.
    truth = O.screen_space_uv_derivative(c["vN"].double(), c["vt"].double(), vi, vi, index, bary.double(), mask, campos.double(),
                                         camrot.double(), focal.double())
    e_g = (got.cpu().double() - truth).abs().amax((-1, -2))
    e_r = (want.double() - truth).abs().amax((-1, -2))
    assert bool(th.isfinite(got).all())
    # EVERY pixel of every case, in units of the problem's own sensitivity: how far the f64 result moves when each vertex
    # and uv coordinate moves by half an f32 ulp (two sign patterns), plus one ulp of the value.  A forward-stable
    # evaluation stays within a small multiple of that however ill-conditioned the pixel is.  Measured over 546 cases /
    # 944 k pixels (tests/diag_uv_derivative_conditioning.py): kernel 50 / 90 / 99 / 99.9 / 100 % = 0.39 / 0.95 / 1.8 / 3.0 /
    # 19 units -- the reference's float32 composite 0.52 / 1.8 / 16 / 108 / 2405.  The bar: 64.
    sens = th.zeros_like(e_g)
    for ph in (0, 1):
        sg = lambda t: 1.0 - 2.0 * ((th.arange(t.numel(), dtype=th.float64) + ph) % 2).reshape(t.shape)  # noqa: E731
        moved = O.screen_space_uv_derivative(c["vN"].double() * (1 + 2.0 ** -24 * sg(c["vN"])), c["vt"].double() * (1 + 2.0 ** -24 * sg(c["vt"])),
                                             vi, vi, index, bary.double(), mask, campos.double(), camrot.double(), focal.double())
        sens = th.maximum(sens, (moved - truth).abs().amax((-1, -2)))
    unit = sens + 2.0 ** -23 * truth.abs().amax((-1, -2))
    over = (e_g / unit.clamp_min(1e-300))[mask]
    assert over.numel() == 0 or float(over.max()) <= 64.0, \
        f"screen_space_uv_derivative (f32): a pixel is {float(over.max()):.1f} units of its own sensitivity off the f64 result (bar 64)"
    scale = float(truth.abs().max())
    assert float(e_g.max()) <= 100 * float(e_r.max()) + 1e-4 * scale + 1e-30, \
        f"screen_space_uv_derivative (f32): worst pixel {float(e_g.max()):.3e} vs f64, the reference composite's {float(e_r.max()):.3e}"
    if int(mask.sum()) >= 20:
        px_scale = truth.abs().amax((-1, -2)).clamp_min(1e-30)
        rg, rr = (e_g / px_scale)[mask], (e_r / px_scale)[mask]
        # (absolute 1e-6, or the composite's own median on the same pixels where that is larger: on a handful of faces the
        # median IS one face's rounding error -- seeds 450324 and 760460, two faces each: composite 1.1e-6 and 2.0e-7, round
        # 3's kernel 1.1e-6 and 2.9e-6, this one 4e-8 and 1e-7)
        med_g, med_r = float(rg.median()), float(rr.median())
        assert med_g <= max(1e-6, K_F64 * med_r), f"screen_space_uv_derivative (f32): median relative error {med_g:.3e}, the composite's {med_r:.3e}"
        # The rounding error of an evaluation is a property of the FACE (its matrices are per-face constants), shared by
        # all of its pixels: the sample behind a quantile over pixels is the number of faces.  So the 90 % quantile is
        # compared only where enough faces stand behind it.
        if int(index[mask].unique().numel()) >= 40:
            q90g, q90r = float(th.quantile(rg, 0.9)), float(th.quantile(rr, 0.9))
            assert q90g <= K_F64 * q90r + 1e-6, f"screen_space_uv_derivative (f32): 90 % quantile of the relative error {q90g:.3e}, the composite's {q90r:.3e}"


def describe(c):
    return (f"N={c['N']} H={c['H']} W={c['W']} V={c['V']} F={c['vi'].shape[-2]} {str(c['dtype']).split('.')[-1]} "
            f"batched_vi={c['batched_vi']}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--first", type=int, default=0)
    a = ap.parse_args()
    bad, undefined = 0, 0
    for seed in range(a.first, a.first + a.cases):
        c = make_case(seed)
        try:
            note = run_case(c)
            if note:
                undefined += 1
                print(f"NOTE seed {seed}: {describe(c)}: {note}", flush=True)
        except Exception as e:
            bad += 1
            print(f"FAIL seed {seed}: {describe(c)}: {type(e).__name__}: {str(e)[:160]}", flush=True)
    print(f"{a.cases - bad}/{a.cases} cases passed" + (f" ({undefined} of them only up to screen_space_uv_derivative: reference undefined)" if undefined else ""))
    sys.exit(1 if bad else 0)
