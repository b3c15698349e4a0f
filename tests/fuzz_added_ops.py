"""TEST INFRASTRUCTURE ONLY (not collected by pytest) -- seeded random shapes for five operators that were tested on fixed
shape lists only: `filter2d`, `composite_layers`, `shade`, `mesh_laplacian` / `cotangent_weights` and `msi`, each through the
ctypes binding of the C ABI (poisoned outputs, and with DRTK_CAPI_GUARD sentinels around every output and workspace) and
through the Python API under autograd.  The two routes agree bit for bit (msi: `out` bit for bit, the texture gradient,
which is summed with atomics, within the float64 bound of tests/test_gpu_msi.py on a float64 run of both routes).  Every
result is compared with the operator's own oracle under the bounds of its own GPU test module, whose helpers this script
imports: no bound is stated here.

usage: python tests/fuzz_added_ops.py [--first S] [--cases K]      cases make_case(S) .. make_case(S + K - 1)

"Towards X" below: one draw in three picks from the list X, the others are uniform in the stated range.

filter2d: up, down 1 .. 8 and k 1 .. 32 where the forward and its gradient call are defined; three cases in four a generic
triple, one in four a tuned family (which also runs through the generic kernel, as
test_tuned_and_generic_instantiations_agree requires); output sizes towards 1, 2 and one either side of 16, 32, 64, 128,
else 1 .. 140; the input the multiple of `down` whose output is nearest; 1 .. 7 planes as N x C; float32 / float64 /
float16; reflection only where torch's rule admits it for the forward and the gradient call; x contiguous or a column
slice of a wider tensor; a generic case runs three triples at its output sizes (so that 240 seeds hold over 80 of them).  Against filter2d_oracle.apply / gradient under test_gpu_filter2d.check_inputs.

composite_layers: K 1 .. 8, C towards 1, 3, 4, 5, 16, 17 (else 1 .. 17), N 1 .. 3; pixel counts towards one either side of
P, 256 P and 512 P (P: the pixels of a lane, kPix of csrc/composite.hip, for the drawn dtype and pass), else H, W 1 .. 40;
no index / trailing -1 layers / holes; no background / one per view / one view expanded; split tensors / one rgba tensor /
channel slices of wider tensors; one alpha in ten exactly 0, one in ten exactly 1; a random non-empty subset of colour,
alpha and background requires a gradient; grad_T present or absent.  The forward bit for bit against
test_gpu_composite_layers.loop in the same dtype on the device, the gradients under its `bounds`.

shade: every option on or off (each case runs its drawn setting and the one with every option the other way), a random subset of the parameters per view, albedo an image or a parameter, C 1 .. 4,
N 1 .. 4, pixel counts towards {P-1, P, P+1, B-1, B, B+1, 2B+3} of shade_oracle.kernel_constants(), else H, W 1 .. 70; one
case in sixteen S B - 1 or (S+1) B + 1 pixels (more rows than one pass of the finalize kernel); one of
test_gpu_shade.LAYOUTS or contiguous; a random subset of the float inputs requires a gradient.  Inputs by
shade_oracle.build_case (its margins); against shade_oracle.reference under test_gpu_shade.check.

laplacian: soup_mesh(V 3 .. 300, F 1 .. 600) / grid_mesh(2 .. 12, 2 .. 12) / fan_mesh(valence towards 255, 256, 257, 511,
512, 513 -- such a case runs all six --, else 2 .. 700: a fan of valence 1 is one
duplicate-corner face, all its results are zero, which the oracle's check does not admit); one in four with_degenerates; N 1 .. 4; C towards 1, 3, 4, 5, 8, 9 (else 1 .. 9); topology shared or
per view; vi int32 / int64; weights in one of test_gpu_laplacian.W_LAYOUTS or the output of cotangent_weights (the full
pipeline); float32 / float64; a random subset of x / weights / v requires a gradient.  Against laplacian_oracle under
test_gpu_laplacian.compare; the chunk kernel of the long rows is launched exactly where a row has more than
DRTK_GEOMETRY_CHUNK entries.

msi: rays towards 1, 255, 256, 257, 511, 512, 513 (else 1 .. 700), L 1 .. 6, H and W towards 1, 2 (else 1 .. 17),
sub_step_count 1 .. 3, the four sphere ranges, two stop thresholds, two sigma ranges and three origin radii of
msi_oracle.CASES, texture float32 / float64; fragile rays are drawn again until none is left
(msi_oracle.build_case(redraw=True)), so every ray is compared.  Under test_gpu_msi.check_against_the_oracle.

tests/test_gpu_fuzz_added_ops.py runs seeds 0 .. 239 in six blocks of 40 (tests/test_fuzz_added_ops_host.py shows what
they hold); tests/guarded_added_ops.py runs the first 20 under guards.
Measured on an MI355X: a block of 40 cases takes 0.5 to 3.2 s (the first one, with the first use of every library, the
most), oracles included; `--first 0 --cases 240` runs its cases in 10.6 s, 13.2 s of wall time with the start of the process.
With csrc/filter2d.hip's generic `phase` one too large where up > 1 and down > 1, 40 of the 240 seeds fail (seed 2 the
first); with the chunk split of csrc/torch_ops/geometry.cpp taken at `>= kChunk`, seeds 69 and 146 (a row of 256 entries).
"""
import argparse
import os

os.environ.setdefault("DRTK_CAPI_POISON", "1")  # outputs of the ctypes binding pre-filled with NaN / sentinels (drtk_amd/capi.py _out)
import contextlib
import io
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import filter2d_oracle as FO  # noqa: E402
import laplacian_oracle as LO  # noqa: E402
import msi_oracle as MO  # noqa: E402
import shade_oracle as SO  # noqa: E402

DEV = "cuda:0"
OPS = ("filter2d", "composite_layers", "shade", "laplacian", "msi")
DTYPES = {"f32": th.float32, "f64": th.float64, "f16": th.float16}

F2D_MAX_FACTOR, F2D_MAX_TAPS, F2D_MAX_OUT, F2D_GENERIC_RUNS = 8, 32, 140, 3
F2D_NEAR = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
COMPOSITE_NEAR_C = [1, 3, 4, 5, 16, 17]
COMPOSITE_INDEX, COMPOSITE_BACKGROUND, COMPOSITE_FORM = ("none", "trailing", "holes"), ("none", "per_view", "expanded"), ("split", "rgba", "channel_slice")
SHADE_LAYOUTS = ("contiguous", "channel_slices", "view_slice", "expanded_background", "w_strided", "offset_one_element", "cropped_columns")
SHADE_FLOATS = ("normal_img", "pos_img", "albedo", "background", "light_dir", "ambient", "specular", "shininess")
LAPLACIAN_NEAR_VALENCE, LAPLACIAN_NEAR_C = [255, 256, 257, 511, 512, 513], [1, 3, 4, 5, 8, 9]  # one and two chunks of DRTK_GEOMETRY_CHUNK entries
LAPLACIAN_WEIGHTS = ("none", "F3", "1F3", "NF3", "NF3_expand", "cotangent")  # test_gpu_laplacian.W_LAYOUTS, and the full pipeline
MSI_NEAR_RAYS = [1, 255, 256, 257, 511, 512, 513]
MSI_SPHERES, MSI_STOP, MSI_SIGMA, MSI_RADIUS = ((1.0, 0.0), (1.0, 0.05), (1.0, 0.1), (2.0, 0.5)), (1e-7, 1e-2), ((-0.5, 2.5), (0.0, 12.0)), (0.3, 0.8, 2.5)


# ---- what the cases are drawn from ---------------------------------------------------------------------------------------------
def f2d_defined(up, down, k):
    """Are the forward (up, down, k) and its gradient call (down, up, k, backward) defined (on an axis long enough)?"""
    try:
        FO.geometry(1 << 20, k, up, down)
        FO.geometry(1 << 20, k, down, up, backward=True)
    except ValueError:
        return False
    return True


def f2d_triples():
    """(the generic triples, the tuned families) within the factors and taps drawn here"""
    every = [(u, d, k) for u in range(1, F2D_MAX_FACTOR + 1) for d in range(1, F2D_MAX_FACTOR + 1) for k in range(1, F2D_MAX_TAPS + 1)
             if f2d_defined(u, d, k)]
    return {t for t in every if t not in FO.FAMILIES}, [t for t in every if t in FO.FAMILIES]


def f2d_axis(target, up, down, k):
    """(n, out): the input size n, a multiple of `down`, whose output size is nearest `target`"""
    best = None
    for m in range(1, 1 << 20):
        n = m * down
        try:
            out = FO.geometry(n, k, up, down)[2]
        except ValueError:  # an output smaller than 1
            continue
        if best is None or abs(out - target) < abs(best[1] - target):
            best = (n, out)
        if out >= target:
            return best


def composite_pix(dtype, K, backward):
    """kPix<T, K, BACKWARD> of csrc/composite.hip (tests/test_fuzz_added_ops_host.py holds the source to this expression)"""
    return (16 // (4 if dtype == "f32" else 8)) // (2 if backward and K > 4 else 1)


def plane(total):
    """(H, W) with H W = total and W the divisor of total nearest below its square root"""
    w = max(d for d in range(1, int(total ** 0.5) + 1) if total % d == 0)
    return total // w, w


def soup_is_possible(V, seed):
    """Has soup_mesh(V, ., seed) a face to draw?  (It draws the vertices first, then faces until enough of them have
    corner angles above 0.4: with a handful of vertices there may be none.)"""
    if V > 12:
        return True
    v = np.random.default_rng(seed).uniform(-1, 1, (V, 3))
    for a in range(V):
        for b in range(a + 1, V):
            for c in range(b + 1, V):
                if min(corner_angles(v[[a, b, c]])) > 0.4:
                    return True
    return False


def corner_angles(p):
    """the three corner angles of the triangle p [3,3] (numpy)"""
    out = []
    for k in range(3):
        e1, e2 = p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]
        out.append(float(np.arccos(np.clip(np.dot(e1, e2) / (np.linalg.norm(e1) * np.linalg.norm(e2)), -1, 1))))
    return out


_F2D_TRIPLES = []


def make_case(seed):
    """A dict of plain numbers and names; the tensors are made from them in run_case."""
    g = th.Generator().manual_seed(1000003 * seed + 31)
    r = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    pick = lambda seq: seq[r(0, len(seq) - 1)]  # noqa: E731
    towards = lambda near, lo, hi: pick(near) if r(0, 2) == 0 else r(lo, hi)  # noqa: E731
    flag = lambda: r(0, 1) == 1  # noqa: E731
    subset = lambda names: tuple(k for k in names if flag())  # noqa: E731
    op = pick(OPS)
    c = dict(seed=seed, op=op)
    if op == "filter2d":
        if not _F2D_TRIPLES:
            _F2D_TRIPLES.extend(f2d_triples())
        generic, tuned = _F2D_TRIPLES
        # One op in five and three generic cases in four are 36 generic cases in 240 seeds, and the seeds are to hold 80
        # generic triples: a generic case draws F2D_GENERIC_RUNS triples, each run at the case's drawn output sizes, planes,
        # type and layout (a tuned case one family).
        c["tuned"] = r(0, 3) == 0
        targets = [towards(F2D_NEAR, 1, F2D_MAX_OUT) for _ in range(2)]
        runs = []
        while len(runs) < (1 if c["tuned"] else F2D_GENERIC_RUNS):
            if c["tuned"]:
                up, down, k = pick(tuned)
            else:
                up, down, k = r(1, F2D_MAX_FACTOR), r(1, F2D_MAX_FACTOR), r(1, F2D_MAX_TAPS)
                if (up, down, k) not in generic:
                    continue
            (H, OH), (W, OW) = (f2d_axis(t, up, down, k) for t in targets)
            if FO.geometry(OH, k, down, up, backward=True)[2] != H or FO.geometry(OW, k, down, up, backward=True)[2] != W:
                continue
            reflect_ok = all(FO.reflect_ok(n, k, up, down) and FO.reflect_ok(o, k, down, up, backward=True) for n, o in ((H, OH), (W, OW)))
            runs.append(dict(up=up, down=down, k=k, H=H, W=W, OH=OH, OW=OW, padding=pick(FO.BOTH) if reflect_ok else "zeros"))
        planes = r(1, 7)
        N = pick([d for d in range(1, planes + 1) if planes % d == 0])
        c.update(runs=tuple(tuple(run.items()) for run in runs), N=N, C=planes // N, dtype=pick(("f32", "f64", "f16")),
                 layout=pick(("contiguous", "column_slice")))
    elif op == "composite_layers":
        c.update(K=r(1, 8), C=towards(COMPOSITE_NEAR_C, 1, 17), N=r(1, 3), dtype=pick(("f32", "f64")), near_pass=pick(("forward", "backward")))
        P = composite_pix(c["dtype"], c["K"], c["near_pass"] == "backward")
        if r(0, 2) == 0:
            c["H"], c["W"] = plane(pick([t for t in (P - 1, P + 1, 256 * P - 1, 256 * P + 1, 512 * P - 1, 512 * P + 1) if t >= 1]))
        else:
            c["H"], c["W"] = r(1, 40), r(1, 40)
        c.update(index=pick(COMPOSITE_INDEX), background=pick(COMPOSITE_BACKGROUND), form=pick(COMPOSITE_FORM), grad_T=flag())
        names = ("color", "alpha") + (("background",) if c["background"] != "none" else ())
        c["needs"] = subset(names) or (pick(names),)
    elif op == "shade":
        c.update(index=flag(), specular=flag(), background=flag(), gamma=2.2 if flag() else None, per_view=subset(tuple(SO.PARAMS)),
                 albedo_img=flag(), C=r(1, 4), N=r(1, 4), dtype=pick(("f32", "f64")))
        P, B, S, _ = SO.kernel_constants()
        P, B = P[DTYPES[c["dtype"]]], B[DTYPES[c["dtype"]]]
        c["many_rows"] = r(0, 15) == 0
        if c["many_rows"]:
            c["H"], c["W"] = SO._odd_width(pick((S * B - 1, (S + 1) * B + 1)))
        elif r(0, 2) == 0:
            c["H"], c["W"] = SO._odd_width(pick([t for t in (P - 1, P, P + 1, B - 1, B, B + 1, 2 * B + 3) if t >= 1]))
        else:
            c["H"], c["W"] = r(1, 70), r(1, 70)
        c["layout"] = pick(SHADE_LAYOUTS)
        c["needs"] = subset(SHADE_FLOATS)  # (of those, the inputs a run has: shade_runs)
    elif op == "laplacian":
        mesh = pick(("soup", "grid", "fan"))
        if mesh == "soup":
            c.update(mesh=mesh, V=r(3, 300), F=r(1, 600), mesh_seed=r(0, 10 ** 6))
            while not soup_is_possible(c["V"], c["mesh_seed"]):
                c["mesh_seed"] += 1
        elif mesh == "grid":
            c.update(mesh=mesh, rows=r(2, 12), cols=r(2, 12), mesh_seed=r(0, 10 ** 6))
        else:
            # Some fifteen fans in 240 seeds, a third of them towards the list, do not hold four given values of its six (seeds
            # 0 .. 239: eleven fans, two of them towards the list): a case drawn towards the list runs every fan of it
            # (laplacian_runs)
            c.update(mesh=mesh, valences=tuple(LAPLACIAN_NEAR_VALENCE) if r(0, 2) == 0 else (r(2, 700),))
        c.update(degenerate=r(0, 3) == 0, N=r(1, 4), C=towards(LAPLACIAN_NEAR_C, 1, 9), per_view=flag(), vi_dtype=pick(("int32", "int64")),
                 weights=pick(LAPLACIAN_WEIGHTS), dtype=pick(("f32", "f64")))
        c["needs"] = subset(("x", "weights", "v"))
    else:
        c.update(rays=towards(MSI_NEAR_RAYS, 1, 700), L=r(1, 6), H=towards([1, 2], 1, 17), W=towards([1, 2], 1, 17), sub_step_count=r(1, 3),
                 spheres=pick(MSI_SPHERES), stop_thresh=pick(MSI_STOP), sigma=pick(MSI_SIGMA), radius=pick(MSI_RADIUS), dtype=pick(("f32", "f64")))
    return c


def describe(c):
    return " ".join(f"{k}={v}" for k, v in c.items())


# ---- filter2d ----------------------------------------------------------------------------------------------------------------------
def f2d_runs(c):
    """the runs of a case as dicts (up, down, k, H, W, OH, OW, padding)"""
    return [dict(run) for run in c["runs"]]


def f2d_inputs(c, i):
    """(x, f, grad_out) of the case's run i: float32 on the CPU, f random in [-1, 1)"""
    run = f2d_runs(c)[i]
    g = th.Generator().manual_seed(10 * c["seed"] + i)
    f = th.rand(run["k"], generator=g) * 2 - 1
    x = th.rand(c["N"], c["C"], run["H"], run["W"], generator=g) * 2 - 1
    gout = th.rand(c["N"], c["C"], run["OH"], run["OW"], generator=g) * 2 - 1
    return x, f, gout


def run_filter2d(c):
    import test_gpu_filter2d as T

    for i in range(len(c["runs"])):
        run_filter2d_once(c, i, T)


def run_filter2d_once(c, i, T):
    run = f2d_runs(c)[i]
    dtype, up, down, padding = DTYPES[c["dtype"]], run["up"], run["down"], run["padding"]
    x, f, gout = f2d_inputs(c, i)
    # the binding on contiguous tensors against the oracle (and, a tuned family, against the generic kernel)
    T.check_inputs(x, f, gout, up, down, dtype, padding, FO.expected_on(x, f, gout, up, down, padding, dtype == th.float16))
    xd, fd, gd = x.to(DEV, dtype), f.to(DEV), gout.to(DEV, dtype)
    base = T.hip_on(xd, fd, gd, up, down, padding, "capi")
    if c["layout"] == "column_slice":
        wide = th.full((*xd.shape[:3], xd.shape[3] + 3), float("nan"), dtype=dtype, device=DEV)
        wide[..., 1:1 + xd.shape[3]] = xd
        xd = wide[..., 1:1 + xd.shape[3]]
    for api in ("capi", "python"):
        got = T.hip_on(xd, fd, gd, up, down, padding, api)
        for a, b, what in zip(got, base, ("out", "grad_x")):
            assert a.dtype == dtype and a.shape == b.shape and th.equal(a, b), f"{api}, x {c['layout']}: {what} differs from the binding on a contiguous x"


# ---- composite_layers ----------------------------------------------------------------------------------------------------------------
def composite_inputs(c):
    """color, alpha, background, index, g_img, g_T on the CPU in the case's dtype (the background of `expanded`: every view
    that of view 0), as test_gpu_composite_layers.problem makes them but for the alphas of exactly 0 and 1: one in ten each."""
    import test_gpu_composite_layers as T

    N, K, C, H, W = c["N"], c["K"], c["C"], c["H"], c["W"]
    dtype = DTYPES[c["dtype"]]
    g = th.Generator().manual_seed(c["seed"])
    rand = lambda *s: th.rand(*s, generator=g, dtype=th.float64)  # noqa: E731
    color = (rand(N, K, C, H, W) * 2 - 1).to(dtype)
    alpha, u = rand(N, K, H, W), rand(N, K, H, W)
    alpha[u < 0.1], alpha[u > 0.9] = 0.0, 1.0
    bg = (rand(N, C, H, W) * 2 - 1).to(dtype)
    if c["background"] == "expanded":
        bg = bg[:1].expand(N, -1, -1, -1).contiguous()
    count = th.randint(0, K + 1, (N, 1, H, W), generator=g)  # valid layers per pixel, -1 entries trailing
    index = th.where(th.arange(K)[None, :, None, None] < count, th.randint(0, 1000, (N, K, H, W), generator=g), -1)
    if c["index"] == "holes":  # a -1 between valid layers
        index = th.where(rand(N, K, H, W) < 0.25, -1, index)
    g_img = ((rand(N, C, H, W) * 2 - 1) * T.G).to(dtype)
    g_T = ((rand(N, 1, H, W) * 2 - 1) * T.G).to(dtype)
    return color, alpha.to(dtype), (bg if c["background"] != "none" else None), (index.int() if c["index"] != "none" else None), g_img, g_T


def run_composite_layers(c):
    import drtk_amd
    import test_gpu_composite_layers as T
    from drtk_amd import capi

    dtype, N, needs = DTYPES[c["dtype"]], c["N"], c["needs"]
    color, alpha, bg, index, g_img, g_T = composite_inputs(c)
    # the float64 oracle: the loop on the CPU and autograd
    c64, a64, b64 = T.f64(color), T.f64(alpha), (None if bg is None else T.f64(bg))
    ri, rT = T.loop(c64, a64, index, b64)
    ((ri * g_img.double()).sum() + ((rT * g_T.double()).sum() if c["grad_T"] else 0)).backward()
    ref = dict(img=ri.detach(), T=rT.detach(), gc=c64.grad, ga=a64.grad, gb=None if b64 is None else b64.grad)
    M = max(float(color.abs().max()), float(bg.abs().max()) if bg is not None else 0.0)
    bound = T.bounds(c["K"], c["C"], dtype, M)
    color, alpha, g_img, g_T = (t.to(DEV) for t in (color, alpha, g_img, g_T))
    index = None if index is None else index.to(DEV)
    bg = None if bg is None else bg.to(DEV)
    want_img, want_T = T.loop(color, alpha, index, bg)  # the loop, same dtype, on the device
    if not c["grad_T"]:
        g_T = None
    want = dict(want_color="color" in needs, want_alpha="alpha" in needs, want_background="background" in needs)

    def form(col, alp):
        """(color, alpha) as the binding and the operator take them in the case's form, made from col and alp"""
        if c["form"] == "split":
            return col, alp
        if c["form"] == "rgba":
            return th.cat([col, alp[:, :, None]], 2), None
        nan = lambda *s: th.full(s, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
        return th.cat([nan(*col.shape[:2], 1, *col.shape[3:]), col], 2)[:, :, 1:], th.stack([nan(*alp.shape), alp], 2)[:, :, 1]

    def background(b):
        return b if b is None or c["background"] != "expanded" else b[:1].expand(N, -1, -1, -1)

    # the binding
    fc, fa = form(color, alpha)
    img, trans = capi.composite_layers(fc, fa, index, background(bg))
    rgba = c["form"] == "rgba"
    if rgba:  # one gradient tensor for both
        want.update(want_color=want["want_color"] or want["want_alpha"], want_alpha=want["want_color"] or want["want_alpha"])
    gc, ga, gb = capi.composite_layers_backward(g_img, g_T, fc, fa, index, background(bg), **want)
    if rgba and gc is not None:
        gc, ga = gc[:, :, :-1], gc[:, :, -1]
    got = dict(img=img, T=trans, gc=gc, ga=ga, gb=gb)
    what = f"{describe(c)} capi"
    assert img.dtype == dtype and img.shape == want_img.shape and trans.shape == want_T.shape, what
    assert th.equal(img, want_img) and th.equal(trans, want_T), f"{what}: forward differs from the loop in the same dtype"
    for key, wanted in (("gc", want["want_color"]), ("ga", want["want_alpha"]), ("gb", want["want_background"] and bg is not None)):
        assert (got[key] is not None) == wanted, (what, key)
    for key, r in ref.items():
        if r is None or got[key] is None:
            continue
        assert got[key].shape == r.shape and got[key].dtype == dtype, (what, key)
        err = float((got[key].double().cpu() - r).abs().max())
        assert err <= bound[key], f"{what} {key}: {err:.3e} > {bound[key]:.3e}"
    if index is not None:
        masked = index == -1
        assert ga is None or not bool(ga[masked].any()), f"{what}: alpha gradient at a skipped layer"
        assert gc is None or not bool(gc[masked[:, :, None].expand_as(gc)].any()), f"{what}: colour gradient at a skipped layer"

    # the Python API under autograd: the same bits
    lc = color.clone().requires_grad_(want["want_color"])
    la = alpha.clone().requires_grad_(want["want_alpha"])
    lb = None if bg is None else bg.clone().requires_grad_("background" in needs)
    fc, fa = form(lc, la)
    pimg, pT = drtk_amd.composite_layers(fc, fa, index, background(lb))
    ((pimg * g_img).sum() + ((pT * g_T).sum() if g_T is not None else 0)).backward()
    assert th.equal(pimg, img) and th.equal(pT, trans), "the Python API and the C ABI binding differ in the forward"
    for leaf, mine, key in ((lc, gc, "gc"), (la, ga, "ga"), (lb, gb, "gb")):
        if mine is None:
            assert leaf is None or leaf.grad is None, key
        elif key == "gb" and c["background"] == "expanded":  # the one view's gradient: the sum over the views
            assert th.equal(leaf.grad[:1], mine.sum(0, keepdim=True)) and not bool(leaf.grad[1:].any()), key
        else:
            assert th.equal(leaf.grad, mine), f"the Python API and the C ABI binding differ in {key}"


# ---- shade ---------------------------------------------------------------------------------------------------------------------------
def shade_runs(c):
    """The two runs of a case, as descriptions of their own: the drawn setting of the four options, then every option the
    other way.  (Forty cases drawing one setting each left one of the sixteen out; drawn with its complement, a setting
    is missed only where neither of a pair is drawn.)  `needs`: those of the case's whose input the run has."""
    runs = []
    for flip in (False, True):
        run = dict(c, run=int(flip))
        if flip:
            run.update(index=not c["index"], specular=not c["specular"], background=not c["background"], gamma=None if c["gamma"] else 2.2)
        present = ["normal_img", "albedo", "light_dir", "ambient"] + (["pos_img", "specular", "shininess"] if run["specular"] else []) \
            + (["background"] if run["background"] else [])
        run["needs"] = tuple(k for k in c["needs"] if k in present)
        runs.append(run)
    return runs


def shade_inputs(c):
    """shade_oracle.build_case on a run's description (an `expanded_background`: every view has the background of view 0)"""
    inp, grad_out = SO.build_case(c, 2 * c["seed"] + c["run"], f"seed{c['seed']}")
    if c["layout"] == "expanded_background" and inp["background"] is not None:
        inp["background"] = inp["background"][:1].expand(c["N"], -1, -1, -1).contiguous()
    return inp, grad_out


def shade_laid_out(a, layout):
    """The arguments `a` of shade (device tensors) with the same values in `layout` (test_gpu_shade.LAYOUTS), every image
    made from the one in `a` by operations autograd goes through exactly, whatever lies around it NaN (-1 for the index)."""
    out = dict(a)
    images = [k for k in ("normal_img", "pos_img", "albedo", "background") if a[k] is not None and a[k].ndim == 4]

    def around(t, fill, shape, where):
        big = th.full(shape, fill, dtype=t.dtype, device=t.device)
        big[where] = t
        return big[where]

    if layout == "channel_slices":  # one [N, 3 + 3 + C, H, W] tensor, as interpolate returns it
        names = [k for k in images if k != "background"]
        attr, lo = th.cat([a[k] for k in names], 1), 0
        for k in names:
            out[k], lo = attr[:, lo:lo + a[k].shape[1]], lo + a[k].shape[1]
    elif layout == "expanded_background":
        if a["background"] is not None:
            out["background"] = a["background"][:1].expand(a["background"].shape[0], -1, -1, -1)
    elif layout != "contiguous":
        for k in images + (["index_img"] if a["index_img"] is not None and layout != "w_strided" else []):
            t = a[k]
            fill = -1 if k == "index_img" else float("nan")
            N, W = t.shape[0], t.shape[-1]
            if layout == "view_slice":
                out[k] = around(t, fill, (N + 2, *t.shape[1:]), slice(1, N + 1))
            elif layout == "w_strided":  # copied once
                out[k] = around(t, fill, (*t.shape[:-1], 2 * W), (..., slice(None, None, 2)))
            elif layout == "offset_one_element":  # element alignment only
                out[k] = around(t.flatten(), fill, (t.numel() + 1,), slice(1, None)).view(t.shape)
            else:  # rows W + 3 apart: a lane's pixels may span two rows
                out[k] = around(t, fill, (*t.shape[:-1], W + 3), (..., slice(2, W + 2)))
    return out


def run_shade(c):
    for run in shade_runs(c):
        run_shade_once(run)


def run_shade_once(c):
    import drtk_amd
    import test_gpu_shade as T
    from drtk_amd import capi

    dtype, needs = DTYPES[c["dtype"]], c["needs"]
    inp, grad_out = shade_inputs(c)
    # test_gpu_shade.check compares the gradients of pos_img and shininess where it finds that of specular: the binding gives
    # it too then (a gradient has the same bits whatever else was asked for)
    wanted = needs + (("specular",) if c["specular"] and "specular" not in needs and ("pos_img" in needs or "shininess" in needs) else ())
    keep = lambda r: {k: v.cpu() for k, v in r.items() if k == "out" or k.startswith("mag_") or k[5:] in wanted}  # noqa: E731
    r64 = keep(SO.reference(inp, grad_out, th.float64, DEV))
    r32 = keep(SO.reference(inp, grad_out, th.float32, DEV)) if dtype == th.float32 else None
    a, g = T.to_device(inp, dtype), grad_out.to(DEV, dtype)
    # the binding, the images in the case's layout
    alt = shade_laid_out(a, c["layout"])
    got = {"out": capi.shade_forward(**alt)}
    if needs:
        got.update({"grad_" + k: v for k, v in capi.shade_backward(g, **alt, want=wanted).items()})
    assert set(got) == {"out"} | {"grad_" + k for k in wanted}, sorted(got)
    T.check({k: v.cpu() for k, v in got.items()}, r64, r32, dtype, f"seed{c['seed']} capi")
    # the Python API under autograd: the same bits
    leaves = {k: (a[k].detach().clone().requires_grad_(True) if k in needs else a[k]) for k in a}
    out = drtk_amd.shade(**shade_laid_out(leaves, c["layout"]))
    assert th.equal(out, got["out"]), "the Python API and the C ABI binding differ in the output"
    if needs:
        out.backward(g)
    for k in needs:
        mine, theirs = leaves[k].grad, got["grad_" + k]
        if k == "background" and c["layout"] == "expanded_background":  # the one view's gradient: the sum over the views
            assert th.equal(mine[:1], theirs.sum(0, keepdim=True)) and not bool(mine[1:].any()), k
        else:
            assert th.equal(mine, theirs), f"the Python API and the C ABI binding differ in grad_{k}"


# ---- laplacian -------------------------------------------------------------------------------------------------------------------------
def laplacian_runs(c):
    """The runs of a case, as descriptions of their own: one, or the fans of a case drawn towards the chunk boundaries"""
    if c["mesh"] != "fan":
        return [dict(c, run=0)]
    return [dict(c, run=i, valence=valence) for i, valence in enumerate(c["valences"])]


def laplacian_mesh(c):
    """(v0 [V,3] float64, vi [F,3] int64) of a run, before the views are made"""
    if c["mesh"] == "soup":
        v0, vi = LO.soup_mesh(c["V"], c["F"], c["mesh_seed"])
    elif c["mesh"] == "grid":
        v0, vi = LO.grid_mesh(c["rows"], c["cols"], c["mesh_seed"])
    else:
        v0, vi = LO.fan_mesh(c["valence"])
    return LO.with_degenerates(v0, vi) if c["degenerate"] else (v0, vi)


def laplacian_inputs(c):
    """(v, x, grad, vi) of laplacian_oracle.build_case on a run, float64 holding float32 values, vi in the case's index type"""
    v, x, grad, vi = LO.build_case(*laplacian_mesh(c), c["N"], c["C"], c["per_view"], 4 * c["seed"] + c["run"], degenerate=c["degenerate"])
    v, x, grad = (t.float().double() for t in (v, x, grad))
    return v, x, grad, (vi.int() if c["vi_dtype"] == "int32" else vi)


def longest_row(vi, V):
    """the most (face, corner) entries a vertex of a view's topology has"""
    t = vi.long() if vi.ndim == 3 else vi.long()[None]
    return max(int(th.bincount(b.reshape(-1), minlength=V).max()) for b in t)


def chunk_launches(fn):
    """(fn(), how often the kernel of the long rows' chunks was launched meanwhile)"""
    from drtk_amd import capi

    th.cuda.synchronize()
    capi.kernel_timing_begin()
    try:
        res = fn()
        th.cuda.synchronize()
    finally:
        rep = capi.kernel_timing_report()
    return res, sum(n for k, (n, _) in rep.items() if k.split("<")[0] == "laplacian_chunk_kernel")


def run_laplacian(c):
    for run in laplacian_runs(c):
        run_laplacian_once(run)


def run_laplacian_once(c):
    import drtk_amd
    import test_gpu_laplacian as T
    from drtk_amd import capi

    dtype, needs, N = DTYPES[c["dtype"]], c["needs"], c["N"]
    v, x, grad, vi = laplacian_inputs(c)
    V = x.shape[1]
    long_rows = longest_row(vi, V) > capi.GEOMETRY_CHUNK
    name = f"seed{c['seed']} run {c['run']}"
    if c["weights"] == "cotangent":  # the full pipeline, every gradient, either route; then the gradients asked for alone
        ops, launches = chunk_launches(lambda: T.check_inputs(v, x, grad, vi, dtype, "ops", name, degenerate=c["degenerate"]))
        assert (launches > 0) == long_rows, f"{launches} launches of the chunk kernel, the longest row has {longest_row(vi, V)} entries"
        binding = T.check_inputs(v, x, grad, vi, dtype, "capi", name, degenerate=c["degenerate"])
        for k in T.KEYS:
            assert th.equal(ops[k], binding[k]), f"the Python API and the C ABI binding differ in {k}"
        vv = v.to(DEV, dtype).requires_grad_("v" in needs)
        xx = x.to(DEV, dtype).requires_grad_("x" in needs)
        w = drtk_amd.cotangent_weights(vv, vi.to(DEV))
        w = w.detach().requires_grad_(True) if ("weights" in needs and "v" not in needs) else w
        out = drtk_amd.mesh_laplacian(xx, vi.to(DEV), w)
        assert th.equal(out.detach().cpu(), ops["out"])
        if out.requires_grad:
            if w.requires_grad:
                w.retain_grad()
            out.backward(grad.to(DEV, dtype))
        for leaf, key, asked in ((xx, "grad_x", "x" in needs), (vv, "grad_v", "v" in needs), (w, "grad_w", "weights" in needs)):
            if asked:
                assert th.equal(leaf.grad.cpu(), ops[key]), f"{key} alone differs from {key} among all gradients"
            else:
                assert not leaf.is_leaf or leaf.grad is None, key
        return
    # weights in one of the layouts (test_every_layout_of_vi_and_weights_through_ops_and_capi on the case's mesh)
    layout = c["weights"]
    w_all = LO.cot_weights(v, vi)
    # (applied where the weights live: a copy to the device would make an expanded tensor contiguous)
    w_of = {"none": lambda w: None, "F3": lambda w: w[0], "1F3": lambda w: w[:1], "NF3": lambda w: w, "NF3_expand": lambda w: w[:1].expand(N, -1, -1)}[layout]

    def run(lap, dt, dev, asked):
        xx = x.to(dt).to(dev).clone().requires_grad_("x" in asked)
        ww = w_of(w_all.to(dt).to(dev))
        if ww is not None:
            ww = ww.detach().requires_grad_("weights" in asked)
            assert (ww.stride(0) == 0) == (layout == "NF3_expand" and N > 1)
        out = lap(xx, vi.to(dev), ww)
        res = {"out": out.detach().cpu()}
        if out.requires_grad:
            out.backward(grad.to(dt).to(dev))
            if xx.requires_grad:
                res["grad_x"] = xx.grad.cpu()
            if ww is not None and ww.requires_grad:
                res["grad_w"] = ww.grad.cpu()
        return res

    got, launches = chunk_launches(lambda: run(drtk_amd.mesh_laplacian, dtype, DEV, needs))
    assert (launches > 0) == long_rows, f"{launches} launches of the chunk kernel, the longest row has {longest_row(vi, V)} entries"
    r64 = run(LO.mesh_laplacian, th.float64, "cpu", needs)
    r32 = run(LO.mesh_laplacian, th.float32, "cpu", needs) if dtype == th.float32 else None
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    T.compare(got, r64, r32, dtype, name)
    # the C ABI on the same data: shared weights are [1,F,3] there, an expanded tensor is N rows like any other
    xd, gd = x.to(DEV, dtype), grad.to(DEV, dtype)
    vi32 = vi.to(DEV).int()
    inc = capi.vertex_incidence_numpy(vi.numpy(), V)
    wd = w_of(w_all.to(dtype).to(DEV))
    assert th.equal(capi.geometry_laplacian(xd, vi32, inc, wd).cpu(), got["out"]), "the Python API and the C ABI binding differ in out"
    if "grad_x" in got:
        assert th.equal(capi.geometry_laplacian(gd, vi32, inc, wd).cpu(), got["grad_x"]), "the Python API and the C ABI binding differ in grad_x"
    if "grad_w" in got:
        gw = capi.geometry_laplacian_grad_weights(gd, xd, vi32, shared_weights=layout in ("F3", "1F3"))
        assert th.equal(gw.cpu().reshape(got["grad_w"].shape), got["grad_w"]), "the Python API and the C ABI binding differ in grad_w"


# ---- msi ---------------------------------------------------------------------------------------------------------------------------------
def msi_inputs(c):
    """msi_oracle.build_case on the case's numbers, the fragile rays drawn again: (inputs, march arguments, an empty fragile
    mask, float64 result, float32 result)"""
    return MO.build_case(c["seed"], c["rays"], (c["L"], c["H"], c["W"]), c["sub_step_count"], *c["spheres"], c["stop_thresh"], c["sigma"],
                         c["radius"], redraw=True)


def run_msi(c):
    import test_gpu_msi as T

    dtype = DTYPES[c["dtype"]]
    case = msi_inputs(c)
    (o, d, tex, gout), args, fragile, r64, _ = case
    assert not bool(fragile.any())
    name = f"seed{c['seed']}"
    binding = T.check_against_the_oracle(case, dtype, "capi", name)
    python = T.check_against_the_oracle(case, dtype, "python", name)
    assert th.equal(binding[0], python[0]), "the Python API and the C ABI binding differ in out"
    if dtype != th.float64:  # the gradient is summed with atomics: the two routes are compared in float64, under its bound
        binding, python = (T.hip(o, d, tex.double(), gout.double(), args, api) for api in ("capi", "python"))
        assert th.equal(binding[0], python[0]), "the Python API and the C ABI binding differ in out (float64)"
    # the same terms in another atomic order: the float64 bound (test_texture_gradient_ignores_grad_out_column_3)
    assert float((binding[1] - python[1]).abs().max()) <= 1e-12 * float(r64.grad_texture.abs().max()), "the two routes' grad_texture"


RUN = {"filter2d": run_filter2d, "composite_layers": run_composite_layers, "shade": run_shade, "laplacian": run_laplacian, "msi": run_msi}


def run_case(c, check_guards=True):
    from drtk_amd import capi

    with contextlib.redirect_stdout(io.StringIO()):  # the figures the operators' checks print: a failure carries its own
        RUN[c["op"]](c)
    if check_guards:  # DRTK_CAPI_GUARD=g: nothing was written outside an output or a workspace (no-op otherwise)
        capi.check_guards()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--first", type=int, default=0)
    a = ap.parse_args()
    bad, t0 = 0, time.time()
    for seed in range(a.first, a.first + a.cases):
        c = make_case(seed)
        try:
            run_case(c)
        except AssertionError as e:
            bad += 1
            print(f"FAIL {describe(c)}: {str(e)[:600]}", flush=True)
        except Exception as e:  # an error of the runtime or the library: nothing more is started on the device
            print(f"ERROR {describe(c)}: {type(e).__name__}: {str(e)[:600]}\nstopped after seed {seed}", flush=True)
            sys.exit(2)
    print(f"{time.time() - t0:.1f} s")
    print(f"{a.cases - bad}/{a.cases} cases passed")
    sys.exit(1 if bad else 0)
