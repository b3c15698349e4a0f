"""CPU: tests/fuzz_added_ops.py, seeds 0 .. 239 (tests/test_gpu_fuzz_added_ops.py), from the drawn numbers and the inputs made
from them on the CPU: every case is one its operator's oracle admits, and the 240 seeds hold the crossings the fuzzer is
for -- otherwise the GPU test would pass by accident of the draw.  Also: the oracles' builders, split from their by-name
cases for the fuzzer, give the named cases the tensors they gave before, bit for bit."""
import collections
import functools
import os
import zlib

import torch as th
from conftest import ROOT

import filter2d_oracle as FO
import fuzz_added_ops as F
import laplacian_oracle as LO
import msi_oracle as MO
import shade_oracle as SO

PER_BLOCK, BLOCKS = 40, 6  # those of tests/test_gpu_fuzz_added_ops.py (asserted below)


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(F.make_case(seed) for seed in range(PER_BLOCK * BLOCKS))


def of(op):
    return [c for c in cases() if c["op"] == op]


def test_the_cases_are_seeded_plain_numbers_and_every_operator_is_drawn():
    import test_gpu_fuzz_added_ops as G

    assert (G.PER_BLOCK, G.BLOCKS) == (PER_BLOCK, BLOCKS) and len(cases()) == 240
    assert list(cases()) == [F.make_case(seed) for seed in range(240)]  # seeded

    def plain(v):
        return all(plain(e) for e in v) if isinstance(v, tuple) else v is None or isinstance(v, (bool, int, float, str))

    for c in cases():
        assert all(plain(v) for v in c.values()), c
        assert F.describe(c).startswith(f"seed={c['seed']} op={c['op']}")
    ops = collections.Counter(c["op"] for c in cases())
    assert set(ops) == set(F.OPS) and min(ops.values()) >= 35, ops


def test_filter2d_cases():
    generic, tuned = F.f2d_triples()
    assert len(generic) == 1429 and sum(u > 1 and d > 1 for u, d, _ in generic) == 1029  # the enumeration of the issue
    assert set(tuned) == {t for t in FO.FAMILIES if max(t[:2]) <= F.F2D_MAX_FACTOR and t[2] <= F.F2D_MAX_TAPS}
    drawn = of("filter2d")
    runs = [(c, run, i) for c in drawn for i, run in enumerate(F.f2d_runs(c))]
    for c in drawn:
        assert len(c["runs"]) == (1 if c["tuned"] else F.F2D_GENERIC_RUNS), c
        assert 1 <= c["N"] * c["C"] <= 7 and c["layout"] in ("contiguous", "column_slice"), c
    for c, run, i in runs:
        up, down, k = run["up"], run["down"], run["k"]
        assert 1 <= min(up, down) and max(up, down) <= 8 and 1 <= k <= 32 and c["tuned"] == ((up, down, k) in FO.FAMILIES), c
        for n, o in ((run["H"], run["OH"]), (run["W"], run["OW"])):
            # geometry defined either way, and the backward exists
            assert n % down == 0 and FO.geometry(n, k, up, down)[2] == o and FO.geometry(o, k, down, up, backward=True)[2] == n, c
            assert 1 <= o <= F.F2D_MAX_OUT + up, c
            if run["padding"] == "reflection":
                assert FO.reflect_ok(n, k, up, down) and FO.reflect_ok(o, k, down, up, backward=True), c
        x, f, gout = F.f2d_inputs(c, i)
        assert x.shape == (c["N"], c["C"], run["H"], run["W"]) and f.shape == (k,) and gout.shape == (c["N"], c["C"], run["OH"], run["OW"])
    triples = {(run["up"], run["down"], run["k"]) for c, run, _ in runs if not c["tuned"]}
    assert len(triples) >= 80 and sum(u > 1 and d > 1 for u, d, _ in triples) >= 40, (len(triples), sorted(triples))
    assert sum(c["tuned"] for c in drawn) >= 5
    for w in FO.TILE_WIDTHS:  # an output wider than a tile of each width, its last tile ragged: the forward's, the gradient call's
        assert any(run["OW"] > w and run["OW"] % w for c, run, _ in runs if not c["tuned"]), w
        assert any(run["W"] > w and run["W"] % w for c, run, _ in runs if not c["tuned"]), w
    assert {run["padding"] for _, run, _ in runs} == set(FO.BOTH) and {c["dtype"] for c in drawn} == {"f32", "f64", "f16"}
    assert {c["layout"] for c in drawn} == {"contiguous", "column_slice"}


def test_composite_layers_cases():
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "composite.hip")).read()
    assert "constexpr int kPix = (16 / int(sizeof(T))) / ((BACKWARD && K > 4) ? 2 : 1);" in src
    assert [F.composite_pix(d, K, b) for d in ("f32", "f64") for K in (4, 5) for b in (False, True)] == [4, 4, 4, 2, 2, 2, 2, 1]
    drawn = of("composite_layers")
    for c in drawn:
        assert 1 <= c["K"] <= 8 and 1 <= c["C"] <= 17 and 1 <= c["N"] <= 3 and c["H"] >= 1 and c["W"] >= 1 and c["H"] * c["W"] <= 2049, c
        assert c["needs"] and set(c["needs"]) <= {"color", "alpha"} | ({"background"} if c["background"] != "none" else set()), c
    assert {c["K"] for c in drawn} == set(range(1, 9))
    for key, values in (("index", F.COMPOSITE_INDEX), ("background", F.COMPOSITE_BACKGROUND), ("form", F.COMPOSITE_FORM),
                        ("grad_T", (False, True)), ("dtype", ("f32", "f64"))):
        assert {c[key] for c in drawn} == set(values), key
    sides = {c["H"] * c["W"] - 256 * F.composite_pix(c["dtype"], c["K"], c["near_pass"] == "backward") for c in drawn}
    assert {-1, 1} <= sides, sorted(sides)
    c = next(c for c in drawn if c["index"] == "holes" and c["background"] == "expanded" and c["H"] * c["W"] * c["K"] * c["N"] >= 100)
    color, alpha, bg, index, g_img, g_T = F.composite_inputs(c)
    assert bool((alpha == 0).any()) and bool((alpha == 1).any()) and bool((index == -1).any()) and th.equal(bg[0], bg[-1])
    assert float(g_img.abs().max()) <= 3 and float(g_T.abs().max()) <= 3


def test_shade_cases():
    import test_gpu_shade  # noqa: F401  (LAYOUTS; importing it needs no GPU)

    P, B, S, _ = SO.kernel_constants()
    cases_drawn = of("shade")
    drawn = [run for c in cases_drawn for run in F.shade_runs(c)]
    assert len(drawn) == 2 * len(cases_drawn) and all(set(run["needs"]) <= set(c["needs"]) for c in cases_drawn for run in F.shade_runs(c))
    assert set(F.SHADE_LAYOUTS) == {"contiguous"} | set(test_gpu_shade.LAYOUTS) and F.SHADE_FLOATS == test_gpu_shade.FLOATS
    for c in drawn:
        assert 1 <= c["C"] <= 4 and 1 <= c["N"] <= 4 and set(c["per_view"]) <= set(SO.PARAMS), c
        dt = F.DTYPES[c["dtype"]]
        assert c["many_rows"] == (c["H"] * c["W"] > S * B[dt] - B[dt]) and (not c["many_rows"] or c["H"] * c["W"] in (S * B[dt] - 1, (S + 1) * B[dt] + 1)), c
        inp, grad_out = F.shade_inputs(c)  # (raises where the margins are not reached)
        cat = SO.categories(inp)
        fg = cat["fg"]
        assert float(cat["ndl"].abs()[fg].min()) >= SO.MARGIN if bool(fg.any()) else True, c
        if c["specular"]:
            assert float(cat["hn"].abs().min()) >= SO.MARGIN and float(cat["hv"].min()) >= 0.1, c
        present = {k for k in F.SHADE_FLOATS if inp[k] is not None}
        assert set(c["needs"]) <= present, c
        assert (inp["index_img"] is not None) == c["index"] and (inp["background"] is not None) == c["background"]
        assert (inp["albedo"].ndim == 4) == c["albedo_img"] and inp["normal_img"].shape == (c["N"], 3, c["H"], c["W"])
    options = {(c["index"], c["specular"], c["background"], c["gamma"] is not None) for c in drawn}
    assert len(options) == 16, sorted(options)
    for p in SO.PARAMS:  # (specular and shininess: where there is a highlight)
        on = [c for c in drawn if c["specular"] or p not in ("specular", "shininess")]
        if p == "albedo":
            on = [c for c in on if not c["albedo_img"]]
        assert {p in c["per_view"] for c in on} == {False, True}, p
    assert {c["layout"] for c in drawn} == set(F.SHADE_LAYOUTS)
    assert {c["dtype"] for c in drawn if c["many_rows"]} == {"f32", "f64"}
    assert {c["albedo_img"] for c in drawn} == {False, True} and {c["C"] for c in drawn} == {1, 2, 3, 4}


def test_laplacian_cases():
    import test_gpu_laplacian  # noqa: F401  (W_LAYOUTS; importing it needs no GPU)

    drawn = [run for c in of("laplacian") for run in F.laplacian_runs(c)]
    assert all(c["valences"] in ((c["valences"][0],), tuple(F.LAPLACIAN_NEAR_VALENCE)) for c in of("laplacian") if c["mesh"] == "fan")
    assert F.LAPLACIAN_WEIGHTS == test_gpu_laplacian.W_LAYOUTS + ("cotangent",)
    for c in drawn:
        assert 1 <= c["N"] <= 4 and 1 <= c["C"] <= 9 and set(c["needs"]) <= {"x", "weights", "v"}, c
        v0, vi = F.laplacian_mesh(c)
        proper = vi[:-2] if c["degenerate"] else vi
        if c["mesh"] == "soup":
            assert 3 <= c["V"] <= 300 and 1 <= c["F"] <= 600 and proper.shape == (c["F"], 3), c
            angles = [a for f in proper.numpy() for a in F.corner_angles(v0.numpy()[f])]
            assert min(angles) > 0.4, c  # soup_mesh's bound
        elif c["mesh"] == "fan":
            assert 2 <= c["valence"] <= 700 and proper.shape == (c["valence"], 3), c
        else:
            assert 2 <= min(c["rows"], c["cols"]) and max(c["rows"], c["cols"]) <= 12, c
        v, x, grad, t = F.laplacian_inputs(c)
        V = v0.shape[0]
        assert v.shape == (c["N"], V, 3) and x.shape == grad.shape == (c["N"], V, c["C"])
        assert t.shape == ((c["N"],) if c["per_view"] else ()) + vi.shape and str(t.dtype) == "torch." + c["vi_dtype"]
        assert 0 <= int(t.min()) and int(t.max()) < V and th.equal(v.float().double(), v)
        if c["mesh"] == "fan":
            assert F.longest_row(t, V) == c["valence"] + int(c["degenerate"]), c  # (the duplicate-corner face holds vertex 0 too)
    fans = collections.Counter(c["valence"] for c in drawn if c["mesh"] == "fan")
    rows = collections.Counter(F.longest_row(F.laplacian_inputs(c)[3], c["valence"] + 1 + 4 * c["degenerate"]) for c in drawn if c["mesh"] == "fan")
    # (rows: a fan with the degenerate faces has one entry more in the row of vertex 0)
    assert all(fans[n] >= 1 and rows[n] >= 1 for n in (256, 257, 512, 513)), (sorted(fans.items()), sorted(rows.items()))
    for key, values in (("weights", F.LAPLACIAN_WEIGHTS), ("vi_dtype", ("int32", "int64")), ("per_view", (False, True)),
                        ("mesh", ("soup", "grid", "fan")), ("dtype", ("f32", "f64"))):
        assert {c[key] for c in drawn} == set(values), key
    assert any(c["degenerate"] and c["per_view"] for c in drawn)
    assert max(c["C"] for c in drawn) > 5
    for name in ("x", "weights", "v"):
        assert {name in c["needs"] for c in drawn} == {False, True}


def test_msi_cases():
    drawn = of("msi")
    some_stop, some_skip = collections.Counter(), 0
    for c in drawn:
        assert 1 <= c["rays"] <= 700 and 1 <= c["L"] <= 6 and 1 <= min(c["H"], c["W"]) and max(c["H"], c["W"]) <= 17, c
        assert 1 <= c["sub_step_count"] <= 3, c
        (o, d, tex, gout), args, fragile, r64, r32 = F.msi_inputs(c)  # (asserts that the redraws end)
        N = c["rays"]
        assert o.shape == d.shape == (N, 3) and tex.shape == (c["L"], 4, c["H"], c["W"]) and gout.shape == (N, 4)
        assert not bool(fragile.any()) and float(r64.margin.min()) >= MO.FRAGILE_MARGIN, c  # zero fragile rays
        assert bool(th.isfinite(r64.out).all()) and bool(th.isfinite(r64.grad_texture).all())
        if N / 10 <= int(r64.stopped.sum()) <= N - N / 10:
            some_stop[c["stop_thresh"]] += 1
        some_skip += int(r64.skipped.sum()) >= N / 10
    assert sum(c["H"] == 1 for c in drawn) >= 3 and sum(c["W"] == 1 for c in drawn) >= 3
    assert {c["L"] for c in drawn} == set(range(1, 7)) and {c["stop_thresh"] for c in drawn} == set(F.MSI_STOP)
    assert {c["dtype"] for c in drawn} == {"f32", "f64"} and {c["sub_step_count"] for c in drawn} == {1, 2, 3}
    assert sum(some_stop.values()) >= 5, some_stop
    assert some_skip >= 5, some_skip
    assert {c["rays"] for c in drawn} & set(F.MSI_NEAR_RAYS) >= {255, 257} or len({c["rays"] for c in drawn} & set(F.MSI_NEAR_RAYS)) >= 4


# ---- the builders give the named cases what `case(name)` gave before ---------------------------------------------------------------
def shade_case_before(name):
    """shade_oracle.case as it was before build_case was split from it"""
    c = SO.CASES[name]
    N, C, H, W = c["N"], c["C"], c["H"], c["W"]
    gen = th.Generator().manual_seed(zlib.crc32(name.encode()))
    f32 = lambda t: t.float().double()  # noqa: E731
    rand = lambda *s: th.rand(*s, generator=gen, dtype=th.float64)  # noqa: E731

    def directions(*lead):
        g = th.randn(*lead, 3, generator=gen, dtype=th.float64)
        return g / g.norm(dim=-1, keepdim=True).clamp(min=1e-3)

    def param(key, value):
        return f32(value if key in c["per_view"] else value[0])

    def vectors(lo, hi):  # [N, 3, H, W], norms in [lo, hi]
        return f32((directions(N, H, W) * (lo + (hi - lo) * rand(N, H, W, 1))).permute(0, 3, 1, 2).contiguous())

    inp = {"normal_img": vectors(0.2, 2.0), "light_dir": param("light_dir", directions(N) * (0.5 + 1.5 * rand(N, 1)))}
    inp["albedo"] = f32(0.05 + 0.95 * rand(N, C, H, W)) if c["albedo_img"] else param("albedo", 0.05 + 0.95 * rand(N, C))
    inp["ambient"] = param("ambient", 0.05 + 0.45 * rand(N, C))
    inp["index_img"] = None
    if c["index"]:
        idx = th.randint(0, 1000, (N, H, W), generator=gen, dtype=th.int32)
        inp["index_img"] = th.where(rand(N, H, W) < 0.35, th.full_like(idx, -1), idx)
    inp["pos_img"] = inp["specular"] = inp["shininess"] = None
    if c["specular"]:
        inp["pos_img"] = vectors(0.5, 3.0)
        inp["specular"] = param("specular", 0.05 + 0.95 * rand(N, C))
        inp["shininess"] = param("shininess", 1.5 + 28.5 * rand(N, 1))
    inp["background"] = f32(0.05 + 0.95 * rand(N, C, H, W)) if c["background"] else None
    inp["gamma"] = c["gamma"]
    for _ in range(200):
        cat = SO.categories(inp)
        bad = cat["ndl"].abs() < 2 * SO.MARGIN
        if c["specular"]:
            bad |= (cat["hn"].abs() < 2 * SO.MARGIN) | (cat["hv"] < 0.2)
        if not bool(bad.any()):
            break
        m = bad[:, None]
        inp["normal_img"] = th.where(m, vectors(0.2, 2.0), inp["normal_img"])
        if c["specular"]:
            inp["pos_img"] = th.where(m, vectors(0.5, 3.0), inp["pos_img"])
    else:
        raise AssertionError(f"{name}: no draw with the margins")
    t = th.arange(N * C * H * W, dtype=th.float64).view(N, C, H, W)
    grad_out = f32(th.cos(t * 0.37) * (0.5 + rand(N, C, H, W)))
    return inp, grad_out


def laplacian_case_before(name):
    """laplacian_oracle.case as it was before build_case was split from it"""
    mesh, n, c, per_view = LO.CASES[name]
    keep_last = 0
    if mesh == "one":
        v0, vi = th.tensor([[0.1, 0.0, 0.2], [1.0, 0.2, 0.0], [0.3, 0.9, 0.1]], dtype=th.float64), th.tensor([[0, 1, 2]])
    elif mesh == "soup":
        v0, vi = LO.soup_mesh(257, 257, 3)
    elif mesh == "degenerate":
        v0, vi = LO.with_degenerates(*LO.grid_mesh(5, 7, 4))
        keep_last = 2
    else:
        v0, vi = LO.fan_mesh(int(mesh[3:]))
    g = th.Generator().manual_seed(sum(map(ord, name)))
    v = v0[None] * (1 + 0.1 * th.arange(n, dtype=th.float64))[:, None, None] + 0.02 * th.randn(n, *v0.shape, dtype=th.float64, generator=g)
    if mesh == "degenerate":
        v[:, -3:] = v0[-3:]  # the collinear face keeps its integer coordinates
    x = th.randn(n, v0.shape[0], c, dtype=th.float64, generator=g)
    grad = th.randn(n, v0.shape[0], c, dtype=th.float64, generator=g)
    if per_view:
        k = vi.shape[0] - keep_last
        vi = th.stack([th.cat([vi[:k].roll(i, 0).roll(i, 1), vi[k:]]) for i in range(n)])
    return v, x, grad, vi


def msi_make_case_before(seed, N, L, H, W, sigma_range, origin_radius, dtype=th.float32):
    """msi_oracle.make_case as it was before draw_rays was split from it"""
    g = th.Generator().manual_seed(seed)
    rnd = lambda *shape: th.rand(*shape, generator=g, dtype=th.float64)  # noqa: E731
    tex = th.empty(L, 4, H, W, dtype=th.float64)
    tex[:, :3] = th.where(rnd(L, 3, H, W) < 0.3, rnd(L, 3, H, W) * -0.2, rnd(L, 3, H, W) * 1.2)
    tex[:, 3] = rnd(L, H, W) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
    unit = lambda x: x / x.norm(dim=1, keepdim=True)  # noqa: E731
    o = unit(th.randn(N, 3, generator=g, dtype=th.float64)) * (rnd(N, 1) ** (1 / 3) * origin_radius)
    d = unit(th.randn(N, 3, generator=g, dtype=th.float64)) * (rnd(N, 1) * 2.9 + 0.1)
    gout = rnd(N, 4) * 2 - 1
    return o.float(), d.float(), tex.float().to(dtype), gout.float().to(dtype)


def msi_case_before(name):
    """msi_oracle.case as it was before build_case was split from it"""
    seed, N, (L, H, W), sub, mn, mx, stop, sig, rad = MO.CASES[name]
    o, d, tex, gout = msi_make_case_before(seed, N, L, H, W, sig, rad)
    args = (sub, mn, mx, stop)
    fragile = MO.march(o, d, tex.double(), *args).margin < MO.FRAGILE_MARGIN
    gout = gout.clone()
    gout[fragile] = 0
    r64 = MO.march(o, d, tex.double(), *args, grad_out=gout.double())
    r32 = MO.march(o, d, tex, *args, grad_out=gout)
    return ((o, d, tex, gout), args, fragile, r64, r32)


def same(a, b):
    return (a is None and b is None) or (not th.is_tensor(a) and a == b) or (th.is_tensor(a) and a.dtype == b.dtype and a.shape == b.shape and th.equal(a, b))


def test_the_by_name_cases_are_what_they_were_bit_for_bit():
    for name in ("opt_i1s1b1g1", "n2_c3", "plane1"):
        (inp, grad_out), (inp0, grad_out0) = SO.case(name), shade_case_before(name)
        assert list(inp) == list(inp0) and all(same(inp[k], inp0[k]) for k in inp) and same(grad_out, grad_out0), name
    for name in ("degenerate_per_view", "fan300_shared", "soup257_c5_n3", "one_face"):
        assert all(same(a, b) for a, b in zip(LO.case(name), laplacian_case_before(name))), name
    for name in ("one_layer", "outside_skip"):
        (inputs, args, fragile, r64, r32), (inputs0, args0, fragile0, r64_0, r32_0) = MO.case(name), msi_case_before(name)
        assert all(same(a, b) for a, b in zip(inputs, inputs0)) and args == args0 and same(fragile, fragile0), name
        for r, r0 in ((r64, r64_0), (r32, r32_0)):
            assert all(same(getattr(r, k), getattr(r0, k)) for k in ("out", "grad_texture", "magnitudes", "margin", "stopped")), name
    # the redraw of the fuzzer leaves the case's first draw where no ray is fragile, and the texture in any case
    seed, N, shape, sub, mn, mx, stop, sig, rad = MO.CASES["one_layer"]
    (o, d, tex, gout), _, fragile, _, _ = MO.build_case(seed, 200, shape, sub, mn, mx, stop, sig, rad, redraw=True)
    o0, d0, tex0, gout0 = msi_make_case_before(seed, 200, *shape, sig, rad)
    first = MO.march(o0, d0, tex0.double(), sub, mn, mx, stop).margin >= MO.FRAGILE_MARGIN
    assert same(tex, tex0) and same(gout, gout0) and th.equal(o[first], o0[first]) and th.equal(d[first], d0[first]) and not bool(fragile.any())
