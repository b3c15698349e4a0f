"""GPU: the mesh geometry of drtk.utils on the HIP route (csrc/geometry.hip through the drtk_amd_ext operators and the
C ABI) -- against the reference's outputs and VJPs (tests/golden/refpy_geometry_*.npz: three meshes with vti = vi and
`seam`, whose UV atlas has a topology of its own, T = V + 6 UV vertices), through the operators and through the C ABI
composed by _run_all_capi, against the float64 PyTorch formulation at full size, bitwise reproducibility, the incidence
cache, graph capture, a shading step end to end, and the shapes that stress the vertex pass (a 65 536-valence fan,
70 000 views, no faces).  The helpers that take tensors -- _run_all_capi, _near_degenerate, _split, check_float64,
check_float32 -- and their bounds are also those of the seeded random cases of tests/fuzz_geometry.py
(tests/test_gpu_fuzz_geometry.py), which states no bound of its own."""
import os

import numpy as np
import pytest
import torch as th
from conftest import ROOT

from f64_distance import assert_within_f64_distance

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("band", "poles", "multi", "seam")


def _load(tag):
    """the three meshes of refpy_geometry_<tag>.npz and the seam mesh of refpy_geometry_seam_<tag>.npz, in one dict"""
    d = {}
    for stem in (f"refpy_geometry_{tag}", f"refpy_geometry_seam_{tag}"):
        z = np.load(os.path.join(ROOT, "tests", "golden", stem + ".npz"))
        d.update({k: th.from_numpy(z[k]) for k in z.files})
    return d


def _run_all(d, name, dtype, idx_dtype, dev):
    """Every function on the fixture's inputs, forward and VJP, through drtk.utils: {name: tensor on the CPU}"""
    from drtk.utils.geometry import face_attribute_to_vert, face_dpdt, face_info, vert_binormals, vert_normals

    p = lambda k: d[f"{name}_{k}"].to(dev).clone()  # noqa: E731
    vi = p("vi").to(idx_dtype)
    res = {}
    v = p("v").to(dtype).requires_grad_(True)
    fi = face_info(v, vi)
    th.autograd.backward([fi[k] for k in ("normals", "areas", "edges")],
                         [p(f"g_face_info_{k}").to(dtype) for k in ("normals", "areas", "edges")])
    res.update({f"face_info_{k}": fi[k] for k in ("normals", "areas", "edges")})
    res["face_info_grad_v"] = v.grad
    v = p("v").to(dtype).requires_grad_(True)
    vn = vert_normals(v, vi)
    vn.backward(p("g_vert_normals").to(dtype))
    res["vert_normals"], res["vert_normals_grad_v"] = vn, v.grad
    fn = p("fnorms").to(dtype).requires_grad_(True)
    vnf = vert_normals(p("v").to(dtype), vi, fn)
    vnf.backward(p("g_vert_normals").to(dtype))
    res["vert_normals_fnorms"], res["vert_normals_grad_fnorms"] = vnf, fn.grad
    attr = p("attr").to(dtype).requires_grad_(True)
    fv = face_attribute_to_vert(p("v").to(dtype), vi, attr)
    fv.backward(p("g_face_attribute_to_vert").to(dtype))
    res["face_attribute_to_vert"], res["face_attribute_to_vert_grad_attr"] = fv, attr.grad
    if f"{name}_vt" in d:
        vti = p("vti").to(idx_dtype)
        v, vt = p("v").to(dtype).requires_grad_(True), p("vt").to(dtype).requires_grad_(True)
        dpdt, v012 = face_dpdt(v, vt, vi, vti)
        th.autograd.backward([dpdt, v012], [p("g_face_dpdt").to(dtype), p("g_face_dpdt_v012").to(dtype)])
        res["face_dpdt"], res["face_dpdt_v012"], res["face_dpdt_grad_v"], res["face_dpdt_grad_vt"] = dpdt, v012, v.grad, vt.grad
        v, vt = p("v").to(dtype).requires_grad_(True), p("vt").to(dtype).requires_grad_(True)
        vb = vert_binormals(v, vt, vi, vti)
        vb.backward(p("g_vert_binormals").to(dtype))
        res["vert_binormals"], res["vert_binormals_grad_v"], res["vert_binormals_grad_vt"] = vb, v.grad, vt.grad
    return {k: t.detach().cpu() for k, t in res.items()}


# outputs that go through the face normal c / max(|c|, 1e-8): a face with |c| < 1e-8 multiplies the rounding noise of c by
# 1e8 (two nearly coinciding corners make c a difference of nearly equal products), so those entries are compared apart
_FACE_C = ("face_info_normals",)
_VERT_C = ("face_info_grad_v", "vert_normals", "vert_normals_grad_v")


def _near_degenerate(areas, vi, V):
    """(faces [N,F] with |c| < 1e-8 in the reference's areas [N,F,1], vertices [N,V] that touch one through vi)"""
    faces = (2 * areas[..., 0]) < 1e-8
    N = areas.shape[0]
    vi = vi.long()
    vi = vi.expand(N, -1, -1) if vi.dim() == 3 else vi[None].expand(N, -1, -1)
    verts = th.zeros(N, V, dtype=th.bool)
    for n in range(N):
        verts[n, vi[n][faces[n]].reshape(-1)] = True
    return faces, verts


def _split(k, t, faces, verts):
    """(entries compared with the bound, entries compared apart)"""
    if k in _FACE_C:
        return t[~faces], t[faces]
    if k in _VERT_C:
        return t[~verts], t[verts]
    return t, t[:0]


@pytest.mark.parametrize("idx_dtype", [th.int32, th.int64])
@pytest.mark.parametrize("name", NAMES)
def test_hip_route_matches_the_reference_fixtures(name, idx_dtype):
    """float64 against the reference's float64 to 1e-9 of the output's scale, float32 within the f64-distance bound;
    entries behind a face with |c| < 1e-8: the exactly degenerate ones element by element, the others (rounding noise
    times 1e8 in the reference as well) only for being finite."""
    import drtk_amd.geometry as G

    d32, d64 = _load("f32"), _load("f64")
    G.geometry_cache_clear()
    got64 = _run_all(d64, name, th.float64, idx_dtype, DEV)
    got32 = _run_all(d32, name, th.float32, idx_dtype, DEV)
    _check_against_the_fixtures(name, got64, got32, d32, d64)


def _fixture_case(d, name):
    """The arrays of mesh `name` without their prefix: a case as _run_all_capi and check_float64 / check_float32 take it"""
    return {k[len(name) + 1:]: t for k, t in d.items() if k.startswith(name + "_")}


def _run_all_capi(case, dtype, dev):
    """What _run_all computes, composed from the four geometry entry points of the C ABI (int32 topology, the numpy
    incidence) the way csrc/torch_ops/geometry.cpp composes them: {name: tensor on the CPU}, the same keys.  `case`: the
    inputs and upstream gradients under a fixture's names without the prefix (_fixture_case; tests/fuzz_geometry.py makes
    its own) -- of g_face_info_{normals,areas,edges} those that are there, the outputs of face_info those that
    `face_info_outputs` lists (default all three), face_dpdt and vert_binormals on `vi_shared` [F,3] where vi is one list
    per view (default vi)."""
    from drtk_amd import capi

    p = lambda k: case[k].to(dev).clone()  # noqa: E731
    g = lambda k: p(k).to(dtype) if k in case else None  # noqa: E731
    vi = p("vi").to(th.int32)
    v = g("v")
    V = v.shape[1]
    inc = capi.vertex_incidence_numpy(vi.cpu().numpy(), V)
    to_v = lambda rows: capi.geometry_vertex_gather(rows, inc, V, per_corner=True)[0]  # noqa: E731
    res = {}
    kinds = tuple(case.get("face_info_outputs", ("normals", "areas", "edges")))
    f = capi.geometry_face_forward(v, vi, outputs=kinds)
    res.update({f"face_info_{k}": f[k] for k in kinds})
    pos, uv = capi.geometry_face_backward(v, vi, grad_normals=g("g_face_info_normals"), grad_areas=g("g_face_info_areas"),
                                          grad_edges=g("g_face_info_edges"))
    assert uv is None
    res["face_info_grad_v"] = to_v(pos)
    normals = f["normals"] if "normals" in kinds else capi.geometry_face_forward(v, vi, outputs=("normals",))["normals"]
    vn, sums = capi.geometry_vertex_gather(normals, inc, V, normalize=True)
    pos, _ = capi.geometry_face_backward(v, vi, grad_vert=g("g_vert_normals"), vert_sums=sums)
    res["vert_normals"], res["vert_normals_grad_v"] = vn, to_v(pos)
    vnf, sums = capi.geometry_vertex_gather(g("fnorms"), inc, V, normalize=True)
    res["vert_normals_fnorms"] = vnf
    res["vert_normals_grad_fnorms"] = capi.geometry_face_gather(g("g_vert_normals"), vi, vert_sums=sums)
    fv, none = capi.geometry_vertex_gather(g("attr"), inc, V)
    assert none is None
    res["face_attribute_to_vert"] = fv
    res["face_attribute_to_vert_grad_attr"] = capi.geometry_face_gather(g("g_face_attribute_to_vert"), vi)
    if "vt" in case:
        if "vi_shared" in case:
            vi = p("vi_shared").to(th.int32)
            inc = capi.vertex_incidence_numpy(vi.cpu().numpy(), V)
        vti, vt = p("vti").to(th.int32), g("vt")
        T = vt.shape[1]
        tinc = capi.vertex_incidence_numpy(vti.cpu().numpy(), T)
        to_vt = lambda rows: capi.geometry_vertex_gather(rows, tinc, T, per_corner=True)[0]  # noqa: E731
        f2 = capi.geometry_face_forward(v, vi, vt, vti, outputs=("dpdt", "v012", "dpdt_u"))
        pos, uv = capi.geometry_face_backward(v, vi, vt, vti, grad_dpdt=g("g_face_dpdt"), grad_v012=g("g_face_dpdt_v012"))
        res["face_dpdt"], res["face_dpdt_v012"], res["face_dpdt_grad_v"], res["face_dpdt_grad_vt"] = f2["dpdt"], f2["v012"], to_v(pos), to_vt(uv)
        vb, sums = capi.geometry_vertex_gather(f2["dpdt_u"], inc, V, normalize=True)
        pos, uv = capi.geometry_face_backward(v, vi, vt, vti, grad_vert=g("g_vert_binormals"), vert_sums=sums)
        res["vert_binormals"], res["vert_binormals_grad_v"], res["vert_binormals_grad_vt"] = vb, to_v(pos), to_vt(uv)
    return {k: t.detach().cpu() for k, t in res.items()}


def check_float64(k, got, ref, faces, verts, what):
    """Output or gradient `k` of a float64 run against the float64 reference: within 1e-9 of the output's scale; entries
    behind a face with |c| < 1e-8 (`faces`, `verts` of _near_degenerate): finite, and a face normal that is exactly 0 in
    the reference exactly 0."""
    (a, a_deg), (b, b_deg) = _split(k, got, faces, verts), _split(k, ref, faces, verts)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= 1e-9 * max(1.0, float(b.abs().max()) if b.numel() else 0.0), (what, k, err)
    assert bool(th.isfinite(a_deg).all()), (what, k)
    exact = b_deg == 0
    assert th.equal(a_deg[exact], b_deg[exact]) or k not in _FACE_C, (what, k)


def check_float32(k, got, ref32, ref64, faces, verts, what):
    """The same of a float32 run: the entries not behind such a face within the f64-distance bound (its defaults), the others
    finite"""
    ok = [_split(k, x, faces, verts)[0] for x in (got, ref32, ref64)]
    assert_within_f64_distance(*ok, f"{what} {k}")
    assert bool(th.isfinite(_split(k, got, faces, verts)[1]).all()), (what, k)


def _check_against_the_fixtures(name, got64, got32, d32, d64):
    """The bounds of test_hip_route_matches_the_reference_fixtures (its docstring), on what _run_all or _run_all_capi gave."""
    faces, verts = _near_degenerate(d64[f"{name}_face_info_areas"], d64[f"{name}_vi"], d64[f"{name}_v"].shape[1])
    for k, t in got64.items():
        check_float64(k, t, d64[f"{name}_{k}"], faces, verts, name)
    assert got32.keys() == got64.keys()
    for k, t in got32.items():
        check_float32(k, t, d32[f"{name}_{k}"], d64[f"{name}_{k}"], faces, verts, name)
    if name == "multi":
        # its degenerate faces list a vertex twice: c is exactly 0 and the 1e8 branch is taken exactly; a vertex listed
        # twice receives two 1e8-scaled corner rows that cancel, so it is held to double rounding at that scale
        for k in _VERT_C:
            a, b = got64[k][verts], d64[f"{name}_{k}"][verts]
            assert float((a - b).abs().max()) <= 1e-15 * 1e8 * 10 * max(1.0, float(b.abs().max())), k


@pytest.mark.parametrize("name", NAMES)
def test_c_abi_composition_matches_the_reference_fixtures(name):
    """The same fixtures through the four entry points of the C ABI, composed by _run_all_capi (which tests/fuzz_geometry.py
    and tests/guarded_added_ops.py use): the bounds of the operators' test above."""
    d32, d64 = _load("f32"), _load("f64")
    got64 = _run_all_capi(_fixture_case(d64, name), th.float64, DEV)
    got32 = _run_all_capi(_fixture_case(d32, name), th.float32, DEV)
    assert set(got64) == {k[len(name) + 1:] for k in d64 if k.startswith(name + "_") and (k[len(name) + 1:].split("_")[0] in ("face", "vert"))}
    _check_against_the_fixtures(name, got64, got32, d32, d64)


def _sphere_views(n, size, dtype=th.float32, dev=DEV):
    """configs[2]'s mesh (pole triangles included), one scaled and shifted copy per view (pole corners stay equal)"""
    from drtk_amd import synthetic as S

    v0, vi = S.uv_sphere(*S.MESH_SIZES[size], dtype=th.float64)
    k = th.arange(n, dtype=th.float64)
    # the shift makes the south pole's corners (x, z ~ 1e-16) round to the same float32 value too
    v = v0[None] * (1 + 0.1 * k)[:, None, None] + th.stack([0.1 * k + 0.1, -0.05 * k, 0.02 * k + 0.1], -1)[:, None, :]
    return v.to(dtype).to(dev), vi.to(dev)


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
@pytest.mark.parametrize("layout", ["F3", "1F3", "NF3_expand", "NF3"])
@pytest.mark.parametrize("idx_dtype", [th.int32, th.int64])
def test_every_layout_and_index_dtype_through_ops_and_capi(dtype, layout, idx_dtype):
    """All vi layouts and index dtypes give the bitwise-same results; the C ABI called through ctypes gives the bitwise-
    same results as the operators (the same kernels)."""
    from drtk_amd import capi
    import drtk_amd.geometry as G

    N = 3
    v, vi = _sphere_views(N, "10k", dtype)
    vt = (v[:, :, :2] * 0.5 + 0.5).contiguous()
    base = vi
    vi_l = {"F3": vi, "1F3": vi[None], "NF3_expand": vi[None].expand(N, -1, -1), "NF3": vi[None].repeat(N, 1, 1)}[layout]
    vi_l = vi_l.to(idx_dtype)
    ops = G._ops()
    g = th.randn(N, v.shape[1], 3, dtype=dtype, device=DEV)

    def fwd_bwd(vi_x):
        x = v.clone().requires_grad_(True)
        out = ops.vert_normals(x, vi_x, None)
        out.backward(g)
        n, a, e = ops.face_info(v, vi_x, True, True, True)
        attr = th.randn(N, vi.shape[0], 4, dtype=dtype, device=DEV, generator=th.Generator(DEV).manual_seed(1))
        fv = ops.face_attribute_to_vert(v, vi_x, attr)
        return out.detach(), x.grad, n, a, e, fv

    want = fwd_bwd(base)
    got = fwd_bwd(vi_l)
    for a, b in zip(want, got):
        assert th.equal(a, b)
    # dpdt / binormals take [F,3] topology in either index dtype
    x, y = v.clone().requires_grad_(True), vt.clone().requires_grad_(True)
    vb = G.vert_binormals(x, y, vi.to(idx_dtype), vi.to(idx_dtype))
    vb.backward(g)
    dp, v012 = G.face_dpdt(v, vt, vi.to(idx_dtype), vi.to(idx_dtype))
    # the same through the C ABI
    inc = capi.vertex_incidence_numpy(vi_l.cpu().numpy() if layout != "NF3_expand" else vi.cpu().numpy(), v.shape[1])
    vi32 = (vi_l if layout != "NF3_expand" else vi).to(th.int32)
    f = capi.geometry_face_forward(v, vi32, outputs=("normals", "areas", "edges"))
    assert th.equal(f["normals"], want[2]) and th.equal(f["areas"], want[3]) and th.equal(f["edges"], want[4])
    vn, sums = capi.geometry_vertex_gather(f["normals"], inc, v.shape[1], normalize=True)
    assert th.equal(vn, want[0])
    pos, _ = capi.geometry_face_backward(v, vi32, grad_vert=g, vert_sums=sums)
    gv, _ = capi.geometry_vertex_gather(pos, inc, v.shape[1], per_corner=True)
    assert th.equal(gv, want[1])
    f2 = capi.geometry_face_forward(v, vi.to(th.int32), vt, vi.to(th.int32), outputs=("dpdt", "v012", "dpdt_u"))
    # (the pole faces' UV matrices are singular here: non-finite dpdt, compared as bits too)
    for a, b in ((f2["dpdt"], dp), (f2["v012"], v012), (f2["dpdt_u"], dp[:, :, 0])):
        th.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert capi.check_guards() >= 0


def _accumulated_grad_magnitude(v, vi, g):
    """[N,V,3]: what vert_normals' backward accumulates into each vertex, in magnitude (float64 formulation): the sum of
    the absolute per-(face, corner) gradient rows, plus, for a face with c = 0, the rounding of the upstream gradient
    it sees amplified by its 1e8 Jacobian -- 1e8 * (|p1 - p0| + |p0 - p2|) * sum over its corners of |g| / |vertex sum|
    (F.normalize's backward removes the normal component of g by cancellation)"""
    import drtk_amd.geometry as G

    v64, vi_c, g64 = v.detach().cpu().double(), vi.cpu(), g.cpu().double()
    pc = G._corners(v64, vi_c).requires_grad_(True)  # [N,F,3,3]
    p0, p1, p2 = pc.unbind(2)
    c = th.linalg.cross(p0 - p2, p1 - p0, dim=-1)
    fn = c / th.linalg.vector_norm(c, dim=-1, keepdim=True).clamp(min=1e-8)
    sums = G._face_attribute_to_vert_torch(v64, vi_c, fn)
    th.nn.functional.normalize(sums, dim=-1).backward(g64)
    N, F = pc.shape[:2]
    idx = G._topology(vi_c, N).reshape(N, -1, 1).expand(-1, -1, 3)
    rows = pc.grad.abs()
    with th.no_grad():
        ratio = (g64.norm(dim=-1) / sums.norm(dim=-1).clamp(min=1e-12))[..., None]  # [N,V,1]
        seen = G._corners(ratio, vi_c).sum(2)  # [N,F,1]
        amp = 1e8 * ((p1 - p0).norm(dim=-1, keepdim=True) + (p0 - p2).norm(dim=-1, keepdim=True)) * seen
        amp = amp * (c.norm(dim=-1, keepdim=True) < 1e-8)
        rows = rows + amp[:, :, None, :].expand(-1, -1, 3, 3)
    return th.zeros_like(v64).scatter_add(1, idx, rows.reshape(N, 3 * F, 3))


def test_full_size_vert_normals_parity_and_the_pole_branches():
    """configs[2]'s mesh, 8 views, float32 HIP against the float64 (and float32) formulation: the f64-distance bound on
    vertices that touch no degenerate face, the pole vertices (1e8-scaled gradients) element by element."""
    import drtk_amd.geometry as G

    N = 8
    v, vi = _sphere_views(N, "100k")
    g = th.randn(N, v.shape[1], 3, device=DEV, generator=th.Generator(DEV).manual_seed(3))
    x = v.clone().requires_grad_(True)
    out = G.vert_normals(x, vi)
    out.backward(g)
    res = {}
    for dt in (th.float32, th.float64):
        xc = v.detach().cpu().to(dt).requires_grad_(True)
        o = G.vert_normals(xc, vi.cpu())
        o.backward(g.cpu().to(dt))
        res[dt] = (o.detach(), xc.grad)
    area = G.face_info(v.double().cpu(), vi.cpu(), ["areas"])[..., 0]
    assert th.equal(area == 0, 2 * area < 1e-8)  # exactly degenerate, no near-degenerate face
    degenerate = vi.cpu()[(area == 0).any(0)].long().unique()
    assert degenerate.numel() > 0
    keep = th.ones(v.shape[1], dtype=th.bool)
    keep[degenerate] = False
    for i, what in ((0, "vert_normals"), (1, "grad_v")):
        got = (out.detach() if i == 0 else x.grad).cpu()
        assert_within_f64_distance(got[:, keep], res[th.float32][i][:, keep], res[th.float64][i][:, keep], what)
        # element by element, against what was accumulated into the element (the 1e8-scaled corner rows of the pole
        # faces partly cancel at a pole vertex): |got - f64| <= 64 float32 ulps of that magnitude + 1e-5 of the value
        ref = res[th.float64][i][:, degenerate]
        acc = (_accumulated_grad_magnitude(v, vi, g) if i else th.ones_like(res[th.float64][0]))[:, degenerate]
        err = (got[:, degenerate].double() - ref).abs()
        bound = 64 * 2.0 ** -24 * acc + 1e-5 * ref.abs()
        assert bool((err <= bound).all()), (what, float((err / bound).max()))
    assert float(x.grad.abs().max()) > 1e6  # the pole branch is there


def _fwd_bwd_all(v, vt, vi):
    import drtk_amd.geometry as G

    x, y = v.clone().requires_grad_(True), vt.clone().requires_grad_(True)
    vn = G.vert_normals(x, vi)
    vb = G.vert_binormals(x, y, vi, vi)
    fi = G.face_info(x, vi)
    loss = (vn * 1.5).sum() + (vb * vb.roll(1, 1)).sum() + fi["areas"].sum() + (fi["normals"] ** 2).sum() + fi["edges"].sum()
    loss.backward()
    return [vn.detach(), vb.detach(), fi["normals"].detach(), x.grad, y.grad]


def test_bitwise_reproducible_from_cold_and_warm_cache():
    import drtk_amd.geometry as G

    v, vi = _sphere_views(4, "10k")
    vt = th.rand(v.shape[0], v.shape[1], 2, device=DEV, generator=th.Generator(DEV).manual_seed(4))  # no singular UV
    G.geometry_cache_clear()
    a = _fwd_bwd_all(v, vt, vi)
    G.geometry_cache_clear()
    b = _fwd_bwd_all(v, vt, vi)
    c = _fwd_bwd_all(v, vt, vi)
    for x, y, z in zip(a, b, c):
        assert bool(th.isfinite(x).all())
        assert th.equal(x, y) and th.equal(x, z)


def test_cache_stats_and_in_place_edit_misses():
    import drtk_amd.geometry as G

    v, vi = _sphere_views(2, "10k")
    vi = vi.clone()
    G.geometry_cache_clear()
    G.vert_normals(v, vi)
    assert G.geometry_cache_stats() == (0, 1, 1)
    G.vert_normals(v, vi)
    G.face_info(v, vi, ["normals"])
    assert G.geometry_cache_stats() == (2, 1, 1)
    before = G.vert_normals(v, vi)
    vi[:, [1, 2]] = vi[:, [2, 1]].clone()  # flip every face: in place, same storage
    after = G.vert_normals(v, vi)
    hits, misses, entries = G.geometry_cache_stats()
    assert misses == 2 and entries == 2
    assert th.allclose(after, -before, atol=1e-6)


def test_graph_capture_replay_equals_eager():
    import drtk_amd
    import drtk_amd.geometry as G

    v, vi = _sphere_views(4, "10k")
    vt = th.rand(v.shape[0], v.shape[1], 2, device=DEV, generator=th.Generator(DEV).manual_seed(4))  # no singular UV
    x = v.clone().requires_grad_(True)
    y = vt.clone().requires_grad_(True)

    def step():
        vn = G.vert_normals(x, vi)
        vb = G.vert_binormals(x, y, vi, vi)
        loss = (vn * vn.roll(1, 1)).sum() + vb.sum()
        loss.backward()
        return vn

    # a cache miss during a capture is an error that says what to do (raised before anything is enqueued)
    G.geometry_cache_clear()
    err = None
    g, s = th.cuda.CUDAGraph(), th.cuda.Stream()
    with th.cuda.stream(s), th.cuda.graph(g, stream=s):
        try:
            G.vert_normals(v, vi)
        except RuntimeError as e:
            err = str(e)
    th.cuda.synchronize()
    assert err is not None and "before the capture" in err, err
    cap = drtk_amd.capture_step(step, [x, y])
    cap()
    th.cuda.synchronize()
    got = (cap.outputs.detach().clone(), x.grad.clone(), y.grad.clone())
    x.grad = y.grad = None
    want = step()
    for a, b in zip(got, (want.detach(), x.grad, y.grad)):
        assert th.equal(a, b)


def test_shading_step_end_to_end_matches_the_composite():
    """transform -> rasterize -> render -> interpolate(vert_normals) -> Lambert -> loss -> backward: grad_v of the HIP
    route against the composite route (vert_normals in PyTorch), float32 against float64, on one coverage."""
    import drtk_amd
    import drtk_amd.geometry as G
    from drtk_amd import synthetic as S

    N, H, W = 2, 96, 128
    v0, vi = S.uv_sphere(*S.MESH_SIZES["10k"], lobes=0.15, dtype=th.float64)
    v0, vi = v0.to(DEV), vi.to(DEV)
    campos, camrot, focal, princpt = S.ring_cameras(N, W, H, device=DEV, dtype=th.float64)
    world = (v0[None].expand(N, -1, -1) + 0.01 * th.randn(N, v0.shape[0], 3, dtype=th.float64, device=DEV,
                                                           generator=th.Generator(DEV).manual_seed(5))).contiguous()
    light = th.tensor([0.3, 0.8, -0.5], device=DEV, dtype=th.float64)
    with th.no_grad():
        index_img = drtk_amd.rasterize(drtk_amd.transform(world.float(), campos.float(), camrot.float(), focal.float(),
                                                          princpt.float()), vi, H, W)
    w = th.rand(N, 1, H, W, device=DEV, dtype=th.float64, generator=th.Generator(DEV).manual_seed(6))

    def step(dtype, normals):
        x = world.to(dtype).clone().requires_grad_(True)
        v_pix = drtk_amd.transform(x, campos.to(dtype), camrot.to(dtype), focal.to(dtype), princpt.to(dtype))
        _, bary = drtk_amd.render(v_pix, vi, index_img)
        vn = normals(x, vi)
        n_img = drtk_amd.interpolate(vn, vi, index_img, bary)
        shade = (n_img * light.to(dtype)[None, :, None, None]).sum(1, keepdim=True).clamp(min=0)
        (shade * w.to(dtype)).sum().backward()
        return x.grad

    def composite(x, vi):
        return th.nn.functional.normalize(G._face_attribute_to_vert_torch(x, vi, G._face_info_torch(x, vi, {"normals"})["normals"]), dim=-1)

    got = step(th.float32, G.vert_normals)
    c32 = step(th.float32, composite)
    c64 = step(th.float64, composite)
    assert float(got.abs().max()) > 0
    assert_within_f64_distance(got, c32, c64, "shading step grad_v")


def test_valence_65536_fan_and_per_view_topology():
    """One vertex in 65 536 faces (its row is summed in chunks), shared and per-view topology: against the float64
    formulation, and bitwise reproducible."""
    import drtk_amd.geometry as G

    F, N = 65536, 3
    ang = th.arange(F + 1, dtype=th.float64) * (2 * np.pi / F)
    ring = th.stack([th.cos(ang), th.sin(ang), 0.2 * th.sin(7 * ang)], -1)
    v0 = th.cat([th.zeros(1, 3, dtype=th.float64), ring])
    vi = th.stack([th.zeros(F, dtype=th.long), th.arange(1, F + 1), th.arange(2, F + 2)], -1)
    vi[-1, 2] = 1
    v = th.stack([v0 * (1 + 0.5 * k) for k in range(N)]).float().to(DEV)
    g = th.randn(N, v.shape[1], 3, device=DEV, generator=th.Generator(DEV).manual_seed(9))
    for vi_x in (vi.to(DEV), vi[None].repeat(N, 1, 1).int().to(DEV)):
        outs = []
        for _ in range(2):
            x = v.clone().requires_grad_(True)
            o = G.vert_normals(x, vi_x)
            o.backward(g)
            outs.append((o.detach(), x.grad))
        assert th.equal(outs[0][0], outs[1][0]) and th.equal(outs[0][1], outs[1][1])
        ref = {}
        for dt in (th.float32, th.float64):
            xc = v.cpu().to(dt).requires_grad_(True)
            o = G.vert_normals(xc, vi_x.cpu())
            o.backward(g.cpu().to(dt))
            ref[dt] = (o.detach(), xc.grad)
        assert_within_f64_distance(outs[0][0], ref[th.float32][0], ref[th.float64][0], "fan normals")
        assert_within_f64_distance(outs[0][1], ref[th.float32][1], ref[th.float64][1], "fan grad_v")


def test_70000_views_of_a_tiny_mesh_and_no_faces():
    import drtk_amd.geometry as G

    N = 70000
    v = th.randn(N, 4, 3, device=DEV, dtype=th.float64, generator=th.Generator(DEV).manual_seed(11))
    vi = th.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], device=DEV)
    g = th.randn(N, 4, 3, device=DEV, dtype=th.float64, generator=th.Generator(DEV).manual_seed(12))
    x = v.clone().requires_grad_(True)
    o = G.vert_normals(x, vi)
    o.backward(g)
    xc = v.cpu().requires_grad_(True)
    oc = G.vert_normals(xc, vi.cpu())
    oc.backward(g.cpu())
    assert th.allclose(o.cpu(), oc, rtol=1e-9, atol=1e-12)
    assert th.allclose(x.grad.cpu(), xc.grad, rtol=1e-7, atol=1e-9 * float(xc.grad.abs().max()))
    fi = G.face_info(v, vi)
    assert th.allclose(fi["areas"].cpu(), G.face_info(v.cpu(), vi.cpu(), ["areas"]), rtol=1e-12)
    # no faces at all
    e = th.zeros(0, 3, dtype=th.int32, device=DEV)
    x = th.randn(2, 5, 3, device=DEV).requires_grad_(True)
    o = G.vert_normals(x, e)
    assert o.shape == (2, 5, 3) and th.equal(o, th.zeros_like(o))
    o.backward(th.ones_like(o))
    assert th.equal(x.grad, th.zeros_like(x))
    assert G.face_info(x, e, ["normals"]).shape == (2, 0, 3)


def _weighted_sum(*outs):
    """a loss with a generic gradient: each output weighted by a fixed pattern (the same on any device)"""
    total = 0
    for o in outs:
        w = th.cos(th.arange(o.numel(), dtype=o.dtype, device=o.device) * 0.37).view_as(o)
        total = total + (o * w).sum()
    return total


_VIEW_CASES = {
    "face_info": lambda G, v, vt, a, vi: _weighted_sum(*G.face_info(v, vi).values()),
    "vert_normals": lambda G, v, vt, a, vi: _weighted_sum(G.vert_normals(v, vi)),
    "vert_normals_fnorms": lambda G, v, vt, a, vi: _weighted_sum(G.vert_normals(v, vi, a[..., :3])),
    "face_attribute_to_vert": lambda G, v, vt, a, vi: _weighted_sum(G.face_attribute_to_vert(v, vi, a)),
    "face_dpdt": lambda G, v, vt, a, vi: _weighted_sum(*G.face_dpdt(v, vt, vi, vi)),
    "vert_binormals": lambda G, v, vt, a, vi: _weighted_sum(G.vert_binormals(v, vt, vi, vi)),
}


@pytest.mark.parametrize("case", list(_VIEW_CASES))
def test_views_and_non_contiguous_inputs_get_their_gradients(case):
    """v an expanded view of one shared mesh, vt a column slice, the per-face attribute a transposed view: the gradient
    reaches every leaf that requires it (also when only one of v and vt does), equal in float64 to the PyTorch
    formulation's on the CPU."""
    import drtk_amd.geometry as G

    d = _load("f64")
    N = 3
    v0, vi = d["band_v"][0], d["band_vi"].long()  # no degenerate face
    V, F = v0.shape[0], vi.shape[0]
    gen = th.Generator().manual_seed(31)
    vt4 = th.rand(N, V, 4, dtype=th.float64, generator=gen)
    vt4[..., 1:3] = d["band_vt"][0][None] + 0.01 * th.rand(N, V, 2, dtype=th.float64, generator=gen)
    attr_t = th.randn(N, 5, F, dtype=th.float64, generator=gen)

    def grads(dev, need):
        leaves = [x.to(dev).clone().requires_grad_(r) for x, r in zip((v0, vt4, attr_t), need)]
        v = leaves[0][None].expand(N, -1, -1)
        vt = leaves[1][..., 1:3]
        attr = leaves[2].transpose(1, 2)
        assert not (v.is_contiguous() or vt.is_contiguous() or attr.is_contiguous())
        loss = _VIEW_CASES[case](G, v, vt, attr, vi.to(dev))
        want = [x for x in leaves if x.requires_grad]
        return [None if g is None else g.cpu() for g in th.autograd.grad(loss, want, allow_unused=True)]

    needs = [(True, True, True)]
    if case in ("face_dpdt", "vert_binormals"):
        needs += [(False, True, False), (True, False, False)]
    for need in needs:
        got, ref = grads(DEV, need), grads("cpu", need)
        assert [g is None for g in got] == [g is None for g in ref], (case, need)
        assert any(g is not None for g in ref)
        for a, b in zip(got, ref):
            if b is not None:
                assert float(b.abs().max()) > 0
                err = float((a - b).abs().max())
                assert err <= 1e-9 * float(b.abs().max()), (case, need, err)


def test_double_backward_is_an_error():
    """The backward passes are kernels: create_graph=True through them raises instead of giving zero second-order
    terms."""
    import drtk_amd.geometry as G

    d = _load("f32")
    v = d["band_v"].to(DEV).requires_grad_(True)
    vt = d["band_vt"].to(DEV)
    vi = d["band_vi"].to(DEV)
    attr = d["band_attr"].to(DEV).requires_grad_(True)
    for out, wrt in ((G.vert_normals(v, vi), v), (G.face_info(v, vi, ["normals"]), v),
                     (G.face_dpdt(v, vt, vi, vi)[0], v), (G.vert_binormals(v, vt, vi, vi), v),
                     (G.face_attribute_to_vert(v, vi, attr), attr)):
        with pytest.raises(RuntimeError, match="double backward"):
            th.autograd.grad(out.sum(), wrt, create_graph=True)
        (g,) = th.autograd.grad(out.sum(), wrt)  # a plain backward still works
        assert bool(th.isfinite(g).all())

