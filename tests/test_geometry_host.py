"""CPU: the mesh geometry of drtk.utils (face_info, vert_normals, face_attribute_to_vert, face_dpdt, vert_binormals,
index) -- names and signatures of the reference, the PyTorch formulation against the reference's own outputs and
VJPs (tests/golden/refpy_geometry_*.npz, written by tests/gen_golden_geometry.py; `seam` with a UV topology of its own),
the C ABI's argument checks and the incidence builders."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch as th
from conftest import ROOT

from f64_distance import assert_within_f64_distance

NAMES = ("band", "poles", "multi", "seam")


def _load(tag):
    """the three meshes of refpy_geometry_<tag>.npz and the seam mesh of refpy_geometry_seam_<tag>.npz, in one dict"""
    d = {}
    for stem in (f"refpy_geometry_{tag}", f"refpy_geometry_seam_{tag}"):
        z = np.load(os.path.join(ROOT, "tests", "golden", stem + ".npz"))
        d.update({k: th.from_numpy(z[k]) for k in z.files})
    return d


def test_the_seam_fixture_has_a_uv_topology_of_its_own():
    """vti != vi and T = V + n_lat + 1 (a column of UV vertices more than the mesh has), every UV vertex used, and a vertex of
    the mesh's first column listed under two UV vertices: what makes face_dpdt / vert_binormals with the position incidence
    in place of the UV one, or V in place of T, fail on this fixture."""
    d = _load("f64")
    vi, vti = d["seam_vi"].long(), d["seam_vti"].long()
    V, T = d["seam_v"].shape[1], d["seam_vt"].shape[1]
    assert vi.shape == vti.shape == (60, 3) and (V, T) == (36, 42) and not th.equal(vi, vti)
    assert th.equal(vti.unique(), th.arange(T)) and th.equal(vi.unique(), th.arange(V))
    pairs = {(int(a), int(b)) for a, b in zip(vi.reshape(-1), vti.reshape(-1))}
    assert max(sum(1 for a, _ in pairs if a == vert) for vert in range(V)) == 2
    assert d["seam_vt"].shape[0] == 2 and not th.equal(d["seam_vt"][0], d["seam_vt"][1])


def test_drop_in_names_resolve_and_project_points_grad_stays_out():
    import drtk
    import drtk_amd
    from drtk.utils import face_dpdt, face_info, index, vert_binormals, vert_normals  # noqa: F401
    from drtk.utils.geometry import face_attribute_to_vert
    from drtk.utils.indexing import index as index2

    assert index2 is index and face_attribute_to_vert is drtk_amd.face_attribute_to_vert
    for n in ("face_info", "vert_normals", "face_dpdt", "vert_binormals"):
        assert getattr(drtk.utils, n) is getattr(drtk_amd, n), n
    with pytest.raises(AttributeError, match="not provided"):
        drtk.utils.project_points_grad  # noqa: B018


def test_signatures_match_the_reference():
    from drtk.utils import face_dpdt, face_info, index, vert_binormals, vert_normals
    from drtk.utils.geometry import face_attribute_to_vert

    want = {
        face_info: [("v", inspect._empty), ("vi", inspect._empty), ("to_compute", None)],
        vert_normals: [("v", inspect._empty), ("vi", inspect._empty), ("fnorms", None)],
        face_dpdt: [("v", inspect._empty), ("vt", inspect._empty), ("vi", inspect._empty), ("vti", inspect._empty)],
        vert_binormals: [("v", inspect._empty), ("vt", inspect._empty), ("vi", inspect._empty), ("vti", inspect._empty)],
        face_attribute_to_vert: [("v", inspect._empty), ("vi", inspect._empty), ("attr", inspect._empty)],
        index: [("x", inspect._empty), ("idxs", inspect._empty), ("dim", inspect._empty)],
    }
    for fn, params in want.items():
        got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
        assert got == params, (fn.__name__, got)


def test_index_matches_the_reference_example():
    from drtk.utils import index

    x = th.randn(2, 7, 3)
    idxs = th.randint(0, 7, (5, 3))
    y = index(x, idxs, 1)
    assert y.shape == (2, 5, 3, 3)
    assert th.equal(y[1, 4, 2], x[1, idxs[4, 2]])


def _run_all(d, name, dtype, idx_dtype=th.int64):
    """The CPU formulation on the fixture's inputs: {output or VJP name: tensor}"""
    from drtk.utils.geometry import face_attribute_to_vert, face_dpdt, face_info, vert_binormals, vert_normals

    p = lambda k: d[f"{name}_{k}"].clone()  # noqa: E731  (fresh leaves: .to() of the same dtype is no copy)
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
    return res


@pytest.mark.parametrize("idx_dtype", [th.int32, th.int64])
@pytest.mark.parametrize("name", NAMES)
def test_cpu_formulation_float64_matches_the_reference(name, idx_dtype):
    d = _load("f64")
    got = _run_all(d, name, th.float64, idx_dtype)
    assert got
    for k, t in got.items():
        ref = d[f"{name}_{k}"]
        scale = max(1.0, float(ref.abs().max()))
        err = float((t.detach() - ref).abs().max())
        assert err <= 1e-12 * scale, (name, k, err, scale)


@pytest.mark.parametrize("name", NAMES)
def test_cpu_formulation_float32_within_the_f64_distance(name):
    d32, d64 = _load("f32"), _load("f64")
    got = _run_all(d32, name, th.float32)
    for k, t in got.items():
        assert_within_f64_distance(t, d32[f"{name}_{k}"], d64[f"{name}_{k}"], f"{name} {k}")


def test_degenerate_branches_reproduce_the_composite():
    """A face with c = 0 has a zero normal and a 1e8-scaled gradient; a vertex whose summed normal vanishes (here an
    unreferenced one) gets 1e12 * g from F.normalize -- both as in the fixtures."""
    d = _load("f64")
    got = _run_all(d, "poles", th.float64)
    assert float(got["face_info_grad_v"].abs().max()) > 1e6
    assert float((got["face_info_normals"].norm(dim=-1) == 0).sum()) > 0
    got = _run_all(d, "multi", th.float64)
    assert float(got["vert_normals_grad_v"].abs().max()) == pytest.approx(float(d["multi_vert_normals_grad_v"].abs().max()))
    assert th.equal(got["vert_normals"][:, 6], th.zeros(2, 3, dtype=th.float64))


def test_numpy_incidence_rows_are_ascending_and_match_the_operator():
    from drtk_amd import capi

    rng = np.random.default_rng(0)
    vi = rng.integers(0, 40, size=(3, 300, 3))
    vi[:, :150, 0] = 7  # one row longer than a chunk
    crow, entries, cptr, cbeg, crow_of = capi.vertex_incidence_numpy(vi, 40, chunk=64)
    assert crow[0] == 0 and crow[-1] == entries.size == vi.size
    for r in range(3 * 40):
        row = entries[crow[r]:crow[r + 1]]
        assert np.all(np.diff(row) > 0), r
        b, vert = divmod(r, 40)
        assert np.all(vi[b].reshape(-1)[row] == vert)
    long_rows = np.nonzero(np.diff(cptr))[0]
    assert set(long_rows) == {7, 47, 87} and np.all(crow_of[cptr[7]:cptr[8]] == 7)
    assert np.array_equal(cbeg[cptr[7]:cptr[8]], crow[7] + 64 * np.arange(cptr[8] - cptr[7]))
    import drtk_amd  # noqa: F401 -- registers the operators

    c2, e2 = th.ops.drtk_amd_ext.vertex_incidence(th.from_numpy(vi), 40)
    assert np.array_equal(c2.numpy(), crow) and np.array_equal(e2.numpy(), entries)
    c3, e3 = th.ops.drtk_amd_ext.vertex_incidence(th.from_numpy(vi[0]).int(), 40)
    ref = capi.vertex_incidence_numpy(vi[0], 40)
    assert np.array_equal(c3.numpy(), ref[0]) and np.array_equal(e3.numpy(), ref[1])
    fan = np.stack([np.zeros(600, np.int64), np.arange(1, 601), np.arange(2, 602)], -1)  # row 0: 600 > one chunk
    c4, e4 = th.ops.drtk_amd_ext.vertex_incidence(th.from_numpy(fan), 602)
    ref = capi.vertex_incidence_numpy(fan, 602)
    assert np.array_equal(c4.numpy(), ref[0]) and np.array_equal(e4.numpy(), ref[1]) and ref[2][1] == 3
    with pytest.raises(RuntimeError, match="outside"):
        th.ops.drtk_amd_ext.vertex_incidence(th.tensor([[0, 1, 40]]), 40)


def test_geometry_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    z, nz = ctypes.c_void_p(0), ctypes.c_void_p(16)
    i64 = ctypes.c_int64
    out = ctypes.c_size_t(0)
    assert L.drtk_amd_geometry_vertex_gather_workspace_bytes(ctypes.c_int(0), i64(8), i64(1), i64(5), i64(3), ctypes.byref(out)) == 0
    assert out.value == 8 * 5 * 3 * 4
    assert L.drtk_amd_geometry_vertex_gather_workspace_bytes(ctypes.c_int(1), i64(8), i64(8), i64(5), i64(2), ctypes.byref(out)) == 0
    assert out.value == 5 * 2 * 8
    assert L.drtk_amd_geometry_vertex_gather_workspace_bytes(ctypes.c_int(0), i64(8), i64(3), i64(5), i64(3), ctypes.byref(out)) == -1
    assert L.drtk_amd_geometry_vertex_gather_workspace_bytes(ctypes.c_int(2), i64(8), i64(1), i64(5), i64(3), ctypes.byref(out)) == -1

    def fwd(dtype=0, N=1, V=3, T=0, F=1, normals=nz, vt=z, vti=z, dpdt=z, v_sN=9, vi_sN=0):
        return L.drtk_amd_geometry_face_forward(ctypes.c_int(dtype), nz, i64(v_sN), nz, i64(vi_sN), vt, i64(2 * T), vti,
                                                i64(N), i64(V), i64(T), i64(F), normals, z, z, dpdt, z, z, z)
    assert fwd(dtype=2) == -1                 # unknown dtype
    assert fwd(normals=z) == -1               # nothing requested
    assert fwd(V=-1) == -1 and fwd(v_sN=7) == -1 and fwd(vi_sN=5) == -1
    assert fwd(dpdt=nz, normals=z) == -1      # dpdt without vt / vti
    assert fwd(N=0) == 0 and fwd(F=0) == 0    # nothing to do: no launch

    def bwd(vt=z, uv=z, g_normals=z, g_dpdt=z, sums=z, g_vert=z, N=1, F=1):
        return L.drtk_amd_geometry_face_backward(ctypes.c_int(0), nz, i64(9), nz, i64(0), vt, i64(0), nz, i64(N), i64(3),
                                                 i64(0), i64(F), g_vert, sums, g_normals, z, z, g_dpdt, z, nz, uv, z)
    assert bwd(g_dpdt=nz) == -1               # dpdt gradient without vt
    assert bwd(vt=nz, g_normals=nz, uv=nz) == -1  # normals gradient in the dpdt pass
    assert bwd(vt=nz) == -1                   # dpdt pass without uv rows
    assert bwd(sums=nz) == -1                 # sums without the vertex gradient
    assert bwd(N=0) == 0

    def gat(A=3, per_corner=0, src_sN=3, normalize=0, sums=z, C=0, ws=z, wsb=0, B=1, N=1):
        return L.drtk_amd_geometry_vertex_gather(ctypes.c_int(0), nz, i64(src_sN), ctypes.c_int(per_corner), i64(A), nz, nz,
                                                 nz, nz, nz, i64(C), i64(B), i64(N), i64(3), i64(1), ctypes.c_int(normalize),
                                                 nz, sums, ws, ctypes.c_size_t(wsb), z)
    assert gat(src_sN=4) == -1 and gat(per_corner=1) == -1 and gat(per_corner=2) == -1
    assert gat(A=2, src_sN=2, normalize=1) == -1   # normalize needs A = 3
    assert gat(sums=nz) == -1                      # sums without normalize
    assert gat(B=2) == -1                          # B is 1 or N
    assert gat(C=2) == -2                          # chunks need a workspace
    assert gat(N=0) == 0
    assert L.drtk_amd_geometry_face_gather(ctypes.c_int(0), nz, nz, nz, i64(0), i64(1), i64(3), i64(1), i64(2), nz, z) == -1
