"""TEST INFRASTRUCTURE ONLY (not collected by pytest) -- seeded random cases for the mesh-geometry helpers of
csrc/geometry.hip: `face_info`, `vert_normals` (from v and from given fnorms), `face_attribute_to_vert`, `face_dpdt` and
`vert_binormals`.  Every case runs all six forward and backward through the Python API on the device, and through the ctypes
binding of the C ABI composed by test_gpu_geometry._run_all_capi (poisoned outputs; with DRTK_CAPI_GUARD sentinels around
every output and workspace).  The two routes agree bit for bit, and so do the first result and a repeat from a cold incidence
cache.  The reference is the PyTorch formulation of drtk_amd/geometry.py on CPU tensors under autograd (pinned to the
reference's library by the fixtures of tests/test_geometry_host.py, `seam` with its own UV topology among them), on the very
inputs the device gets -- rounded to float32 first in a float32 case -- in float64 as the oracle and in float32 as the
`oracle_f32` of tests/f64_distance.py.  No bound is stated here: check_float64, check_float32, _near_degenerate and _split of
tests/test_gpu_geometry.py are the fixture test's.

usage: python tests/fuzz_geometry.py [--first S] [--cases K]      cases make_case(S) .. make_case(S + K - 1)

"Towards X" below: one draw in three picks from the list X, the others are uniform in the stated range.

uv topology: one case in eight is `few` on a soup of 500 .. 600 faces (3 .. 6 UV vertices, so a UV vertex's row has more than
DRTK_GEOMETRY_CHUNK entries: the chunk kernel with A = 2 through the UV incidence); the others one of
  same     vti = vi, T = V (not with degenerate faces: a face that lists a vertex twice has a singular UV matrix);
  seam     a grid_mesh cut along a column, or a sphere_mesh with a latitude / longitude atlas that has a column more than the
           mesh and one UV vertex per pole face: T > V;
  corners  vti = arange(3 F).view(F, 3), T = 3 F;
  few      3 .. 6 UV vertices on a circle (no three collinear), each face three distinct ones.
mesh (laplacian_oracle): seam: grid_mesh(2 .. 12, 2 .. 12) or sphere_mesh(3 .. 16, 2 .. 12); otherwise soup_mesh three times
in seven, grid_mesh once, fan_mesh twice, sphere_mesh once.  soup: V 3 .. 300, F 1 .. 600; one soup in three takes F so that
N F is one of 255, 256, 257, 511, 512, 513 (N a divisor of it), one in three V so that N V is (degenerate faces and vertices
counted).  fan: valence towards 255, 256, 257, 300, 511, 512, 513 -- such a case runs all seven, with the attribute widths
3, 4, 1, 2, 5, 9, 8 in that order, so that the rows of more than a chunk meet A = 1, 2, 5 and 9 --, else 2 .. 700.
laplacian_oracle.sphere_mesh has one vertex per pole and no degenerate face; faces whose c is exactly 0 come from
with_degenerates (a face that lists a vertex twice, a collinear face with integer coordinates, an unreferenced vertex), one
case in four.
views: N 1 .. 4, view n the mesh scaled by 1 + 0.1 n and moved by 0.02 randn.  position topology: [F,3], [1,F,3], [N,F,3]
expanded, or (soups, twice as often) [N,F,3] with a face list per view: a permutation of the faces with 1 .. 3 of them
replaced by other faces of the same soup, the degenerate faces last; face_dpdt and vert_binormals take the shared list.
int32 / int64 indices.  A of face_attribute_to_vert towards 1, 2, 3, 4, 5, 8, 9, else 1 .. 9.  float32 / float64.  A random
non-empty subset of v, vt, fnorms and attr requires a gradient; face_info runs with a random non-empty subset of its outputs
and upstream gradients on a random non-empty subset of those.  layout: contiguous / v expanded from one shared mesh (every
view then has the vertices of view 0) / vt a column slice of a wider tensor / attr a transposed view; the gradient is
compared at the view and at the leaf.

Conditions on a draw, checked on the CPU (tests/test_fuzz_geometry_host.py asserts them for every seed); a draw that misses
one is drawn again, all of it, from a generator seeded with (seed, attempt), at most 20 times:
  (a) no face has 0 < 2 area < 1e-6 (in float64, any view): degenerate faces are exactly degenerate;
  (b) no face has a UV matrix with |det| < 1e-3 |t1 - t0| |t2 - t0|;
  (c) a float32 case: for every output and gradient, over the entries compared under the bound,
      3 max|oracle_f32 - oracle_f64| <= 1e-3 max|oracle_f64| (the bound stays within 100 times its floor);
  (d) at most 2 % of the faces are degenerate and at most 10 % of the vertices touch one.

tests/test_gpu_fuzz_geometry.py runs seeds 0 .. 239 in six blocks of 40 (tests/test_fuzz_geometry_host.py counts what they
hold); tests/guarded_added_ops.py runs the first 20 under guards.
Measured on an MI355X: a block of 40 cases takes 0.7 to 0.9 s, the first one 2.8 s (the first use of every library), the CPU
oracles and the draws included; all six blocks 7.9 s; `--first 0 --cases 240` runs its cases in 7.6 s.  For comparison:
tests/test_gpu_geometry.py took 3.5 s (36 tests) at the parent commit and takes 4.0 s (42 tests) now.

What it found: with the 2x2 UV inverse of face_dpdt carried in float32, seeds 13, 99, 155 and 207 (float32, a sliver UV
triangle among the faces) failed -- face_dpdt at 1.02, 1.1 and 1.7 times the bound and vert_binormals' gradient to vt at 1.1
times, the kernel 3.0 to 5.7 times as far from the float64 result as the PyTorch formulation's pivoted float32 inverse.
csrc/geometry.hip now forms the inverse and what goes through it in double; all 240 seeds pass.

Mutations of the kernels, each on a scratch copy, seeds 0 .. 239 (all of them plain failed assertions):
  (i)   dpdt_prep builds the UV incidence from vi (run on the 145 seeds whose position indices are all below T): 113 fail,
        seed 1 the first (face_dpdt: the face pass reads its UV corners through that incidence's index list too);
        tests/test_gpu_geometry.py of the parent commit passes (vti = vi, T = V throughout).
  (ii)  geom_vertex_gather_kernel stops one chunk early (`c < c1 - 1`): 51 fail, seed 4 the first; of the parent's
        tests/test_gpu_geometry.py only test_valence_65536_fan_and_per_view_topology fails.
  (iii) geom_vertex_chunk_kernel starts a row's last chunk one entry late where it is shorter than a chunk: 49 fail, seed 4 the
        first; tests/test_gpu_geometry.py of the parent commit passes (its one long row is 256 whole chunks).
"""
import argparse
import os

os.environ.setdefault("DRTK_CAPI_POISON", "1")  # outputs of the ctypes binding pre-filled with NaN / sentinels (drtk_amd/capi.py _out)
import functools
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import laplacian_oracle as LO  # noqa: E402

DEV = "cuda:0"
DTYPES = {"f32": th.float32, "f64": th.float64}
CHUNK, BLOCK = 256, 256  # DRTK_GEOMETRY_CHUNK of include/drtk_amd.h, kBlock of csrc/common.hpp (tests/test_fuzz_geometry_host.py reads both)
NEAR_VALENCE = (CHUNK - 1, CHUNK, CHUNK + 1, 300, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)
NEAR_VALENCE_A = (3, 4, 1, 2, 5, 9, 8)  # the attribute width of each of those runs
NEAR_LANES = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1)
NEAR_A = (1, 2, 3, 4, 5, 8, 9)
UV = ("same", "seam", "corners", "few")
MESHES = ("soup", "soup", "soup", "grid", "fan", "fan", "sphere")
TOPOLOGY = ("F3", "1F3", "NF3_expand", "NF3")
LAYOUTS = ("contiguous", "v_expanded", "vt_slice", "attr_transposed")
KINDS = ("normals", "areas", "edges")
NEEDS = ("v", "vt", "fnorms", "attr")
SPARE = 12  # faces a soup draws beyond its F: up to three per view replace faces of that view's list
MAX_ATTEMPTS = 20


# ---- what the cases are drawn from ---------------------------------------------------------------------------------------------
def soup_is_possible(V, seed):
    """Has soup_mesh(V, ., seed) a face to draw?  (Its faces have corner angles above 0.4: a handful of vertices may have none.)"""
    if V > 12:
        return True
    v = np.random.default_rng(seed).uniform(-1, 1, (V, 3))
    for a in range(V):
        for b in range(a + 1, V):
            for c in range(b + 1, V):
                p = v[[a, b, c]]
                cos = [np.dot(p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]) / (np.linalg.norm(p[(k + 1) % 3] - p[k]) * np.linalg.norm(p[(k + 2) % 3] - p[k])) for k in range(3)]
                if max(cos) < np.cos(0.4):
                    return True
    return False


def draw(seed, attempt):
    """A dict of plain numbers and names; the tensors are made from them in `inputs`."""
    g = th.Generator().manual_seed(1000003 * seed + 7919 * attempt + 17)
    r = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    pick = lambda seq: seq[r(0, len(seq) - 1)]  # noqa: E731
    towards = lambda near, lo, hi: pick(near) if r(0, 2) == 0 else r(lo, hi)  # noqa: E731
    flag = lambda: r(0, 1) == 1  # noqa: E731
    subset = lambda names: tuple(k for k in names if flag()) or (pick(names),)  # noqa: E731
    c = dict(seed=seed, attempt=attempt)
    degenerate = r(0, 3) == 0
    big_few = r(0, 7) == 0
    uv = "few" if big_few else pick(UV if not degenerate else tuple(u for u in UV if u != "same"))
    mesh = "soup" if big_few else pick(("grid", "sphere")) if uv == "seam" else pick(MESHES)
    N = r(1, 4)
    c.update(uv=uv, mesh=mesh)
    if mesh == "soup":
        V, F = r(3, 300), r(500, 600) if big_few else r(1, 600)
        extra_f, extra_v = (2, 4) if degenerate else (0, 0)
        lanes_f = pick(NEAR_LANES) if r(0, 2) == 0 and not big_few else None
        lanes_v = pick(NEAR_LANES) if r(0, 2) == 0 else None
        if lanes_f is not None:
            N = pick([n for n in range(1, 5) if lanes_f % n == 0 and lanes_f // n - extra_f >= 1])
            F = lanes_f // N - extra_f
        if lanes_v is not None:
            fits = [t for t in NEAR_LANES if t % N == 0 and t // N - extra_v >= 3]
            if lanes_f is None:
                N = pick([n for n in range(1, 5) if lanes_v % n == 0])
                V = lanes_v // N - extra_v
            elif fits:
                V = pick(fits) // N - extra_v
        c.update(V=V, F=F, mesh_seed=r(0, 10 ** 6))
        while not soup_is_possible(c["V"], c["mesh_seed"]):
            c["mesh_seed"] += 1
    elif mesh == "grid":
        c.update(rows=r(2, 12), cols=r(2, 12), mesh_seed=r(0, 10 ** 6))
        c["cut"] = r(1, c["cols"] - 1)
    elif mesh == "fan":
        c.update(valences=tuple(NEAR_VALENCE) if r(0, 2) == 0 else (r(2, 700),))
    else:
        c.update(segments=r(3, 16), rings=r(2, 12))
    topology = pick(TOPOLOGY + ("NF3",)) if mesh == "soup" else pick(TOPOLOGY[:3])
    c.update(degenerate=degenerate, N=N, topology=topology, vi_dtype=pick(("int32", "int64")), A=towards(NEAR_A, 1, 9), T=r(3, 6),
             dtype=pick(("f32", "f64")), needs=subset(NEEDS), layout=pick(LAYOUTS), data_seed=r(0, 10 ** 6))
    c["kinds"] = subset(KINDS)
    c["upstream"] = subset(c["kinds"])
    return c


def describe(c):
    return " ".join(f"{k}={v}" for k, v in c.items())


def runs(c):
    """The runs of a case, as descriptions of their own: one, or the fans of a case drawn towards the chunk boundaries"""
    if c["mesh"] != "fan":
        return [dict(c, run=0)]
    listed = c["valences"] == tuple(NEAR_VALENCE)
    return [dict(c, run=i, valence=valence, A=NEAR_VALENCE_A[i] if listed else c["A"]) for i, valence in enumerate(c["valences"])]


# ---- the inputs of a run ---------------------------------------------------------------------------------------------------------
def circle(T, g):
    """T points on a circle at distinct angles: no three collinear"""
    ang = 2 * np.pi * (th.arange(T, dtype=th.float64) + 0.6 * th.rand(T, generator=g, dtype=th.float64) - 0.3) / T
    return 0.5 + 0.4 * th.stack([th.cos(ang), th.sin(ang)], -1)


def position_mesh(c):
    """(v0 [V,3] float64, vi [F,3] int64 with the degenerate faces last, spare faces [k,3], how many faces are proper)"""
    spare = th.zeros(0, 3, dtype=th.long)
    if c["mesh"] == "soup":
        v0, faces = LO.soup_mesh(c["V"], c["F"] + SPARE, c["mesh_seed"])
        vi, spare = faces[:c["F"]], faces[c["F"]:]
    elif c["mesh"] == "grid":
        v0, vi = LO.grid_mesh(c["rows"], c["cols"], c["mesh_seed"])
    elif c["mesh"] == "fan":
        v0, vi = LO.fan_mesh(c["valence"])
    else:
        v0, vi = LO.sphere_mesh(c["segments"], c["rings"])
    proper = vi.shape[0]
    if c["degenerate"]:
        v0, vi = LO.with_degenerates(v0, vi)
    return v0, vi, spare, proper


def atlas(c):
    """(vt0 [T,2] float64, vti [F,3] int64, the smaller side of a cell) of a `seam` case's proper faces, in the order of the mesh's"""
    if c["mesh"] == "grid":
        rows, cols, cut = c["rows"], c["cols"], c["cut"]
        r_, c_ = (t.ravel() for t in np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij"))
        shift = (c_ >= cut).astype(np.int64)  # the cells right of the cut take the second copy of column `cut`
        uid = lambda r, k: r * (cols + 1) + k + shift  # noqa: E731
        a, b, cc, d = uid(r_, c_), uid(r_, c_ + 1), uid(r_ + 1, c_), uid(r_ + 1, c_ + 1)
        vti = np.concatenate([np.stack([a, b, cc], -1), np.stack([b, d, cc], -1)])  # grid_mesh's order
        nr, nc = rows, cols + 1
    else:
        seg, rings = c["segments"], c["rings"]
        uid = lambda r, k: r * (seg + 1) + k  # noqa: E731
        j = np.arange(seg)
        faces = [np.stack([uid(0, j), uid(1, j), uid(1, j + 1)], -1), np.stack([uid(rings, j), uid(rings - 1, j + 1), uid(rings - 1, j)], -1)]
        i_, j_ = (t.ravel() for t in np.meshgrid(np.arange(1, rings - 1), j, indexing="ij"))
        a, b, cc, d = uid(i_, j_), uid(i_, j_ + 1), uid(i_ + 1, j_), uid(i_ + 1, j_ + 1)
        faces += [np.stack([a, cc, b], -1), np.stack([b, cc, d], -1)]  # sphere_mesh's order
        vti = np.concatenate(faces)
        nr, nc = rings + 1, seg + 1
    w, u = np.meshgrid(0.02 + 0.96 * np.arange(nr) / (nr - 1), 0.02 + 0.96 * np.arange(nc) / (nc - 1), indexing="ij")
    return th.from_numpy(np.stack([u, w], -1).reshape(-1, 2)), th.from_numpy(vti.astype(np.int64)), 0.96 / max(nr - 1, nc - 1)


@functools.lru_cache(maxsize=64)
def _inputs(key):
    c = dict(key)
    g = th.Generator().manual_seed(7 * c["data_seed"] + c["run"])
    rand = lambda *s: th.rand(*s, generator=g, dtype=th.float64)  # noqa: E731
    randn = lambda *s: th.randn(*s, generator=g, dtype=th.float64)  # noqa: E731
    N, A = c["N"], c["A"]
    v0, vi, spare, proper = position_mesh(c)
    V, F = v0.shape[0], vi.shape[0]
    v = v0[None] * (1 + 0.1 * th.arange(N, dtype=th.float64))[:, None, None] + 0.02 * randn(N, V, 3)
    if c["degenerate"]:
        v[:, -3:] = v0[-3:]  # the collinear face keeps its integer coordinates
    if c["layout"] == "v_expanded":
        v = v[:1].expand(N, -1, -1).contiguous()
    # UV vertices and their topology
    if c["uv"] == "same":
        vt0, vti, jitter = rand(V, 2), vi.clone(), 0.01
    elif c["uv"] == "seam":
        vt0, vti, cell = atlas(c)
        jitter = 0.05 * cell
        if c["degenerate"]:  # the two degenerate faces: a UV triangle of their own each
            T0 = vt0.shape[0]
            vt0 = th.cat([vt0, circle(3, g), circle(3, g)])
            vti = th.cat([vti, T0 + th.arange(6).view(2, 3)])
    elif c["uv"] == "corners":
        vt0, vti, jitter = rand(3 * F, 2), th.arange(3 * F).view(F, 3), 0.01
    else:
        vt0, jitter = circle(c["T"], g), 0.01
        vti = th.stack([th.randperm(c["T"], generator=g)[:3] for _ in range(F)])
    vt = vt0[None] + jitter * (2 * rand(N, *vt0.shape) - 1)
    # the position topology as the functions get it (the index type first: a conversion would copy an expanded tensor)
    vi, spare, vti = (x.to(getattr(th, c["vi_dtype"])) for x in (vi, spare, vti))
    shared = vi
    if c["topology"] == "NF3":
        lists = []
        for n in range(N):
            t = vi[:proper][th.randperm(proper, generator=g)].clone()
            k = min(int(th.randint(1, 4, (1,), generator=g)), proper)
            t[th.randperm(proper, generator=g)[:k]] = spare[3 * n:3 * n + k]
            lists.append(th.cat([t, vi[proper:]]))
        vi = th.stack(lists)
    elif c["topology"] == "1F3":
        vi = vi[None]
    elif c["topology"] == "NF3_expand":
        vi = vi[None].expand(N, -1, -1)
    t = dict(v=v, vt=vt, vi=vi, vi_shared=shared, vti=vti, fnorms=randn(N, F, 3), attr=randn(N, F, A))
    shapes = dict(face_info_normals=(N, F, 3), face_info_areas=(N, F, 1), face_info_edges=(N, F, 3, 3), vert_normals=(N, V, 3),
                  face_attribute_to_vert=(N, V, A), face_dpdt=(N, F, 2, 3), face_dpdt_v012=(N, F, 3, 3), vert_binormals=(N, V, 3))
    for k, s in shapes.items():
        if not k.startswith("face_info_") or k[len("face_info_"):] in c["upstream"]:
            t["g_" + k] = randn(*s)
    if c["dtype"] == "f32":  # the very values the device gets
        t = {k: (x.float().double() if x.is_floating_point() else x) for k, x in t.items()}
    return t


def inputs(c):
    """The tensors of a run on the CPU: float64 (holding float32 values in a float32 case), indices in the case's type; vi in
    the case's position topology, vi_shared [F,3] for face_dpdt and vert_binormals.  Shared by every use: not to be changed."""
    return _inputs(tuple(sorted((k, v) for k, v in c.items())))


# ---- the six functions, on any device ------------------------------------------------------------------------------------------------
def apply(c, t, dtype, dev):
    """Every function forward and backward through drtk_amd.geometry on the run's inputs `t` in `dtype` on `dev` (CPU tensors
    take its PyTorch formulation), the inputs in the case's layout: {name: CPU tensor} under the fixtures' names; a gradient
    at the view the function got, and `<name>_leaf` at the leaf it is a view of where the layout makes one."""
    import drtk_amd.geometry as G

    needs, layout, N = c["needs"], c["layout"], c["N"]
    to = lambda k: t[k].to(dtype).to(dev)  # noqa: E731
    vi, vi_shared, vti = (t[k].to(dev) for k in ("vi", "vi_shared", "vti"))  # (.to(dev) keeps an expanded tensor's strides)
    res = {}

    def leaf_v(req):
        if layout == "v_expanded":
            leaf = to("v")[0].clone().requires_grad_(req)
            view = leaf[None].expand(N, -1, -1)
        else:
            leaf = view = to("v").clone().requires_grad_(req)
        return leaf, view

    def leaf_vt(req):
        if layout == "vt_slice":
            wide = th.full((*t["vt"].shape[:2], 4), float("nan"), dtype=dtype, device=dev)
            wide[..., 1:3] = to("vt")
            leaf = wide.requires_grad_(req)
            return leaf, leaf[..., 1:3]
        leaf = to("vt").clone().requires_grad_(req)
        return leaf, leaf

    def leaf_attr(req):
        if layout == "attr_transposed":
            leaf = to("attr").transpose(1, 2).contiguous().requires_grad_(req)
            return leaf, leaf.transpose(1, 2)
        leaf = to("attr").clone().requires_grad_(req)
        return leaf, leaf

    def backward(outs, grads, wrt):
        """grads of `outs` into the (leaf, view, name) of `wrt` that require one"""
        wrt = [(leaf, view, name) for leaf, view, name in wrt if leaf.requires_grad]
        if not wrt:
            return
        for leaf, view, _ in wrt:
            if view is not leaf:
                view.retain_grad()
        pairs = [(o, g) for o, g in zip(outs, grads) if o.requires_grad]  # (face_dpdt's v012 does not depend on vt)
        th.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        for leaf, view, name in wrt:
            res[name] = view.grad
            if view is not leaf:
                res[name + "_leaf"] = leaf.grad

    kinds = [k for k in KINDS if k in c["kinds"]]
    lv, v = leaf_v("v" in needs)
    fi = G.face_info(v, vi, list(kinds))
    fi = fi if isinstance(fi, dict) else {kinds[0]: fi}
    res.update({f"face_info_{k}": fi[k] for k in kinds})
    up = [k for k in kinds if k in c["upstream"]]
    backward([fi[k] for k in up], [to(f"g_face_info_{k}") for k in up], [(lv, v, "face_info_grad_v")])
    lv, v = leaf_v("v" in needs)
    res["vert_normals"] = G.vert_normals(v, vi)
    backward([res["vert_normals"]], [to("g_vert_normals")], [(lv, v, "vert_normals_grad_v")])
    fn = to("fnorms").clone().requires_grad_("fnorms" in needs)
    res["vert_normals_fnorms"] = G.vert_normals(leaf_v(False)[1], vi, fn)
    backward([res["vert_normals_fnorms"]], [to("g_vert_normals")], [(fn, fn, "vert_normals_grad_fnorms")])
    la, attr = leaf_attr("attr" in needs)
    res["face_attribute_to_vert"] = G.face_attribute_to_vert(leaf_v(False)[1], vi, attr)
    backward([res["face_attribute_to_vert"]], [to("g_face_attribute_to_vert")], [(la, attr, "face_attribute_to_vert_grad_attr")])
    (lv, v), (lt, vt) = leaf_v("v" in needs), leaf_vt("vt" in needs)
    res["face_dpdt"], res["face_dpdt_v012"] = G.face_dpdt(v, vt, vi_shared, vti)
    backward([res["face_dpdt"], res["face_dpdt_v012"]], [to("g_face_dpdt"), to("g_face_dpdt_v012")],
             [(lv, v, "face_dpdt_grad_v"), (lt, vt, "face_dpdt_grad_vt")])
    (lv, v), (lt, vt) = leaf_v("v" in needs), leaf_vt("vt" in needs)
    res["vert_binormals"] = G.vert_binormals(v, vt, vi_shared, vti)
    backward([res["vert_binormals"]], [to("g_vert_binormals")], [(lv, v, "vert_binormals_grad_v"), (lt, vt, "vert_binormals_grad_vt")])
    return {k: x.detach().cpu() for k, x in res.items()}


@functools.lru_cache(maxsize=64)
def _oracles(key):
    c = dict(key)
    t = inputs(c)
    return apply(c, t, th.float64, "cpu"), (apply(c, t, th.float32, "cpu") if c["dtype"] == "f32" else None)


def oracles(c):
    """(the PyTorch formulation on the run's inputs in float64, the same in float32 for a float32 case or None)"""
    return _oracles(tuple(sorted((k, v) for k, v in c.items())))


def degenerate_sets(c, t):
    """(faces [N,F], vertices [N,V]) of test_gpu_geometry._near_degenerate, from the float64 formulation's areas"""
    import drtk_amd.geometry as G
    import test_gpu_geometry as T

    areas = G.face_info(t["v"], t["vi"], ["areas"])
    return T._near_degenerate(areas, t["vi"], t["v"].shape[1])


def sets_of(k, x, faces, verts):
    """(the fixtures' name of result k, faces, vertices) as test_gpu_geometry._split takes them: a gradient at the leaf of an
    expanded v [V,3] is split at the vertices that touch a degenerate face in any view"""
    import test_gpu_geometry as T

    name = k[:-len("_leaf")] if k.endswith("_leaf") else k
    return name, faces, (verts.any(0) if name != k and name in T._VERT_C and x.dim() == 2 else verts)


def compared(k, x, faces, verts):
    """the entries of result k that are compared under the bound"""
    import test_gpu_geometry as T

    name, f, vs = sets_of(k, x, faces, verts)
    return T._split(name, x, f, vs)[0]


def uv_determinants(t):
    """(|det| [N,F], |t1 - t0| |t2 - t0| [N,F]) of the faces' UV matrices"""
    import drtk_amd.geometry as G

    t012 = G._corners(t["vt"], t["vti"])
    d = t012[:, :, 1:3] - t012[:, :, 0:1]
    return th.linalg.det(d).abs(), d[:, :, 0].norm(dim=-1) * d[:, :, 1].norm(dim=-1)


def missed_condition(c):
    """None where every run of the case meets (a) .. (d) of the module's docstring, else which one it misses"""
    import drtk_amd.geometry as G

    for run in runs(c):
        t = inputs(run)
        two_area = 2 * th.cat([G.face_info(t["v"], t[k], ["areas"])[..., 0] for k in ("vi", "vi_shared")], 1)
        if bool(((two_area > 0) & (two_area < 1e-6)).any()):
            return "a"
        det, scale = uv_determinants(t)
        if bool((det < 1e-3 * scale).any()):
            return "b"
        faces, verts = degenerate_sets(run, t)
        if float(faces.double().mean(1).max()) > 0.02 or float(verts.double().mean(1).max()) > 0.10:
            return "d"
        o64, o32 = oracles(run)
        if o32 is not None:
            for k in o64:
                a, b = compared(k, o32[k].double(), faces, verts), compared(k, o64[k], faces, verts)
                if a.numel() and 3 * float((a - b).abs().max()) > 1e-3 * float(b.abs().max()):
                    return "c"
    return None


@functools.lru_cache(maxsize=None)
def make_case(seed):
    """The first draw of `seed` that meets the conditions"""
    for attempt in range(MAX_ATTEMPTS):
        c = draw(seed, attempt)
        if missed_condition(c) is None:
            return c
    raise AssertionError(f"seed {seed}: no draw in {MAX_ATTEMPTS} meets the conditions")


# ---- a case against its oracle ---------------------------------------------------------------------------------------------------------
def compare(got, c, t, dtype, what):
    """`got` (of a run in `dtype`) against the oracles under the bound of the case's precision"""
    import test_gpu_geometry as T

    o64, o32 = oracles(c)
    faces, verts = degenerate_sets(c, t)
    assert set(got) == set(o64), (what, sorted(set(got) ^ set(o64)))
    for k, x in got.items():
        assert x.shape == o64[k].shape and x.dtype == dtype, (what, k, x.shape, x.dtype)
        name, f, vs = sets_of(k, x, faces, verts)
        if c["dtype"] == "f64":
            T.check_float64(name, x, o64[k], f, vs, f"{what} {k}")
        else:
            T.check_float32(name, x, o32[k], o64[k], f, vs, f"{what} {k}")


def run_once(c, dev):
    import drtk_amd.geometry as G
    import test_gpu_geometry as T

    t = inputs(c)
    what = f"run {c['run']}"
    on_device = dev != "cpu"
    dtype = DTYPES[c["dtype"]] if on_device else th.float64  # (on the CPU: the formulation in float64 against itself)
    if on_device:
        G.geometry_cache_clear()
    got = apply(c, t, dtype, dev)
    compare(got, c, t, dtype, what)
    if not on_device:
        return
    # a repeat from a cold cache, then from a warm one: the same bits
    G.geometry_cache_clear()
    for again in (apply(c, t, dtype, dev), apply(c, t, dtype, dev)):
        for k in got:
            assert th.equal(got[k], again[k]), f"{what} {k}: a repeat differs"
    # the C ABI, composed as the operators compose it: the same bits
    case = dict(t, face_info_outputs=tuple(k for k in KINDS if k in c["kinds"]))
    if c["topology"] == "NF3_expand":  # (the binding takes a contiguous list)
        case["vi"] = t["vi_shared"]
    binding = T._run_all_capi(case, dtype, dev)
    for k in got:
        if not k.endswith("_leaf"):
            assert binding[k].shape == got[k].shape and th.equal(binding[k], got[k]), f"{what} {k}: the Python API and the C ABI binding differ"


def run_case(c, check_guards=True, dev=DEV):
    for run in runs(c):
        run_once(run, dev)
    if check_guards and dev != "cpu":  # DRTK_CAPI_GUARD=g: nothing was written outside an output or a workspace (no-op otherwise)
        from drtk_amd import capi

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
