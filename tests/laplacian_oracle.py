"""TEST INFRASTRUCTURE -- an oracle for drtk_amd.cotangent_weights and drtk_amd.mesh_laplacian written from the maths, not
from the package: cotangents as 1 / tan(arccos(.)) of the corner angles, the Laplacian as a dense V x V matrix per view,
gradients by autograd.  It runs in the dtype of its inputs (float64 for the reference value, float32 for the float32
oracle of tests/f64_distance.py).

Conventions (the issue's): face f has corners a0, a1, a2 = vi[f]; weight [f,k] belongs to the edge opposite corner k,
a_{k+1} -- a_{k+2}; L x = sum_j w_ij (x_j - x_i); a face whose c = (p0 - p2) x (p1 - p0) does not satisfy |c| > 0 has
three zero weights and gives the vertices no gradient."""
import numpy as np
import torch as th


def views(t, n):
    """[F,3] / [1,F,3] / [N,F,3] (indices or weights) -> [n,F,3]"""
    t = t if t.dim() == 3 else t[None]
    assert t.shape[0] in (1, n)
    return t.expand(n, -1, -1)


def cot_weights(v, vi):
    """v [N,V,3], vi [F,3] / [B,F,3] -> [N,F,3]"""
    n = v.shape[0]
    t = views(vi.long(), n)
    p = th.stack([v[i][t[i]] for i in range(n)])  # [N,F,3,3]
    with th.no_grad():
        ok = th.linalg.cross(p[:, :, 0] - p[:, :, 2], p[:, :, 1] - p[:, :, 0], dim=-1).norm(dim=-1) > 0
    # a degenerate face is replaced by a fixed proper triangle before any angle is taken (arccos and the edge lengths are
    # not differentiable on it), and its weights by 0 afterwards
    proper = th.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=v.dtype, device=v.device)
    p = th.where(ok[..., None, None], p, proper)
    out = []
    for k in range(3):
        e1, e2 = p[:, :, (k + 1) % 3] - p[:, :, k], p[:, :, (k + 2) % 3] - p[:, :, k]
        angle = th.arccos((e1 * e2).sum(-1) / (e1.norm(dim=-1) * e2.norm(dim=-1)))
        out.append(0.5 / th.tan(angle))
    return th.where(ok[..., None], th.stack(out, -1), th.zeros((), dtype=v.dtype, device=v.device))


def laplacian_matrix(vi, w, num_vertices):
    """vi [F,3] int64, w [F,3] -> dense [V,V]: w[f,k] on (a_{k+1}, a_{k+2}) and its transpose, minus both on the diagonal"""
    V = num_vertices
    L = th.zeros(V * V, dtype=w.dtype, device=w.device)
    for k in range(3):
        i, j = vi[:, (k + 1) % 3], vi[:, (k + 2) % 3]
        for rows, cols, sign in ((i, j, 1.0), (j, i, 1.0), (i, i, -1.0), (j, j, -1.0)):
            L = L.index_add(0, rows * V + cols, sign * w[:, k])
    return L.view(V, V)


def mesh_laplacian(x, vi, weights=None):
    """x [N,V,C], vi [F,3] / [B,F,3], weights None (every face edge 1/2) / [F,3] / [B,F,3] -> [N,V,C]"""
    n, V = x.shape[0], x.shape[1]
    t = views(vi.long(), n)
    if weights is None:
        weights = th.full((1, t.shape[1], 3), 0.5, dtype=x.dtype, device=x.device)
    w = views(weights, n)
    return th.stack([laplacian_matrix(t[i], w[i], V) @ x[i] for i in range(n)])


def accumulated(x, vi, weights=None):
    """sum_j |w_ij| |x_j| (the diagonal included) per element: what was summed into it, in magnitude"""
    n, V = x.shape[0], x.shape[1]
    t = views(vi.long(), n)
    if weights is None:
        weights = th.full((1, t.shape[1], 3), 0.5, dtype=x.dtype, device=x.device)
    w = views(weights, n)
    return th.stack([laplacian_matrix(t[i], w[i], V).abs() @ x[i].abs() for i in range(n)])


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def grid_mesh(rows, cols, seed, jitter=0.2):
    """A jittered rows x cols vertex grid, two triangles per cell: (v [V,3] float64, vi [F,3] int64)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    v = np.stack([xx, yy, np.zeros_like(xx)], -1).reshape(-1, 3) + jitter * rng.uniform(-1, 1, (rows * cols, 3))
    idx = np.arange(rows * cols).reshape(rows, cols)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    vi = np.concatenate([np.stack([a, b, c], -1), np.stack([b, d, c], -1)])
    return th.from_numpy(v), th.from_numpy(vi.astype(np.int64))


def fan_mesh(valence):
    """Vertex 0 in `valence` faces (0, r_k, r_{k+1}) whose other corners wind around the unit sphere half a radian at a
    time -- a fan in topology only, so that every triangle is well shaped however long the row of vertex 0 is (a flat fan
    of valence 600 has corner angles of 0.01, where arccos, and with it this oracle, loses four digits):
    (v [valence+1,3] float64, vi [valence,3] int64)"""
    k = th.arange(valence, dtype=th.float64)
    z = -0.8 + 1.6 * k / max(valence - 1, 1)
    s = th.sqrt(1 - z * z)
    ring = th.stack([s * th.cos(0.5 * k), s * th.sin(0.5 * k), z], -1)
    v = th.cat([th.tensor([[0.05, -0.02, 0.03]], dtype=th.float64), ring])
    j = th.arange(valence)
    vi = th.stack([th.zeros(valence, dtype=th.long), 1 + j, 1 + (j + 1) % valence], -1)
    return v, vi


def soup_mesh(num_vertices, num_faces, seed):
    """Random points in a cube and random faces on three distinct vertices (any topology is a graph to the Laplacian) whose
    corner angles all exceed 0.4: a sliver's cotangent is where arccos, and with it this oracle, loses its digits"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (num_vertices, 3))
    faces = []
    while len(faces) < num_faces:
        f = rng.permutation(num_vertices)[:3]
        p = v[f]
        cos = [np.dot(p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]) / (np.linalg.norm(p[(k + 1) % 3] - p[k]) * np.linalg.norm(p[(k + 2) % 3] - p[k])) for k in range(3)]
        if max(cos) < np.cos(0.4):
            faces.append(f)
    return th.from_numpy(v), th.from_numpy(np.stack(faces).astype(np.int64))


def sphere_mesh(segments, rings):
    """A latitude-longitude sphere with one vertex per pole: V = 2 + (rings - 1) * segments, no degenerate face"""
    lat = np.pi * np.arange(1, rings) / rings
    lon = 2 * np.pi * np.arange(segments) / segments
    body = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)),
                     np.outer(np.cos(lat), np.ones(segments))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], body, [[0.0, 0.0, -1.0]]])
    idx = 1 + np.arange((rings - 1) * segments).reshape(rings - 1, segments)
    nxt = np.roll(idx, -1, 1)
    south = v.shape[0] - 1
    faces = [np.stack([np.zeros(segments, np.int64), idx[0], nxt[0]], -1),
             np.stack([np.full(segments, south), nxt[-1], idx[-1]], -1)]
    a, b, c, d = idx[:-1].ravel(), nxt[:-1].ravel(), idx[1:].ravel(), nxt[1:].ravel()
    faces += [np.stack([a, c, b], -1), np.stack([b, c, d], -1)]
    return th.from_numpy(v), th.from_numpy(np.concatenate(faces).astype(np.int64))


def with_degenerates(v, vi):
    """Adds an unreferenced vertex, a duplicate-corner face on existing vertices and a collinear face on three new vertices
    with integer coordinates (c is exactly 0 in any precision)."""
    V = v.shape[0]
    extra = th.tensor([[0.0, 0.0, 9.0], [10.0, 0.0, 0.0], [12.0, 0.0, 0.0], [13.0, 0.0, 0.0]], dtype=v.dtype)
    faces = th.tensor([[1, 1, 0], [V + 1, V + 2, V + 3]], dtype=vi.dtype)
    return th.cat([v, extra]), th.cat([vi, faces])


# ---- the structural cases of the HIP route ---------------------------------------------------------------------------------
# name: (mesh, views N, channels C, per-view topology).  The smallest shapes at which the kernels can still go wrong: one
# face; 257 faces and vertices (one past a block of 256 lanes); every channel count around the group of four; a vertex in
# 300 and in 600 faces (one and two full chunks of 256 (face, corner) entries plus a tail), the topology shared by the
# views and one per view; an unreferenced vertex, a duplicate-corner face and a collinear face.
CASES = {
    "one_face": ("one", 1, 1, False),
    "soup257_c1_n1": ("soup", 1, 1, False),
    "soup257_c3_n3": ("soup", 3, 3, False),
    "soup257_c4_n1": ("soup", 1, 4, False),
    "soup257_c5_n3": ("soup", 3, 5, True),
    "degenerate_shared": ("degenerate", 3, 3, False),
    "degenerate_per_view": ("degenerate", 3, 5, True),
    "fan300_shared": ("fan300", 2, 3, False),
    "fan300_per_view": ("fan300", 2, 5, True),
    "fan600_shared": ("fan600", 2, 5, False),
    "fan600_per_view": ("fan600", 2, 3, True),
}


def case(name):
    """(v [N,V,3], x [N,V,C], g [N,V,C] float64, vi int64 [F,3] or [N,F,3]); the views' vertices differ, and a per-view
    topology lists the same faces in another order and from another corner (degenerate faces stay last)"""
    mesh, n, c, per_view = CASES[name]
    if mesh == "one":
        v0, vi = th.tensor([[0.1, 0.0, 0.2], [1.0, 0.2, 0.0], [0.3, 0.9, 0.1]], dtype=th.float64), th.tensor([[0, 1, 2]])
    elif mesh == "soup":
        v0, vi = soup_mesh(257, 257, 3)
    elif mesh == "degenerate":
        v0, vi = with_degenerates(*grid_mesh(5, 7, 4))
    else:
        v0, vi = fan_mesh(int(mesh[3:]))
    return build_case(v0, vi, n, c, per_view, sum(map(ord, name)), degenerate=mesh == "degenerate")


def build_case(v0, vi, n, c, per_view, seed, degenerate=False):
    """`case` for any mesh (v0 [V,3] float64, vi [F,3] int64), n views, c channels, drawn from a generator seeded with `seed`;
    `degenerate`: the mesh went through with_degenerates (tests/fuzz_added_ops.py draws its own meshes)."""
    keep_last = 2 if degenerate else 0
    g = th.Generator().manual_seed(seed)
    v = v0[None] * (1 + 0.1 * th.arange(n, dtype=th.float64))[:, None, None] + 0.02 * th.randn(n, *v0.shape, dtype=th.float64, generator=g)
    if degenerate:
        v[:, -3:] = v0[-3:]  # the collinear face keeps its integer coordinates
    x = th.randn(n, v0.shape[0], c, dtype=th.float64, generator=g)
    grad = th.randn(n, v0.shape[0], c, dtype=th.float64, generator=g)
    if per_view:
        k = vi.shape[0] - keep_last
        vi = th.stack([th.cat([vi[:k].roll(i, 0).roll(i, 1), vi[k:]]) for i in range(n)])
    return v, x, grad, vi


def pipeline(cot, lap, v, x, grad, vi):
    """The four results every parity check compares -- {weights, out, grad_x, grad_w, grad_v} of
    out = lap(x, vi, cot(v, vi)) under the upstream gradient `grad` -- from any pair of implementations."""
    vv, xx = v.clone().requires_grad_(True), x.clone().requires_grad_(True)
    w = cot(vv, vi)
    w.retain_grad()
    out = lap(xx, vi, w)
    out.backward(grad)
    return {"weights": w.detach(), "out": out.detach(), "grad_x": xx.grad, "grad_w": w.grad, "grad_v": vv.grad}


def reference(v, x, grad, vi, dtype):
    """pipeline() of this oracle in `dtype` on the CPU"""
    return pipeline(cot_weights, mesh_laplacian, v.cpu().to(dtype), x.cpu().to(dtype), grad.cpu().to(dtype), vi.cpu())
