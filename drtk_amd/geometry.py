"""Mesh geometry of drtk.utils (drtk/utils/geometry.py, drtk/utils/indexing.py of the reference): face normals, areas
and edges, vertex normals, the per-face UV Jacobian and vertex binormals.

HIP tensors in float32 / float64 take the kernels of csrc/geometry.hip through the drtk_amd_ext operators: a face pass
and a vertex pass that sums through the cached vertex incidence of the index tensor -- two launches each way, plus a
chunk pass where a vertex is in more than 256 face corners -- bitwise reproducible (no float atomics).  Everything else -- CPU tensors, other dtypes -- takes the PyTorch formulation below.
Index tensors may be int32 or int64.

`cotangent_weights` and `mesh_laplacian` are this package's additions on the same passes: the mesh regulariser of a
geometry fit (INTEGRATION.md "Mesh regularisers"), which the reference leaves to a padded table built on the host.

Two differences from the reference on the HIP route:
- face_dpdt (and vert_binormals) of a face whose UV matrix is singular gives the non-finite result of the closed-form
  2x2 inverse where the reference raises (a kernel cannot raise without synchronising); the PyTorch formulation raises
  as the reference does.
- the backward passes are kernels, not differentiable graphs: double backward (create_graph=True through these
  functions) raises a RuntimeError instead of returning second-order terms; the PyTorch formulation supports it.
"""
from typing import Dict, List, Optional, Tuple, Union

import torch as th
import torch.nn.functional as thf

_KINDS = ("normals", "edges", "areas")


def _ops():
    from drtk_amd.utils import load_torch_ops

    load_torch_ops("drtk.rasterize_ext")
    return th.ops.drtk_amd_ext


def _hip(v: th.Tensor, *others: Optional[th.Tensor], idx: Tuple[th.Tensor, ...] = ()) -> bool:
    """The kernel route: HIP float32 / float64 tensors of one dtype and device, int32 / int64 indices."""
    if not (v.is_cuda and v.dtype in (th.float32, th.float64)):
        return False
    if any(o is not None and (o.device != v.device or o.dtype != v.dtype) for o in others):
        return False
    return all(i.device == v.device and i.dtype in (th.int32, th.int64) for i in idx)


# --- the PyTorch formulation (CPU tensors and other dtypes) -------------------------------------------------------


def _topology(vi: th.Tensor, n: int) -> th.Tensor:
    """[F,3] / [B,F,3] (B = 1 or n) -> int64 [n,F,3]"""
    if vi.dim() not in (2, 3):
        raise ValueError(f"Expected vi to be 2D [F, 3] or 3D [B, F, 3], got {vi.dim()}D")
    t = vi if vi.dim() == 3 else vi[None]
    return t.expand(n, -1, -1).long()


def _corners(x: th.Tensor, vi: th.Tensor) -> th.Tensor:
    """x [N,V,C], vi [F,3] / [B,F,3] -> the corner values [N,F,3,C]"""
    n, c = x.shape[0], x.shape[-1]
    t = _topology(vi, n)
    flat = t.reshape(n, 3 * t.shape[1], 1).expand(-1, -1, c)  # (sizes spelled out: n may be 0)
    return th.gather(x, 1, flat).view(n, t.shape[1], 3, c)


def _face_info_torch(v, vi, need):
    p = _corners(v, vi)
    p0, p1, p2 = p.unbind(2)
    e0, e1 = p1 - p0, p0 - p2
    out = {}
    if "normals" in need or "areas" in need:
        c = th.linalg.cross(e1, e0, dim=-1)
        length = th.linalg.vector_norm(c, dim=-1, keepdim=True)
        if "areas" in need:
            out["areas"] = 0.5 * length
        if "normals" in need:
            out["normals"] = c / length.clamp(min=1e-8)
    if "edges" in need:
        out["edges"] = th.stack([e0, e1, p2 - p1], dim=2)
    return out


def _face_attribute_to_vert_torch(v, vi, attr):
    n, a = v.shape[0], attr.shape[-1]
    t = _topology(vi, n)
    idx = t.reshape(n, -1, 1).expand(-1, -1, a)
    per_corner = attr.repeat_interleave(3, dim=1)  # [N, 3F, A], row f*3+k
    return th.zeros(n, v.shape[1], a, dtype=v.dtype, device=v.device).scatter_add(1, idx, per_corner)


def _face_dpdt_torch(v, vt, vi, vti):
    v012 = _corners(v, vi)
    t012 = _corners(vt, vti)
    dpdb = v012[:, :, 1:3] - v012[:, :, 0:1]
    dtdb = t012[:, :, 1:3] - t012[:, :, 0:1]
    return th.linalg.inv(dtdb) @ dpdb, v012


def _cotangent_weights_torch(v, vi):
    p = _corners(v, vi)  # [N,F,3,3]
    with th.no_grad():
        ok = th.linalg.vector_norm(th.linalg.cross(p[:, :, 0] - p[:, :, 2], p[:, :, 1] - p[:, :, 0], dim=-1), dim=-1) > 0
    # a face whose |c| > 0 is false is computed from zeros, so that neither its values nor its gradients meet a NaN
    p = th.where(ok[..., None, None], p, th.zeros_like(p))
    c = th.linalg.cross(p[:, :, 0] - p[:, :, 2], p[:, :, 1] - p[:, :, 0], dim=-1)
    two_nrm = 2 * th.where(ok, th.linalg.vector_norm(c, dim=-1), th.ones_like(ok, dtype=p.dtype))
    dots = ((p.roll(-1, 2) - p) * (p.roll(-2, 2) - p)).sum(-1)  # [N,F,3]: (p_{k+1} - p_k) . (p_{k+2} - p_k)
    return th.where(ok[..., None], dots / two_nrm[..., None], th.zeros_like(dots))


def _mesh_laplacian_torch(x, vi, weights):
    n, num_v, c = x.shape
    t = _topology(vi, n)
    xc = _corners(x, vi)  # [N,F,3,C]
    if weights is None:
        w = th.full((1, t.shape[1], 3), 0.5, dtype=x.dtype, device=x.device)
    else:
        w = weights if weights.dim() == 3 else weights[None]
    # per (face, corner k) the row of vertex a_k: w[k+1] (x[a_{k+2}] - x[a_k]) + w[k+2] (x[a_{k+1}] - x[a_k])
    rows = w.roll(-1, 2)[..., None] * (xc.roll(-2, 2) - xc) + w.roll(-2, 2)[..., None] * (xc.roll(-1, 2) - xc)
    idx = t.reshape(n, 3 * t.shape[1], 1).expand(-1, -1, c)
    return th.zeros(n, num_v, c, dtype=rows.dtype, device=x.device).scatter_add(1, idx, rows.reshape(n, 3 * t.shape[1], c))


# --- public API ---------------------------------------------------------------------------------------------------


@th.compiler.disable
def face_info(
    v: th.Tensor, vi: th.Tensor, to_compute: Optional[List[str]] = None
) -> Union[th.Tensor, Dict[str, th.Tensor]]:
    """Per-face normals [N,F,3], edges [N,F,3,3] and areas [N,F,1] of the faces `vi` ([F,3], [1,F,3] or [N,F,3]) of
    `v` [N,V,3]: with c = (p0 - p2) x (p1 - p0), normals = c / max(|c|, 1e-8), areas = |c| / 2, edges =
    (p1 - p0, p0 - p2, p2 - p1).  `to_compute`: any of "normals", "edges", "areas" (default all); one item returns
    the tensor, otherwise a dict.  Signature of drtk/utils/geometry.py face_info."""
    if to_compute is None:
        to_compute = ["normals", "edges", "areas"]
    need = set(to_compute)
    if _hip(v, idx=(vi,)) and need & set(_KINDS):
        normals, areas, edges = _ops().face_info(v, vi, "normals" in need, "areas" in need, "edges" in need)
        out = {k: t for k, t in (("areas", areas), ("normals", normals), ("edges", edges)) if k in need}
    else:
        out = _face_info_torch(v, vi, need)
    if len(to_compute) == 1:
        return out[to_compute[0]]
    return out


@th.compiler.disable
def face_attribute_to_vert(v: th.Tensor, vi: th.Tensor, attr: th.Tensor) -> th.Tensor:
    """Per-vertex sum [N,V,A] of the per-face attribute `attr` [N,F,A] over the (face, corner) pairs that list the
    vertex (a face that lists a vertex twice adds to it twice).  `v` [N,V,*] gives N, V, dtype and device; it gets no
    gradient.  `vi`: [F,3] or [B,F,3], B = 1 or N."""
    if _hip(v, attr, idx=(vi,)):
        return _ops().face_attribute_to_vert(v, vi, attr)
    return _face_attribute_to_vert_torch(v, vi, attr)


@th.compiler.disable
def vert_normals(v: th.Tensor, vi: th.Tensor, fnorms: Optional[th.Tensor] = None) -> th.Tensor:
    """Vertex normals [N,V,3]: F.normalize of the per-vertex sum of the face normals (face_info's, or `fnorms`
    [N,F,3] when given -- the gradient then goes to `fnorms` and `v` gets none).  Signature of
    drtk/utils/geometry.py vert_normals."""
    if _hip(v, fnorms, idx=(vi,)):
        return _ops().vert_normals(v, vi, fnorms)
    if fnorms is None:
        fnorms = _face_info_torch(v, vi, {"normals"})["normals"]
    return thf.normalize(_face_attribute_to_vert_torch(v, vi, fnorms), dim=-1)


def _dpdt_checks(v, vt):
    if v.ndim != 3:
        raise ValueError(f"Expected v to be 3D, got {v.ndim}D")
    if vt.ndim != 3:
        raise ValueError(f"Expected vt to be 3D, got {vt.ndim}D")
    if vt.shape[0] != v.shape[0]:
        raise ValueError(f"Expected vt to have the same batch size as v, got {vt.shape[0]} and {v.shape[0]}")


@th.compiler.disable
def face_dpdt(v: th.Tensor, vt: th.Tensor, vi: th.Tensor, vti: th.Tensor) -> Tuple[th.Tensor, th.Tensor]:
    """(dpdt_t [N,F,2,3], v012 [N,F,3,3]): the transposed Jacobian of positions wrt UVs per face,
    dpdt_t = inv([t1 - t0; t2 - t0]) @ [p1 - p0; p2 - p0], and the corner positions.  v [N,V,3], vt [N,T,2],
    vi and vti [F,3].  A singular UV matrix raises on the PyTorch route (as in the reference) and gives non-finite
    values on the HIP route.  Signature of drtk/utils/geometry.py face_dpdt."""
    _dpdt_checks(v, vt)
    if _hip(v, vt, idx=(vi, vti)):
        return _ops().face_dpdt(v, vt, vi, vti)
    return _face_dpdt_torch(v, vt, vi, vti)


@th.compiler.disable
def vert_binormals(v: th.Tensor, vt: th.Tensor, vi: th.Tensor, vti: th.Tensor) -> th.Tensor:
    """F.normalize of the per-vertex sum of the first row of face_dpdt's dpdt_t [N,V,3]; gradients go to `v` and
    `vt`.  Signature of drtk/utils/geometry.py vert_binormals."""
    _dpdt_checks(v, vt)
    if _hip(v, vt, idx=(vi, vti)):
        return _ops().vert_binormals(v, vt, vi, vti)
    dpdt_t, _ = _face_dpdt_torch(v, vt, vi, vti)
    return thf.normalize(_face_attribute_to_vert_torch(v, vi, dpdt_t[:, :, 0, :]), dim=-1)


@th.compiler.disable
def cotangent_weights(v: th.Tensor, vi: th.Tensor) -> th.Tensor:
    """Cotangent weights [N,F,3] of the faces `vi` ([F,3], [1,F,3] or [N,F,3]) of `v` [N,V,3]: with corners
    a0, a1, a2 = vi[f], w[n,f,k] = dot(p_{k+1} - p_k, p_{k+2} - p_k) / (2 |c|) = cot(angle at corner k) / 2, the weight
    of the edge opposite corner k (a_{k+1} -- a_{k+2}); c = (p0 - p2) x (p1 - p0) as in face_info.  Where |c| > 0 is
    false (duplicate or collinear corners, or a NaN) all three weights are exactly 0 and the face gives `v` no gradient.
    Differentiable with respect to `v`.  This package's addition (the reference has no such function)."""
    if _hip(v, idx=(vi,)):
        return _ops().cotangent_weights(v, vi)
    return _cotangent_weights_torch(v, vi)


@th.compiler.disable
def mesh_laplacian(x: th.Tensor, vi: th.Tensor, weights: Optional[th.Tensor] = None) -> th.Tensor:
    """The weighted graph Laplacian [N,V,C] of `x` [N,V,C] over the faces `vi` ([F,3], [1,F,3] or [N,F,3]):
    out[n,i] = sum_j w_ij (x[n,j] - x[n,i]) (negative semidefinite for non-negative weights), where the face weight
    `weights[f,k]` ([F,3], [1,F,3] or [N,F,3], e.g. `cotangent_weights`) belongs to the edge opposite corner k and an
    edge's w_ij is the sum over the faces that hold it.  `weights=None` is the uniform Laplacian: every face edge weighs
    1/2, so an interior manifold edge totals 1 and a boundary edge 1/2.  An unreferenced vertex gives 0; a face that lists
    a vertex twice adds a zero difference for that edge.  Differentiable with respect to `x` and `weights`.  This
    package's addition (the reference has no such function)."""
    if _hip(x, weights, idx=(vi,)):
        return _ops().mesh_laplacian(x, vi, weights)
    return _mesh_laplacian_torch(x, vi, weights)


def index(x: th.Tensor, idxs: th.Tensor, dim: int) -> th.Tensor:
    """x indexed along `dim` by `idxs`, that dimension replaced by the shape of `idxs` (drtk/utils/indexing.py)."""
    return x.index_select(dim, idxs.reshape(-1)).reshape(*x.shape[:dim], *idxs.shape, *x.shape[dim + 1:])


def geometry_cache_stats() -> Tuple[int, int, int]:
    """(hits, misses, entries) of the vertex-incidence cache of the HIP route."""
    return tuple(_ops().geometry_cache_stats())


def geometry_cache_clear() -> None:
    _ops().geometry_cache_clear()
