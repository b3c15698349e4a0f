"""Closest-point queries and the chamfer distance: the data term of registration to a scan, a depth-sensor cloud or another
mesh (this package's addition; the reference has no such function).

HIP tensors in float32 / float64 take the kernels of csrc/nearest.hip through `drtk_amd_ext::nearest_points`: a brute-force
tiled all-pairs search (no `N*P*M` intermediate), one streaming launch for the gradient to the queries and, for the
gradient to the targets, a device-side stable sort of the indices followed by a chunk pass and a target pass -- fixed
summation order, double accumulation, no float atomics, no host read, bitwise reproducible.  Everything else -- CPU tensors,
other dtypes -- takes the chunked PyTorch formulation below, which evaluates the same expression and so has the same bits.

The squared distance is `((px-qx)*(px-qx) + (py-qy)*(py-qy)) + (pz-qz)*(pz-qz)`, each operation rounded in the tensors'
dtype; the `|p|^2 + |q|^2 - 2 p.q` (GEMM) form is not used: it cancels catastrophically exactly when a fit has converged.

On the HIP route the backward passes are kernels, not differentiable graphs: double backward (create_graph=True) raises a
RuntimeError; the PyTorch formulation supports it.

Not covered: K > 1 neighbours, ragged per-view point counts, point-to-triangle and point-to-plane distances, a
normal-consistency term, grid or tree acceleration, a fused chamfer reduction kernel, float16.
"""
from typing import Optional, Tuple

import torch as th

from drtk_amd.geometry import _hip, _ops

_PAIRS_PER_CHUNK = 1 << 22  # the PyTorch formulation holds this many distances at a time


def _check_points(x, name):
    if x.dim() not in (2, 3) or x.shape[-1] != 3:
        raise ValueError(f"nearest_points(): expected {name} of shape [N, P, 3], [1, P, 3] or [P, 3], got {tuple(x.shape)}")
    return x.shape[0] if x.dim() == 3 else 1


def _check_args(p, q):
    pb, qb = _check_points(p, "p"), _check_points(q, "q")
    if q.dtype != p.dtype:
        raise TypeError(f"nearest_points(): expected q to have the dtype of p, got {q.dtype} for {p.dtype}")
    if not p.dtype.is_floating_point:
        raise TypeError(f"nearest_points(): expected floating-point points, got {p.dtype}")
    if q.device != p.device:
        raise ValueError("nearest_points(): expected q on the device of p")
    n = qb if pb == 1 else pb
    if pb not in (1, n) or qb not in (1, n):
        raise ValueError(f"nearest_points(): expected the batch sizes of p and q to be equal or 1, got {pb} and {qb}")
    return n


def _d2(p, q):
    """The defined expression on broadcasting [...,3] tensors"""
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _nearest_torch(p, q, n):
    """Chunks of queries against all targets; the index search runs without autograd, the distance is then formed again from
    the chosen target, differentiably, with the same expression (the same bits)."""
    pp = (p if p.dim() == 3 else p[None]).expand(n, -1, -1)
    qq = (q if q.dim() == 3 else q[None]).expand(n, -1, -1)
    num_p, num_q = pp.shape[1], qq.shape[1]
    inf = float("inf")
    idx = th.full((n, num_p), -1, dtype=th.int64, device=p.device)
    if num_q > 0 and n * num_p > 0:
        step = max(1, _PAIRS_PER_CHUNK // (n * num_q))
        with th.no_grad():
            for i0 in range(0, num_p, step):
                d = _d2(pp[:, i0:i0 + step, None, :], qq[:, None, :, :])
                d = th.where(d < inf, d, th.full_like(d, inf))  # NaN and +inf are no candidates
                best, j = d.min(-1)  # the first of equal minima
                idx[:, i0:i0 + step] = th.where(best < inf, j, th.full_like(j, -1))
    valid = idx >= 0
    if num_q > 0:
        chosen = th.gather(qq, 1, idx.clamp(min=0)[..., None].expand(-1, -1, 3))
    else:
        chosen = pp * 0
    # rows without a candidate take no part in the graph: their gradient is exactly 0, not 0 * NaN
    mask = valid[..., None]
    zero = th.zeros((), dtype=p.dtype, device=p.device)
    d = _d2(th.where(mask, pp, zero), th.where(mask, chosen, zero))
    return th.where(valid, d, th.full_like(d, inf)), idx


@th.compiler.disable
def nearest_points(p: th.Tensor, q: th.Tensor) -> Tuple[th.Tensor, th.Tensor]:
    """For every query point the nearest target: `(dist2 [N,P], idx [N,P] int64)`.

    `p`: the queries, [N,P,3], [1,P,3] or [P,3]; `q`: the targets, [N,M,3], [1,M,3] or [M,3]; float32 or float64, one dtype
    and device.  N is the larger batch; a batch of 1 (or a stride-0 expand) is shared by the views, read as one row, and gets
    the sum over the views as its gradient.  On the HIP route strided inputs are read in place where a point is three
    consecutive elements (a `[..., :3]` slice of an [N,P,4] or [N,P,6] positions-plus-normals tensor, a slice of views).

    `d2(i,j) = ((px-qx)*(px-qx) + (py-qy)*(py-qy)) + (pz-qz)*(pz-qz)`, every operation rounded in the dtype, no FMA.
    `idx[n,i]` is the LOWEST j whose d2 is minimal among the candidates with d2 < +inf, `dist2[n,i]` that d2.  A candidate
    whose d2 is NaN or +inf (a NaN coordinate, an overflowing square) is never chosen; with no candidate (M = 0, a NaN query)
    idx = -1 and dist2 = +inf.

    `dist2` is differentiable in `p` and `q` with `idx` held constant: grad_p[n,i] = 2 g (p_i - q_idx), grad_q[n,j] = minus
    the sum of that over the queries that chose j; rows with idx = -1 contribute exactly 0, a target nobody chose gets
    exactly 0, and only the requested gradients run.  `idx` is not differentiable.  The op is graph-capturable.

    Not covered: K > 1 neighbours, ragged per-view point counts, point-to-triangle / point-to-plane distances, spatial
    acceleration structures, float16."""
    n = _check_args(p, q)
    if _hip(p, q):
        return _ops().nearest_points(p, q)
    return _nearest_torch(p, q, n)


def _chamfer_term(d2, idx, weights, squared, name):
    valid = idx >= 0
    if squared:
        d = th.where(valid, d2, th.zeros_like(d2))
    else:  # sqrt(0) has no finite derivative: coincident points take the subgradient 0
        pos = valid & (d2 > 0)
        d = th.where(pos, th.where(pos, d2, th.ones_like(d2)).sqrt(), th.zeros_like(d2))
    w = valid.to(d2.dtype)
    if weights is not None:
        if weights.dim() == 1:
            weights = weights[None]
        if weights.dim() != 2 or weights.shape[1] != d2.shape[1] or weights.shape[0] not in (1, d2.shape[0]):
            raise ValueError(f"chamfer_distance(): expected {name} of shape {tuple(d2.shape)}, got {tuple(weights.shape)}")
        w = w * weights.to(d2.dtype)
    total = w.sum(1)
    # a row without weight gives 0, not 0 / 0, and needs no read-back
    return (w * d).sum(1) / th.where(total != 0, total, th.ones_like(total))


def chamfer_distance(x: th.Tensor, y: th.Tensor, x_weights: Optional[th.Tensor] = None, y_weights: Optional[th.Tensor] = None,
                     bidirectional: bool = True, squared: bool = True) -> th.Tensor:
    """The chamfer distance of two point sets, a scalar: the mean over the views of
    `mean_i d(x_i, Y) + mean_j d(y_j, X)` (the first term alone with `bidirectional=False`), d the squared distance to the
    nearest point of the other set, or the distance itself with `squared=False`.

    `x` [N,P,3] / [1,P,3] / [P,3] and `y` [N,M,3] / [1,M,3] / [M,3] as for `nearest_points`, of which this is a thin
    composition (two calls, no kernel of its own).  `x_weights` [N,P] and `y_weights` [N,M] (float or bool; a batch of 1
    is shared) turn the means into weighted means; a view whose weights are all zero contributes 0, not NaN.  A point
    without a nearest neighbour (idx = -1: NaN coordinates, an empty other set) counts as weight 0.

    Not covered: a normal-consistency term, point-to-triangle distances, ragged per-view point counts, a fused reduction."""
    d2, idx = nearest_points(x, y)
    per_view = _chamfer_term(d2, idx, x_weights, squared, "x_weights")
    if bidirectional:
        d2, idx = nearest_points(y, x)
        per_view = per_view + _chamfer_term(d2, idx, y_weights, squared, "y_weights")
    return per_view.sum() / max(per_view.shape[0], 1)
