"""Linear blend skinning: the step from rig parameters to geometry (this package's addition; the reference has no such
function).

HIP tensors in float32 / float64 take the kernels of csrc/skin.hip through `drtk_amd_ext::skin`: one launch forward; backward
one launch for the gradients to the rest pose and the weights and two (a chunk pass and a tiny sum) for the gradient to
the joint transforms, which is a many-to-few reduction through the cached joint incidence of `joint_idx` -- fixed
summation order, double accumulation, no float atomics, bitwise reproducible.  Everything else -- CPU tensors, other
dtypes -- takes the PyTorch gather formulation below.  Index tensors may be int32 or int64.

On the HIP route the backward passes are kernels, not differentiable graphs: double backward (create_graph=True) raises a
RuntimeError; the PyTorch formulation supports it.
"""
from typing import Tuple

import torch as th

from drtk_amd.geometry import _hip, _ops

MAX_SLOTS = 8  # DRTK_SKIN_MAX_SLOTS of include/drtk_amd.h


def _check_args(v, joint_idx, joint_weights, transforms):
    if v.dim() not in (2, 3) or v.shape[-1] != 3:
        raise ValueError(f"skin(): expected v of shape [N, V, 3], [1, V, 3] or [V, 3], got {tuple(v.shape)}")
    if transforms.dim() != 4 or transforms.shape[2] not in (3, 4) or transforms.shape[3] != 4:
        raise ValueError(f"skin(): expected transforms of shape [N, J, 3, 4] or [N, J, 4, 4], got {tuple(transforms.shape)}")
    n, num_v = transforms.shape[0], v.shape[-2]
    if v.dim() == 3 and v.shape[0] not in (1, n):
        raise ValueError(f"skin(): expected the batch size of v to be 1 or {n}, got {v.shape[0]}")
    if joint_idx.dim() != 2 or joint_idx.shape[0] != num_v:
        raise ValueError(f"skin(): expected joint_idx of shape [V, K] with V = {num_v}, got {tuple(joint_idx.shape)}")
    if not 1 <= joint_idx.shape[1] <= MAX_SLOTS:
        raise ValueError(f"skin(): expected 1 <= K <= {MAX_SLOTS} slots per vertex, got K = {joint_idx.shape[1]}")
    if joint_idx.dtype not in (th.int32, th.int64):
        raise TypeError(f"skin(): expected joint_idx to be int32 or int64, got {joint_idx.dtype}")
    if joint_weights.shape != joint_idx.shape:
        raise ValueError(f"skin(): expected joint_weights of the shape of joint_idx, got {tuple(joint_weights.shape)}")
    if joint_weights.dtype != v.dtype or transforms.dtype != v.dtype:
        raise TypeError(f"skin(): expected joint_weights and transforms to have the dtype of v, got {joint_weights.dtype} "
                        f"and {transforms.dtype} for {v.dtype}")
    if not (joint_idx.device == joint_weights.device == transforms.device == v.device):
        raise ValueError("skin(): expected joint_idx, joint_weights and transforms on the device of v")


def _skin_torch(v, joint_idx, joint_weights, transforms):
    """The gather formulation: T[:, idx] of shape [N,V,K,3,4], blended over the slots, applied."""
    n, num_j = transforms.shape[0], transforms.shape[1]
    if joint_idx.numel() and (int(joint_idx.min()) < -1 or int(joint_idx.max()) >= num_j):
        raise ValueError(f"skin(): joint_idx contains a joint index outside [-1, {num_j})")
    vv = (v if v.dim() == 3 else v[None]).expand(n, -1, -1)
    valid = joint_idx >= 0
    j = joint_idx.clamp(min=0).long()
    w = th.where(valid, joint_weights, th.zeros_like(joint_weights))  # an empty slot: its weight is not used, gradient 0
    if num_j == 0:
        return th.zeros(n, vv.shape[1], 3, dtype=v.dtype, device=v.device) + 0 * (vv + w.sum(-1)[None, :, None])
    m = (w[None, :, :, None, None] * transforms[:, :, :3, :][:, j]).sum(2)  # [N,V,3,4]
    return (m[..., :3] * vv[..., None, :]).sum(-1) + m[..., 3]


@th.compiler.disable
def skin(v: th.Tensor, joint_idx: th.Tensor, joint_weights: th.Tensor, transforms: th.Tensor) -> th.Tensor:
    """Linear blend skinning: the posed vertices [N,V,3],
    out[n,i] = sum over the slots k with joint_idx[i,k] >= 0 of joint_weights[i,k] * (R[n,j] v[n,i] + t[n,j]),
    j = joint_idx[i,k], [R|t] = rows 0..2 of transforms[n,j].

    `v`: the rest pose, [N,V,3], [1,V,3] or [V,3] (a stride-0 expand counts as shared and is read as one row), float32 or
    float64.  `joint_idx`: [V,K], int32 or int64, 1 <= K <= 8, entries in [-1, J); -1 is an empty slot: it adds nothing, its
    weight is not read and gets gradient 0; a joint may sit in two slots of one vertex, the contributions add.
    `joint_weights`: [V,K] in the dtype of `v`, used as given (not normalised).  `transforms`: the skinning matrices (posed
    joint times inverse bind), [N,J,3,4] or [N,J,4,4] in the dtype of `v`; only rows 0..2 are read (a `[..., :3, :]` view of a
    4x4 tensor is read in place) and N is taken from here.  A vertex whose slots are all empty gives exactly 0.

    Differentiable with respect to `v`, `joint_weights` and `transforms` (row 3 of a 4x4 input and a joint that no vertex
    names get exactly 0); only the requested gradients run.  On the HIP route an index outside [-1, J) raises from the
    one host read per index tensor, and the op is graph-capturable once that tensor's joint incidence is cached (run it
    once before the capture)."""
    _check_args(v, joint_idx, joint_weights, transforms)
    if _hip(v, joint_weights, transforms, idx=(joint_idx,)):
        return _ops().skin(v, joint_idx, joint_weights, transforms)
    return _skin_torch(v, joint_idx, joint_weights, transforms)


def sparse_skin_weights(dense: th.Tensor, k: int = 4, renormalize: bool = True) -> Tuple[th.Tensor, th.Tensor]:
    """(joint_idx int64 [V,k], joint_weights [V,k]) of a dense skinning matrix `dense` [V,J]: per vertex the k largest
    weights by magnitude (`topk`), in that order; slots whose weight is 0 get index -1.  `renormalize` divides each
    row by the sum of what it keeps (rows that keep nothing stay 0).  With k >= the non-zeros of every row the pair
    reproduces the dense matrix.  Plain PyTorch; most rigs ship a dense matrix."""
    if dense.dim() != 2:
        raise ValueError(f"sparse_skin_weights(): expected dense of shape [V, J], got {tuple(dense.shape)}")
    if not 1 <= k <= MAX_SLOTS:
        raise ValueError(f"sparse_skin_weights(): expected 1 <= k <= {MAX_SLOTS}, got {k}")
    kk = min(k, dense.shape[1])
    _, idx = th.topk(dense.abs(), kk, dim=1)
    w = th.gather(dense, 1, idx)
    if kk < k:
        idx = th.cat([idx, idx.new_zeros(dense.shape[0], k - kk)], 1)
        w = th.cat([w, w.new_zeros(dense.shape[0], k - kk)], 1)
    if renormalize:
        s = w.sum(1, keepdim=True)
        w = th.where(s != 0, w / th.where(s != 0, s, th.ones_like(s)), w)
    idx = th.where(w != 0, idx, th.full_like(idx, -1))
    return idx, w


def joint_incidence(joint_idx: th.Tensor, num_joints: int) -> Tuple[th.Tensor, th.Tensor]:
    """(crow [J+1], entries) of the cached joint incidence of a HIP `joint_idx` [V,K]: joint j's slots i*K+k, ascending, are
    entries[crow[j]:crow[j+1]].  Builds and caches it (one host read); a captured step needs it cached beforehand."""
    return _ops().joint_incidence(joint_idx, num_joints)


def skin_cache_stats() -> Tuple[int, int, int]:
    """(hits, misses, entries) of the joint-incidence cache of the HIP route."""
    return tuple(_ops().skin_cache_stats())


def skin_cache_clear() -> None:
    _ops().skin_cache_clear()
