"""TEST INFRASTRUCTURE -- an oracle for drtk_amd.skin that shares nothing with the package's gather formulation: the slots
are scattered into a DENSE [V,J] weight matrix (index_put with accumulation, so that a joint named twice adds and an empty
slot adds nothing), the per-vertex 3x4 matrices are one einsum of that matrix with the transforms, they are applied with a
second einsum, and every gradient is autograd's.  It runs in the dtype it is given.

CASES are the smallest shapes at which the kernels of csrc/skin.hip can go wrong (the chunk length of the joint backward
and the forward's LDS staging limit are read from the source); build_case(seed) draws random shapes for the fuzz rows."""
import os
import re

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    src = open(os.path.join(ROOT, "drtk_amd", "csrc", "skin.hip")).read()
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert m, f"csrc/skin.hip no longer defines {name}"
    return int(m.group(1))


CHUNK = _constant("kSkinChunk")
LDS_JOINTS = _constant("kSkinLdsJoints")


def skin(v, joint_idx, joint_weights, transforms):
    """v [N,V,3] / [1,V,3] / [V,3], joint_idx [V,K] (-1: empty), joint_weights [V,K], transforms [N,J,3|4,4] -> [N,V,3]"""
    n, num_j = transforms.shape[0], transforms.shape[1]
    num_v, k = joint_idx.shape
    rows = th.arange(num_v, device=joint_idx.device)[:, None].expand(num_v, k)
    valid = joint_idx >= 0
    dense = th.zeros(num_v, num_j, dtype=joint_weights.dtype, device=joint_weights.device)
    dense = dense.index_put((rows[valid], joint_idx[valid].long()), joint_weights[valid], accumulate=True)
    m = th.einsum("vj,njab->nvab", dense, transforms[:, :, :3, :])
    vv = (v if v.dim() == 3 else v[None]).expand(n, -1, -1)
    return th.einsum("nvab,nvb->nva", m[..., :3], vv) + m[..., 3]


def results(fn, v, joint_idx, joint_weights, transforms, grad, dtype, device="cpu"):
    """{"out", "grad_v", "grad_w", "grad_t"} of `fn` (this oracle, or the package) on copies of the inputs in `dtype` on
    `device`; the gradients have the shapes of the inputs as given (a stride-0 expand of v is rebuilt on the device)."""
    expanded = v.dim() == 3 and v.shape[0] > 1 and v.stride(0) == 0
    leaf = (v[:1] if expanded else v).to(dtype).to(device).clone().requires_grad_(True)
    vv = leaf.expand(v.shape[0], -1, -1) if expanded else leaf
    w = joint_weights.to(dtype).to(device).clone().requires_grad_(True)
    if transforms.is_contiguous():
        t_leaf = transforms.to(dtype).to(device).clone().requires_grad_(True)
        t = t_leaf
    else:  # a [..., :3, :] view of a 4x4 tensor: the leaf is the 4x4 tensor
        base = transforms._base
        assert base is not None and base.shape[-2:] == (4, 4) and transforms.shape[-2:] == (3, 4)
        t_leaf = base.to(dtype).to(device).clone().requires_grad_(True)
        t = t_leaf[..., :3, :]
        assert not t.is_contiguous() or t.numel() == 0
    out = fn(vv, joint_idx.to(device), w, t)
    gv, gw, gt = th.autograd.grad(out, (leaf, w, t_leaf), grad.to(dtype).to(device), allow_unused=True)
    zero = lambda g, like: th.zeros_like(like) if g is None else g  # noqa: E731
    return {"out": out.detach().cpu(), "grad_v": zero(gv, leaf).cpu(), "grad_w": zero(gw, w).cpu(), "grad_t": zero(gt, t_leaf).cpu()}


def _inputs(gen, n, num_v, num_j, k, v_batch, idx=None, mat4=False, empty_prob=0.0):
    """Random inputs in float64 that are exact in float32 (one set of inputs for either precision)."""
    r = lambda *s: th.randn(*s, dtype=th.float64, generator=gen).float().double()  # noqa: E731
    v = r(*v_batch, num_v, 3)
    if idx is None:
        idx = th.randint(0, max(num_j, 1), (num_v, k), generator=gen)
        if empty_prob > 0:
            idx[th.rand(num_v, k, generator=gen) < empty_prob] = -1
    w = (th.rand(num_v, k, dtype=th.float64, generator=gen) + 0.1).float().double()
    t = r(n, num_j, 4 if mat4 else 3, 4)
    if mat4:
        t[:, :, 3] = th.tensor([0.0, 0.0, 0.0, 1.0], dtype=th.float64)
    grad = r(n, num_v, 3)
    return v, idx, w, t, grad


def _chunked_idx(gen):
    """K = 2; joint 0: exactly one chunk, joint 1: a chunk plus one entry, joint 2: two chunks plus 37, joint 3: nobody,
    joint 4: the rest -- the slots shuffled over the vertices."""
    counts = {0: CHUNK, 1: CHUNK + 1, 2: 2 * CHUNK + 37}
    flat = th.cat([th.full((c,), j) for j, c in counts.items()])
    total = flat.numel() + 60
    total += total % 2
    flat = th.cat([flat, th.full((total - flat.numel(),), 4)])
    return flat[th.randperm(total, generator=gen)].view(total // 2, 2)


def _k8_idx(gen, num_v, num_j):
    idx = th.randint(0, num_j, (num_v, 8), generator=gen)
    idx[th.rand(num_v, 8, generator=gen) < 0.4] = -1
    idx[3] = -1                      # every slot empty
    idx[5, 1], idx[5, 6] = 2, 2      # one joint in two slots
    idx[6] = th.tensor([-1, 1, -1, 1, 0, -1, -1, 1])
    return idx


def _case(name):
    gen = th.Generator().manual_seed(sum(map(ord, name)))
    if name == "tiny":
        return _inputs(gen, 1, 5, 2, 1, (1,))
    if name == "block_edge":
        return _inputs(gen, 3, 257, 3, 4, (3,))
    if name == "shared_v":
        return _inputs(gen, 3, 130, 6, 3, (1,), empty_prob=0.2)
    if name == "shared_v_expand":
        v, idx, w, t, grad = _inputs(gen, 3, 130, 6, 3, (1,), empty_prob=0.2)
        return v.expand(3, -1, -1), idx, w, t, grad
    if name == "shared_v_2d":
        v, idx, w, t, grad = _inputs(gen, 2, 70, 4, 2, (1,))
        return v[0], idx, w, t, grad
    if name == "k8_slots":
        return _inputs(gen, 2, 90, 5, 8, (2,), idx=_k8_idx(gen, 90, 5))
    if name == "chunked":
        idx = _chunked_idx(gen)
        return _inputs(gen, 2, idx.shape[0], 5, 2, (2,), idx=idx)
    if name == "many_joints":
        return _inputs(gen, 2, 64, LDS_JOINTS + 1, 4, (2,))
    if name == "mat4":
        return _inputs(gen, 2, 77, 7, 4, (2,), mat4=True, empty_prob=0.1)
    if name == "mat4_view":
        v, idx, w, t, grad = _inputs(gen, 2, 77, 7, 4, (1,), mat4=True, empty_prob=0.1)
        return v, idx, w, t[..., :3, :], grad
    raise KeyError(name)


CASES = ("tiny", "block_edge", "shared_v", "shared_v_expand", "shared_v_2d", "k8_slots", "chunked", "many_joints", "mat4",
         "mat4_view")
SEEDS = tuple(range(40))
_cache = {}


def case(name):
    """(v, joint_idx int64, joint_weights, transforms, grad) in float64 on the CPU; built once, never modified"""
    if name not in _cache:
        _cache[name] = _case(name)
    return _cache[name]


def build_case(seed):
    """A seeded random shape: V <= 700, J <= 40, K <= 8, N <= 3; empty slots, every layout of v and of the transforms"""
    gen = th.Generator().manual_seed(1000 + seed)
    ri = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=gen))  # noqa: E731
    n, num_v, num_j, k = ri(1, 3), ri(1, 700), ri(1, 40), ri(1, 8)
    layout, mat = ri(0, 3), ri(0, 2)
    v, idx, w, t, grad = _inputs(gen, n, num_v, num_j, k, (n,) if layout == 0 else (1,), mat4=mat > 0,
                                 empty_prob=(0.0, 0.15, 0.5)[ri(0, 2)])
    if layout == 2:
        v = v.expand(n, -1, -1)
    elif layout == 3:
        v = v[0]
    if mat == 2:
        t = t[..., :3, :]
    return v, idx, w, t, grad


_ref = {}


def reference(key, dtype):
    """The oracle's results for case(key) (a name) or build_case(key) (a seed) in `dtype`; computed once per pair"""
    if (key, dtype) not in _ref:
        inputs = case(key) if isinstance(key, str) else build_case(key)
        _ref[(key, dtype)] = results(skin, *inputs, dtype)
    return _ref[(key, dtype)]


def exact_zeros(joint_idx, transforms):
    """Masks of the elements stated to be exactly 0: {"out": [V] (all slots empty), "grad_w": [V,K] (empty slots),
    "grad_t_joint": [J] (a joint nobody names)}; row 3 of a 4x4 grad_t is exactly 0 as well."""
    num_j = transforms.shape[1]
    named = th.zeros(num_j, dtype=th.bool)
    named[joint_idx[joint_idx >= 0].long()] = True
    return {"out": (joint_idx < 0).all(1), "grad_w": joint_idx < 0, "grad_t_joint": ~named}
