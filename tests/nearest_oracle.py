"""TEST INFRASTRUCTURE -- an oracle for drtk_amd.nearest_points that shares nothing with the package's formulation: a
brute-force statement of the definition on the CPU,

    d2(i,j) = ((px-qx)*(px-qx) + (py-qy)*(py-qy)) + (pz-qz)*(pz-qz)        in the tensors' dtype, as written
    idx[n,i] = the lowest j whose d2 is minimal among the candidates with d2 < +inf, else -1;   dist2 = that d2, else +inf

with the argmin made explicit (the candidates that equal the minimum, the smallest of their indices), and the gradients
written out from the definition with idx held constant -- in float64, or in the dtype asked for:

    grad_p[n,i] = 2 g[n,i] (p_i - q_idx)         grad_q[n,j] = - sum over the i with idx[n,i] = j of 2 g[n,i] (p_i - q_j)

CASES are the smallest shapes at which the kernels of csrc/nearest.hip can go wrong, built from the constants of
include/drtk_amd.h; build_case(seed) draws random shapes for the fuzz rows.  One case is at most about 4096 x 4096 x 2."""
import os
import re

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    m = re.search(r"#define\s+DRTK_NEAREST_" + name + r"\s+(\d+)\b", hdr)
    assert m, f"include/drtk_amd.h no longer defines DRTK_NEAREST_{name}"
    return int(m.group(1))


R = _constant("R")                        # queries per lane
QUERIES = _constant("QUERIES")            # queries per workgroup
TILE = _constant("TILE")                  # targets per LDS tile
SPLIT_BLOCKS = _constant("SPLIT_BLOCKS")  # fewer workgroups than this: the targets are split
CHUNK = _constant("CHUNK")                # sorted positions per workgroup of the grad_q chunk pass


def split(n, num_p, num_q):
    """(S, L) of the launch rule as include/drtk_amd.h states it: S ranges of L targets"""
    cd = lambda a, b: -(-a // b)  # noqa: E731
    blocks = n * cd(num_p, QUERIES)
    if blocks <= 0 or blocks >= SPLIT_BLOCKS or num_q <= TILE:
        return 1, num_q
    s0 = min(cd(SPLIT_BLOCKS, blocks), cd(num_q, TILE))
    length = cd(cd(num_q, s0), TILE) * TILE
    return cd(num_q, length), length


def _batched(p, q):
    pb = p.shape[0] if p.dim() == 3 else 1
    qb = q.shape[0] if q.dim() == 3 else 1
    n = qb if pb == 1 else pb
    return (p if p.dim() == 3 else p[None]).expand(n, -1, -1), (q if q.dim() == 3 else q[None]).expand(n, -1, -1), n


def nearest(p, q):
    """(dist2 [N,P] in the dtype of p, idx [N,P] int64) by the definition"""
    pp, qq, n = _batched(p.detach(), q.detach())
    num_p, num_q = pp.shape[1], qq.shape[1]
    inf = float("inf")
    dist2 = th.full((n, num_p), inf, dtype=p.dtype)
    idx = th.full((n, num_p), -1, dtype=th.int64)
    if num_q == 0 or n * num_p == 0:
        return dist2, idx
    js = th.arange(num_q)
    step = max(1, (1 << 21) // num_q)
    for v in range(n):
        qx, qy, qz = qq[v, :, 0][None], qq[v, :, 1][None], qq[v, :, 2][None]
        for i0 in range(0, num_p, step):
            c = pp[v, i0:i0 + step]
            dx, dy, dz = c[:, 0:1] - qx, c[:, 1:2] - qy, c[:, 2:3] - qz
            d = (dx * dx + dy * dy) + dz * dz
            ok = d < inf
            best = th.where(ok, d, th.full_like(d, inf)).amin(1)
            first = th.where(ok & (d == best[:, None]), js[None], th.full_like(js, num_q)[None]).amin(1)
            dist2[v, i0:i0 + step] = best
            idx[v, i0:i0 + step] = th.where(first < num_q, first, th.full_like(first, -1))
    return dist2, idx


def gradients(p, q, idx, g, dtype=th.float64):
    """(grad_p, grad_q) of the definition with idx held constant, the arithmetic in `dtype`, shaped like p and q as given (a
    shared input gets the sum over the views; a stride-0 expand counts as its one row)"""
    pp, qq, n = _batched(p.detach().to(dtype), q.detach().to(dtype))
    num_q = qq.shape[1]
    valid = idx >= 0
    if num_q > 0:
        chosen = th.gather(qq, 1, idx.clamp(min=0)[..., None].expand(-1, -1, 3))
    else:
        chosen = th.zeros_like(pp)
    zero = th.zeros((), dtype=dtype)
    diff = th.where(valid[..., None], pp, zero) - th.where(valid[..., None], chosen, zero)
    gp = 2 * g.to(dtype)[..., None] * diff
    gq = th.zeros(n, num_q + 1, 3, dtype=dtype)  # (row num_q collects the rows without a neighbour and is dropped)
    for v in range(n):
        gq[v].index_add_(0, th.where(valid[v], idx[v], th.full_like(idx[v], num_q)), -gp[v])
    gq = gq[:, :num_q]

    def shaped(grad, like):
        shared = like.dim() == 2 or like.shape[0] == 1 or (like.shape[0] > 1 and like.stride(0) == 0)
        if shared and like.dim() == 3 and like.shape[0] > 1:  # an expand: the leaf is its one row
            return grad.sum(0, keepdim=True)
        if shared:
            return grad.sum(0, keepdim=True).view(like.shape)
        return grad

    return shaped(gp, p), shaped(gq, q)


def _leaf(x, dtype, device):
    """(leaf, the tensor to pass): a stride-0 expand is rebuilt on the device from its one row"""
    expanded = x.dim() == 3 and x.shape[0] > 1 and x.stride(0) == 0
    leaf = (x[:1] if expanded else x).to(dtype).to(device).clone().requires_grad_(True)
    return leaf, (leaf.expand(x.shape[0], -1, -1) if expanded else leaf)


def results(fn, p, q, g, dtype, device="cpu"):
    """{"dist2", "idx", "grad_p", "grad_q"} of `fn` (the package) on copies of the inputs in `dtype` on `device`, the
    gradients through autograd, shaped like the leaves (an expand: its one row)"""
    pl, pp = _leaf(p, dtype, device)
    ql, qq = _leaf(q, dtype, device)
    dist2, idx = fn(pp, qq)
    assert not idx.requires_grad
    gp, gq = th.autograd.grad(dist2, (pl, ql), g.to(dtype).to(device), allow_unused=True)
    zero = lambda x, like: th.zeros_like(like) if x is None else x  # noqa: E731
    return {"dist2": dist2.detach().cpu(), "idx": idx.cpu(), "grad_p": zero(gp, pl).cpu(), "grad_q": zero(gq, ql).cpu()}


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _r(gen, *shape, scale=1.0):
    """float64 values that are exact in float32 (one set of inputs for either precision)"""
    return (scale * th.randn(*shape, dtype=th.float64, generator=gen)).float().double()


def _random(gen, n, num_p, num_q, p_batch=None, q_batch=None):
    p = _r(gen, *(() if p_batch == 0 else (n if p_batch is None else p_batch,)), num_p, 3)
    q = _r(gen, *(() if q_batch == 0 else (n if q_batch is None else q_batch,)), num_q, 3)
    return p, q, _r(gen, n, num_p)


def _clusters(gen, n, counts, num_q, nan_rows=0):
    """Targets far apart on the x axis; counts[j] queries next to target j (shuffled over i), `nan_rows` NaN queries"""
    q = th.zeros(n, num_q, 3, dtype=th.float64)
    q[:, :, 0] = 16.0 * th.arange(num_q, dtype=th.float64)
    owner = th.cat([th.full((c,), j) for j, c in enumerate(counts)])
    num_p = owner.numel() + nan_rows
    p = th.full((n, num_p, 3), float("nan"), dtype=th.float64)
    for v in range(n):
        perm = th.randperm(num_p, generator=gen)
        rows = perm[:owner.numel()]
        p[v, rows] = q[v, owner] + _r(gen, owner.numel(), 3)
    return p, q, _r(gen, n, num_p)


def _case(name):
    gen = th.Generator().manual_seed(sum(map(ord, name)))
    nan = float("nan")
    if name == "one":
        return _random(gen, 1, 1, 1)
    if name == "queries_exact":
        return _random(gen, 2, QUERIES, 37)
    if name == "queries_minus":
        return _random(gen, 1, QUERIES - 1, 37)
    if name == "queries_plus":
        return _random(gen, 2, QUERIES + 1, 37)
    if name == "not_multiple_of_r":
        return _random(gen, 2, 64 * R + 3, 50)
    if name == "tile_exact":
        return _random(gen, 1, 70, TILE)
    if name == "tile_minus":
        return _random(gen, 2, 70, TILE - 1)
    if name == "tile_plus_split_short":       # S = 2, the last range holds one target
        return _random(gen, 1, 70, TILE + 1)
    if name == "one_target":
        return _random(gen, 2, 3000, 1)
    if name == "below_split_threshold":       # SPLIT_BLOCKS - 1 workgroups: S = 2
        return _random(gen, SPLIT_BLOCKS - 1, 3, TILE + 5)
    if name == "at_split_threshold":          # SPLIT_BLOCKS workgroups: S = 1, two tiles
        return _random(gen, SPLIT_BLOCKS, 3, TILE + 5)
    if name == "split_six":                   # S = 6, the last range 300 targets
        return _random(gen, 1, 40, 5 * TILE + 300)
    if name == "split_long_ranges":           # 300 workgroups: S = 2 ranges of 3 tiles, the last short
        return _random(gen, 300, 2, 4 * TILE + 7)
    if name == "shared_q":
        return _random(gen, 3, 300, 200, q_batch=1)
    if name == "shared_q_2d":
        return _random(gen, 3, 300, 200, q_batch=0)
    if name == "shared_p":
        return _random(gen, 3, CHUNK + 40, 90, p_batch=1)
    if name == "shared_p_2d":
        return _random(gen, 2, 130, 2 * TILE + 3, p_batch=0)
    if name == "shared_expand":
        p, q, g = _random(gen, 3, 150, 140, p_batch=1)
        return p.expand(3, -1, -1), q[:1].expand(3, -1, -1), g
    if name == "all_one_target":              # one run across many chunks
        return _clusters(gen, 2, [0, 0, 3 * CHUNK + 17, 0, 0], 5)
    if name == "own_target":                  # runs of length 1
        q = _r(gen, 2, 2 * CHUNK + 3, 3, scale=8.0)
        return (q + _r(gen, *q.shape, scale=1e-3)).float().double(), q, _r(gen, 2, q.shape[1])
    if name == "runs_end_on_chunk_edges":
        return _clusters(gen, 2, [CHUNK, CHUNK, 0, 2 * CHUNK, 5], 6)
    if name == "minus_one_front":             # 37 NaN queries: a run of -1 at the front of the sorted list
        return _clusters(gen, 2, [CHUNK - 37, 3, CHUNK + 1], 3, nan_rows=37)
    if name == "lattice":                     # integer points: many exactly equal distances
        q = th.randint(-3, 4, (2, TILE + 300, 3), generator=gen).double()
        p = th.randint(-3, 4, (2, 333, 3), generator=gen).double()
        return p, q, _r(gen, 2, 333)
    if name == "duplicates_across_tiles_and_splits":  # S = 3: q[0] again at q[TILE] and at q[2 TILE], the head of range 2
        p, q, g = _random(gen, 1, 200, 2 * TILE + 5)
        q = q + 50.0                          # the cloud; targets 0 and 7 stand apart from it
        q[:, 0] = _r(gen, 1, 3)
        q[:, 7] = _r(gen, 1, 3) - 40.0
        q[:, TILE] = q[:, 0]
        q[:, 2 * TILE] = q[:, 0]
        q[:, 2 * TILE + 3] = q[:, 7]
        p = (q[:, :1] + _r(gen, 1, 200, 3, scale=0.5)).float().double()
        p[:, 100:] = (q[:, 7:8] + _r(gen, 1, 100, 3, scale=0.5)).float().double()
        return p, q, g
    if name == "duplicates_one_range":        # S = 1 (enough workgroups): the duplicate sits in the second tile
        p, q, g = _random(gen, SPLIT_BLOCKS, 2, TILE + 9)
        q[:, 5] = _r(gen, SPLIT_BLOCKS, 3) + 30.0  # apart from the cloud
        q[:, TILE + 2] = q[:, 5]
        p = (q[:, 5:6] + _r(gen, SPLIT_BLOCKS, 2, 3, scale=0.25)).float().double()
        return p, q, g
    if name == "overflow_target":             # 3e19 squared overflows float32: never chosen there
        p, q, g = _random(gen, 2, 90, 40)
        q[:, 3] = th.tensor([3e19, 0.0, 0.0]).double()
        q[0, 11] = th.tensor([0.0, -3e19, 3e19]).double()
        return p, q, g
    if name == "nan_target":
        p, q, g = _random(gen, 2, 90, 40)
        q[:, 0, 1] = nan
        q[1, 17] = nan
        return p, q, g
    if name == "nan_query":
        p, q, g = _random(gen, 2, 2 * CHUNK + 9, 40)
        p[0, 5] = nan
        p[1, CHUNK:CHUNK + 3, 2] = nan
        return p, q, g
    if name == "rejected_in_second_split":    # S = 2: the second range holds NaN, overflow and a duplicate of q[1]
        p, q, g = _random(gen, 1, 80, TILE + 9)
        q[:, TILE] = nan
        q[:, TILE + 1] = th.tensor([3e19, 3e19, 3e19]).double()
        q[:, TILE + 2] = q[:, 1]
        q[:, TILE + 3:, 0] = nan
        p[0, 7] = nan
        return p, q, g
    if name == "second_split_wins":           # S = 2: every target of the first range is rejected
        p, q, g = _random(gen, 1, 80, TILE + 9)
        q[:, :TILE, 2] = nan
        return p, q, g
    if name == "all_rejected":                # S = 2 and S = 1 rows alike: no candidate anywhere
        p, q, g = _random(gen, 1, 80, TILE + 9)
        q[:, :, 0] = nan
        return p, q, g
    raise KeyError(name)


CASES = ("one", "queries_exact", "queries_minus", "queries_plus", "not_multiple_of_r", "tile_exact", "tile_minus",
         "tile_plus_split_short", "one_target", "below_split_threshold", "at_split_threshold", "split_six", "split_long_ranges",
         "shared_q", "shared_q_2d", "shared_p", "shared_p_2d", "shared_expand", "all_one_target", "own_target",
         "runs_end_on_chunk_edges", "minus_one_front", "lattice", "duplicates_across_tiles_and_splits", "duplicates_one_range",
         "overflow_target", "nan_target", "nan_query", "rejected_in_second_split", "second_split_wins", "all_rejected")
# cases whose every gradient is exactly zero (nothing is chosen)
ALL_ZERO = ("all_rejected",)
SEEDS = tuple(range(40))
_cache = {}


def case(name):
    """(p, q, grad) in float64 on the CPU, exact in float32; built once, never modified"""
    if name not in _cache:
        _cache[name] = _case(name)
    return _cache[name]


def build_case(seed):
    """A seeded random shape: N <= 3, P and M <= 2600 (up to three tiles and three workgroups of queries), every batch layout,
    now and then a NaN point or a duplicated target"""
    gen = th.Generator().manual_seed(2000 + seed)
    ri = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=gen))  # noqa: E731
    n = ri(1, 3)
    num_p = ri(1, 2600) if ri(0, 2) else ri(1, 40)
    num_q = ri(1, 2600) if ri(0, 2) else ri(1, 40)
    layout_p, layout_q = ri(0, 3), ri(0, 3)
    p, q, g = _random(gen, n, num_p, num_q, p_batch=(None, 1, 1, 0)[layout_p], q_batch=(None, 1, 1, 0)[layout_q])
    if ri(0, 3) == 0:
        q[..., ri(0, num_q - 1), :] = float("nan")
    if ri(0, 3) == 0:
        p[..., ri(0, num_p - 1), 1] = float("nan")
    if ri(0, 2) == 0 and num_q > 1:
        q[..., num_q - 1, :] = q[..., 0, :]
    if layout_p == 2:
        p = p.expand(n, -1, -1)
    if layout_q == 2:
        q = q.expand(n, -1, -1)
    return p, q, g[:_batched(p, q)[2]]  # (both shared: one view)


_ref = {}


def reference(key, dtype):
    """The oracle on case(key) (a name) or build_case(key) (a seed): {"dist2", "idx"} evaluated in `dtype`, and with that idx
    held constant {"grad_p", "grad_q"} in float64 and {"grad_p_own", "grad_q_own"} in `dtype`; computed once per pair"""
    if (key, dtype) not in _ref:
        p, q, g = case(key) if isinstance(key, str) else build_case(key)
        dist2, idx = nearest(p.to(dtype), q.to(dtype))
        gp, gq = gradients(p, q, idx, g, th.float64)
        gp_own, gq_own = gradients(p, q, idx, g, dtype)
        _ref[(key, dtype)] = {"dist2": dist2, "idx": idx, "grad_p": gp, "grad_q": gq, "grad_p_own": gp_own, "grad_q_own": gq_own}
    return _ref[(key, dtype)]


def chamfer(x, y, x_weights=None, y_weights=None, bidirectional=True, squared=True):
    """chamfer_distance by its definition, composed from `nearest` (no autograd): the mean over the views of the weighted
    means of the distances, a point without a neighbour weighing 0, a view without weight giving 0"""
    def term(a, b, w):
        d2, idx = nearest(a, b)
        valid = idx >= 0
        d = th.where(valid, d2, th.zeros_like(d2))
        if not squared:
            d = d.sqrt()
        w = valid.to(d.dtype) if w is None else valid.to(d.dtype) * w.to(d.dtype)
        out = th.zeros(d.shape[0], dtype=d.dtype)
        for v in range(d.shape[0]):
            if float(w[v].sum()) != 0:
                out[v] = (w[v] * d[v]).sum() / w[v].sum()
        return out

    total = term(x, y, x_weights)
    if bidirectional:
        total = total + term(y, x, y_weights)
    return total.mean() if total.numel() else total.sum()
