"""Index images for the vertex-table scatters (drtk_amd/csrc/segscatter.hpp): render backward, interpolate backward's
register-scan and wide kernels, and the A^T A values kernel reduce per-pixel terms into per-vertex (per-triangle) sums through
a run sum along 64 pixels, a small LDS hash table (kTableSlots entries per 64 x 4 wave tile, kTableProbes linear probes; the
wide kernel: 16 ... 128 entries per 64 x 16 workgroup tile) and direct global atomics where a key finds no slot.  A rasterized
image is coherent -- a tile holds a handful of vertices -- so the table never fills; any index image is a valid input, and the
ones here are built per pixel so that it does: full tables, probe chains exhausted in a nearly empty table, one vertex that
goes through the table in one tile and round it in another, runs cut at every lane boundary the kernels treat specially.

The constants the constructions depend on are READ from the sources (a change of table size must break the construction
loudly, not void it); `home_slot` and `wide_log2_slots` restate the two choices of the kernels the cases are aimed at.
tests/test_scatter_table_cases_host.py asserts, without a GPU, that every case has the property it is named for;
tests/test_gpu_scatter_tables.py runs them through the kernels."""
import functools
import math
import os
import re
import sys
import types

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CSRC = os.path.join(ROOT, "drtk_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(name, pattern, at_least=1):
    """The one integer every match of `pattern` in csrc/<name> captures; raises if there is none or they differ."""
    found = set(re.findall(pattern, _source(name)))
    count = len(re.findall(pattern, _source(name)))
    if len(found) != 1 or count < at_least:
        raise RuntimeError(f"scatter_table_cases: {pattern!r} matches {count} times in {name} with values {sorted(found)}: "
                           "the table's constants moved -- the case constructions of this module must follow them")
    return int(found.pop())


K_TABLE_SLOTS = _constant("segscatter.hpp", r"constexpr\s+int\s+kTableSlots\s*=\s*(\d+)\s*;")
K_TABLE_PROBES = _constant("segscatter.hpp", r"constexpr\s+int\s+kTableProbes\s*=\s*(\d+)\s*;")
K_TILE_ROWS = _constant("segscatter.hpp", r"constexpr\s+int\s+kTileRows\s*=\s*(\d+)\s*;")
HASH_MULTIPLIER = _constant("segscatter.hpp", r"static_cast<uint32_t>\(vid\w*(?:\[k\])?\)\s*\*\s*(\d+)u\)\s*>>\s*\(32\s*-", at_least=3)
K_WAVE = _constant("common.hpp", r"constexpr\s+int\s+kWave\s*=\s*(\d+)\s*;")
K_BLOCK = _constant("common.hpp", r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;")
TABLE_BYTES = _constant("interpolate.hip", r"#define\s+DRTK_INTERP_TABLE_BYTES\s+(\d+)")
WIDE_LOG2_MAX = _constant("interpolate.hip", r"int\s+log2_slots\s*=\s*(\d+)\s*;")
WIDE_LOG2_MIN = _constant("interpolate.hip", r"table\s*=\s*log2_slots\s*>=\s*(\d+)")
SMALL_MAXC_F32 = _constant("interpolate.hip", r"#define\s+DRTK_INTERP_SMALL_MAXC_F32\s+(\d+)")
SMALL_MAXC_F64 = _constant("interpolate.hip", r"#define\s+DRTK_INTERP_SMALL_MAXC_F64\s+(\d+)")
if not re.search(r"using\s+TableAcc\s*=\s*double\s*;", _source("segscatter.hpp")):
    raise RuntimeError("scatter_table_cases: the tables no longer accumulate in double: wide_log2_slots must follow")
TABLE_ACC_BYTES = 8
WAVE_ROWS = K_TILE_ROWS // (K_BLOCK // K_WAVE)  # rows of a wave tile: a workgroup's 16 rows over its 4 waves
LOG2_SLOTS = K_TABLE_SLOTS.bit_length() - 1
assert 1 << LOG2_SLOTS == K_TABLE_SLOTS and WAVE_ROWS * (K_BLOCK // K_WAVE) == K_TILE_ROWS and K_WAVE == 64


def home_slot(vid, log2_slots):
    """table_slot / table_slot_rt: (uint32(vid) * multiplier) >> (32 - log2 slots)."""
    return ((int(vid) * HASH_MULTIPLIER) & 0xFFFFFFFF) >> (32 - log2_slots)


def wide_log2_slots(C):
    """interpolate_backward_impl: the largest table of at most 2^7 slots whose rows of C double accumulators and a key
    fit DRTK_INTERP_TABLE_BYTES; the table is used from 2^4 slots (and only where the rows of attr_grad are not whole
    64-byte segments)."""
    log2_slots = WIDE_LOG2_MAX
    while log2_slots > 0 and (TABLE_ACC_BYTES * C + 4) << log2_slots > TABLE_BYTES:
        log2_slots -= 1
    return log2_slots


def wide_takes_table(C, itemsize=4):
    row = itemsize * C
    return wide_log2_slots(C) >= WIDE_LOG2_MIN and not (row % 64 == 0 or 64 % row == 0)


SHAPES = [(1, 1), (4, 64), (5, 65), (16, 63), (17, 130), (33, 192)]  # tiles of 64 x 16: 1, 1, 2, 1, 6, 9
THREE_TILES = (4, 130)                                               # ... and 3: the tile counts 1, 2, 3, 6, 9 of tile_index' strips
DEFAULT = (17, 130)
N = 2


# ---- pieces ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return th.Generator().manual_seed(s)


def _seed_of(name, *ints):
    return (sum(ord(c) * (i + 1) for i, c in enumerate(name)),) + tuple(int(i) for i in ints)


def _triangles(idx, F, H, W, g):
    """F well-shaped triangles of their own, [F,3,3] pixel-space corners, each AROUND the pixels that `idx` [N,H,W] gives it
    (faces < 0 or >= F: not this call's): centre at their centroid, circumradius 8 pixels + 2.6 x their farthest distance
    from it (corners 120 degrees apart +- 0.15 rad, radii + 0 ... 15 %: the inscribed circle holds them all), depths within 2 %
    of the triangle's own.  The index images here give a triangle to pixels wherever they like; a pixel far outside its
    triangle (the float32 oracle is then hundreds of ulps of the accumulated magnitude from the double one, tried) would make
    render backward's terms a matter of conditioning instead of summation.  Unused faces lie anywhere on the canvas."""
    y, x = th.meshgrid(th.arange(H, dtype=th.float32), th.arange(W, dtype=th.float32), indexing="ij")
    pts = th.stack([x, y], -1)[None].expand(idx.shape[0], -1, -1, -1)
    m = (idx >= 0) & (idx < F)
    f, p = idx[m], pts[m]
    cnt = th.zeros(F).index_add_(0, f, th.ones(f.numel()))
    c = th.zeros(F, 2).index_add_(0, f, p) / cnt.clamp(min=1)[:, None]
    c = th.where((cnt > 0)[:, None], c, th.rand(F, 2, generator=g) * th.tensor([float(W), float(H)]))
    d = th.zeros(F).scatter_reduce_(0, f, (p - c[f]).norm(dim=-1), "amax")
    r = (8 + 2.6 * d)[:, None] * (1 + 0.15 * th.rand(F, 3, generator=g))
    a = th.rand(F, 1, generator=g) * 2 * math.pi + th.tensor([0.0, 2 * math.pi / 3, 4 * math.pi / 3]) + 0.3 * (th.rand(F, 3, generator=g) - 0.5)
    z = (0.8 + 1.2 * th.rand(F, 1, generator=g)) * (1 + 0.02 * th.rand(F, 3, generator=g))
    return th.stack([c[:, None, 0] + r * th.cos(a), c[:, None, 1] + r * th.sin(a), z], -1)


def _run_ids(W, count, g, lo=3, hi=5, background=0.1):
    """One row of runs of lo ... hi pixels over ids [0, count), neighbours different, a share of the runs background."""
    row = th.empty(W, dtype=th.int64)
    x, prev = 0, -2
    while x < W:
        n = int(th.randint(lo, hi + 1, (1,), generator=g))
        t = -1 if float(th.rand(1, generator=g)) < background and prev != -1 else int(th.randint(0, count, (1,), generator=g))
        if t == prev:
            t = (t + 1) % count
        row[x:x + n] = t
        x, prev = x + n, t
    return row


def _bary(N_, H, W, g):
    b = th.rand(N_, 3, H, W, generator=g) + 0.05
    return (b / b.sum(1, keepdim=True)).contiguous()


class Case(types.SimpleNamespace):
    """One case; hashed by identity (the builders are cached), so that the references can be cached per case."""
    __hash__ = object.__hash__

    def __eq__(self, other):
        return self is other


def _finish(name, H, W, g, vi, idx, V, ids, corners, per_view_vi=False, **extra):
    """vi: [F,3] LOCAL vertex numbers 0 ... len(ids)-1, `ids` their vertex ids (< V; the rest of the V vertices is referenced by
    nobody and must come out exactly zero), corners [len(ids),3] their pixel-space positions."""
    ids = th.as_tensor(ids, dtype=th.int64)
    assert ids.numel() == corners.shape[0] and int(ids.max()) < V and ids.unique().numel() == ids.numel()
    v1 = th.stack([th.rand(V, generator=g) * W, th.rand(V, generator=g) * H, 1 + th.rand(V, generator=g)], -1)
    v1[ids] = corners
    v = (v1[None] + 0.25 * th.rand(N, V, 3, generator=g) * th.tensor([1.0, 1.0, 0.02])).contiguous()
    vi_g = ids[vi.long()].int()
    if per_view_vi:  # the second view names every face's corners in rotated order: same triangles, other (corner, vertex) pairs
        vi_g = th.stack([vi_g, vi_g.roll(1, -1)]).contiguous()
    idx = idx.int().contiguous()
    assert idx.shape == (N, H, W) and int(idx.max()) < vi.shape[0] and int(idx.min()) >= -1
    extra.setdefault("well_shaped", True)
    return Case(name=name, N=N, H=H, W=W, V=V, F=vi.shape[0], vi=vi_g.contiguous(), idx=idx, bary=_bary(N, H, W, g),
                                 v=v, per_view_vi=per_view_vi, **extra)


def _disjoint(idx, F, H, W, g):
    return th.arange(3 * F).view(F, 3), _triangles(idx, F, H, W, g).reshape(3 * F, 3)


# ---- patterns -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def per_pixel(H, W, per_view_vi=False):
    """A different triangle at every pixel, faces with vertices of their own: 3 x 64 x 4 = 768 distinct vertices (256
    triangles) in a wave tile against kTableSlots = 64; 3 % of the pixels background (none at 1 x 1)."""
    g = _gen(*_seed_of("per_pixel", H, W, per_view_vi))
    F = H * W
    base = th.randperm(F, generator=g).view(H, W)
    y, x = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    swap = lambda i, n: th.where((i ^ 1) < n, i ^ 1, i)  # noqa: E731
    idx = th.stack([base, base[swap(y, H), swap(x, W)]])  # the second view: neighbours swapped -- every triangle stays near its pixels
    if F > 1:
        idx[th.rand(N, H, W, generator=g) < 0.03] = -1
    vi, corners = _disjoint(idx, F, H, W, g)
    V = 3 * F + 5
    return _finish(f"per_pixel {H}x{W}" + (" per-view vi" if per_view_vi else ""), H, W, g, vi, idx, V,
                   th.randperm(V, generator=g)[:3 * F], corners, per_view_vi)


@functools.lru_cache(maxsize=None)
def per_column(H, W, per_view_vi=False):
    """A different triangle in every COLUMN, with vertices of its own, the same down the column (the second view: neighbouring
    columns swapped): every pixel is a run of its own, and a wave tile holds 3 x 64 = 192 distinct vertices against 64 slots --
    the table must overflow -- while a vertex still collects a term from every row.  For render backward, in place of
    per_pixel: there an output element is ONE term, and the depth component of the float32 oracle's single term is itself
    7 ... 10 ulps of that term from the double one (measured; whatever the triangles' size, depth range or sharing) -- at the
    bound's 8 ulps the figure would say how one term rounds, not how the scatter sums."""
    g = _gen(*_seed_of("per_column", H, W, per_view_vi))
    y, x = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    idx = th.stack([x, th.where((x ^ 1) < W, x ^ 1, x)])
    if H * W > 1:
        idx[th.rand(N, H, W, generator=g) < 0.03] = -1
    vi, corners = _disjoint(idx, W, H, W, g)
    V = 3 * W + 5
    return _finish(f"per_column {H}x{W}" + (" per-view vi" if per_view_vi else ""), H, W, g, vi, idx, V, th.randperm(V, generator=g)[:3 * W], corners, per_view_vi)


def colliding_ids(count, log2_slots, g):
    """`count` ascending ids of ONE home slot of a 2^log2_slots table (the slot and the first id seeded)."""
    target = int(th.randint(0, 1 << log2_slots, (1,), generator=g))
    out, i = [], int(th.randint(0, 50, (1,), generator=g))
    while len(out) < count:
        if home_slot(i, log2_slots) == target:
            out.append(i)
        i += 1
    return out


@functools.lru_cache(maxsize=None)
def collide(H, W, log2_slots=LOG2_SLOTS, key="vertex", per_view_vi=False):
    """Ten triangles in runs of 3 ... 5 pixels whose keys all have one home slot of a 2^log2_slots table: kTableProbes = 6 of
    them find a slot, the others go round a table that is nearly empty.  key = "vertex": the 30 vertex ids of ten disjoint
    triangles -- or, for tables of fewer than 60 slots, half as many ids as the table has slots, shared among the ten;
    key = "triangle" (the A^T A kernel's table): the ten triangle ids."""
    g = _gen(*_seed_of("collide" + key, H, W, log2_slots, per_view_vi))
    T = 10
    rows = th.stack([th.stack([_run_ids(W, T, g) for _ in range(H)]) for _ in range(N)])
    if key == "vertex":
        P = min(3 * T, (1 << log2_slots) // 2)
        pool = colliding_ids(P, log2_slots, g)
        local = th.tensor([[(3 * t + k) % P for k in range(3)] for t in range(T)])
        corners = _triangles(rows, T, H, W, g).reshape(3 * T, 3)[:P]  # (P < 30: the shared corners make no well-shaped faces; interpolate only)
        vi, ids, tris, V = local, pool, list(range(T)), max(pool) + 4
        idx = rows
    else:
        tris = colliding_ids(T, log2_slots, g)
        F = max(tris) + 3
        idx = th.where(rows >= 0, th.tensor(tris)[rows.clamp(min=0)], rows)
        vi, corners = _disjoint(idx, F, H, W, g)
        V = 3 * F + 5
        ids, pool = th.randperm(V, generator=g)[:3 * F], tris
    return _finish(f"collide {H}x{W} 2^{log2_slots} slots, {key} keys" + (" per-view vi" if per_view_vi else ""), H, W, g, vi, idx, V, ids, corners,
                   per_view_vi, pool=pool, log2_slots=log2_slots, well_shaped=key == "triangle" or P == 3 * T)


HOT_GRID = (5, 8)  # 40 hot vertices, 4 x 7 cells, 56 hot triangles


def _swap_neighbours(i, n):
    """i ^ 1 where that is still below n: columns (rows) swapped in pairs."""
    return th.where((i ^ 1) < n, i ^ 1, i)


def _hot_grid(H, W, g):
    """The hot patch: a jittered 5 x 8 lattice over the canvas.  -> (corners [40,3], faces [56,3]: 2c and 2c + 1 are
    cell c's two triangles, hot_face(x, y): the hot triangle a pixel lies in, up to the jitter)."""
    gy, gx = HOT_GRID
    cw, ch = W / (gx - 1), H / (gy - 1)
    yy, xx = th.meshgrid(th.arange(gy), th.arange(gx), indexing="ij")
    corners = th.stack([xx.flatten() * cw, yy.flatten() * ch, th.full((gy * gx,), 1.5)], -1)
    corners = corners + (th.rand(gy * gx, 3, generator=g) - 0.5) * th.tensor([0.2 * cw, 0.2 * ch, 0.02])
    j, i = th.meshgrid(th.arange(gy - 1), th.arange(gx - 1), indexing="ij")
    a = (j * gx + i).flatten()
    upper = th.stack([a, a + 1, a + gx + 1], -1)
    lower = th.stack([a, a + gx + 1, a + gx], -1)
    faces = th.stack([upper, lower], 1).reshape(-1, 3)

    def hot_face(x, y):
        u, w = x.float() / cw, y.float() / ch
        cx, cy = u.floor().clamp(0, gx - 2), w.floor().clamp(0, gy - 2)
        return (2 * (cy * (gx - 1) + cx) + ((u - cx) < (w - cy)).long()).long()

    return corners, faces, hot_face, cw


def _crowded_tile(x, y, hot_face, own):
    """A triangle of the column's own at every pixel, every fourth pixel the hot triangle it lies in."""
    return th.where(x % 4 == 0, hot_face(x, y), own)


def _calm_tile(x, y, hot_face, g):
    """The two hot triangles of the grid cell at the wave tile's centre, in runs of 3 ... 5 pixels."""
    H, W = x.shape
    two = th.stack([_run_ids(W, 2, g, background=0.0) for _ in range(H)])
    cx = (x // K_WAVE * K_WAVE + K_WAVE // 2).clamp(max=W - 1)
    cy = y // WAVE_ROWS * WAVE_ROWS + 1
    return hot_face(cx, cy) // 2 * 2 + two


def _hot_tile(x, y, hot_face, cw, g):
    """Runs of 3 ... 5 pixels over the hot triangles around each run's first pixel (the run's seeded label picks the cell to
    the left, the cell itself or the one to the right, and which of its two triangles); a tenth of the runs background."""
    H, W = x.shape
    runs = th.stack([_run_ids(W, 3000, g) for _ in range(H)])
    head = th.cat([th.ones(H, 1, dtype=th.bool), runs[:, 1:] != runs[:, :-1]], 1)
    start = th.where(head, x, th.zeros_like(x)).cummax(1).values
    near = (start + (runs % 3 - 1) * 0.9 * cw).clamp(0, W - 1)
    return th.where(runs >= 0, hot_face(near, y) // 2 * 2 + runs // 3 % 2, runs)


@functools.lru_cache(maxsize=None)
def mixed(H, W, per_view_vi=False, split=2):
    """40 hot vertices -- a 5 x 8 grid over the canvas, 56 hot triangles -- over three kinds of wave tile, (row group +
    column) mod 3: 0 CROWDED -- `split` triangles of its own in every column (its rows in turn), every fourth pixel the hot
    triangle it lies in: the table overflows, and which of the hot vertices still found a slot is a matter of order;
    1 CALM -- the two hot triangles of the grid cell at the tile's centre in runs of 3 ... 5 pixels: four keys, every one
    finds a slot; 2 HOT -- runs over the hot triangles of the neighbourhood.  A hot vertex is therefore fed through the
    table in one tile and, possibly, round it in another, in one launch.
    split = 2: more than 64 triangles in a crowded wave tile, for the table keyed by triangle; split = 1 for float32
    render backward, which needs some terms per vertex (see per_column) -- and not a triangle per pixel."""
    g = _gen(*_seed_of("mixed", H, W, per_view_vi, split))
    hot_c, hot_vi, hot_face, cw = _hot_grid(H, W, g)
    n_hot_v, n_hot_f = hot_c.shape[0], hot_vi.shape[0]
    y, x = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    kind = (y // WAVE_ROWS + x // K_WAVE) % 3
    own = n_hot_f + th.randperm(split * W, generator=g).view(split, W)[y % split, x]
    idx = th.empty(N, H, W, dtype=th.int64)
    for n in range(N):
        own_n = own if n == 0 else own[:, _swap_neighbours(x[0], W)]  # the second view: neighbouring columns swapped
        crowded = _crowded_tile(x, y, hot_face, own_n)
        calm = _calm_tile(x, y, hot_face, g)
        hot = _hot_tile(x, y, hot_face, cw, g)
        idx[n] = th.where(kind == 0, crowded, th.where(kind == 1, calm, hot))
    fill_vi, fill_c = _disjoint(idx - n_hot_f, split * W, H, W, g)
    vi = th.cat([hot_vi, fill_vi + n_hot_v])
    corners = th.cat([hot_c, fill_c])
    V = corners.shape[0] + 5
    ids = th.randperm(V, generator=g)[:corners.shape[0]]
    name = f"mixed {H}x{W} split {split}" + (" per-view vi" if per_view_vi else "")
    return _finish(name, H, W, g, vi, idx, V, ids, corners, per_view_vi,
                   hot_vertices=ids[:n_hot_v].tolist(), hot_triangles=list(range(n_hot_f)))


RUN_CUTS = {0: (), 1: (16, 32, 64), 2: (16, 32, 64), 3: (15, 17, 63, 64)}  # row kind (y + 2 n) mod 4 -> first pixels of its later runs
RUN_GAP = (16, 18)                                                       # row kind 2: background at x = 16 .. 17


@functools.lru_cache(maxsize=None)
def long_runs(H, W, per_view_vi=False):
    """Row kinds, (y + 2 view) mod 4: 0 -- ONE triangle over the whole width: a run spanning all 64 lanes, which the register
    scan cuts at lanes 16 / 32 / 48 and the wide kernel's sliced form at every 16th pixel (only a run's first lane looked up
    a slot there); 1 -- runs cut exactly at x = 15|16, 31|32, 63|64; 2 -- the same with a background hole at x = 16 .. 17;
    3 -- a two-pixel run over lanes 15|16, a one-pixel run at lane 63.  A triangle of its own for every run of a row kind (the
    rows of one kind share them: a vertex collects more than the one term of a one-pixel run, see per_column)."""
    g = _gen(*_seed_of("long_runs", H, W, per_view_vi))
    per_row = 1 + max(len(c) for c in RUN_CUTS.values())
    idx = th.empty(N, H, W, dtype=th.int64)
    for n in range(N):
        for y in range(H):
            kind = (y + 2 * n) % 4
            idx[n, y] = per_row * kind
            for r, c in enumerate(RUN_CUTS[kind]):
                idx[n, y, c:] = per_row * kind + r + 1
            if kind == 2:
                idx[n, y, RUN_GAP[0]:RUN_GAP[1]] = -1
    vi, corners = _disjoint(idx, per_row * len(RUN_CUTS), H, W, g)
    V = corners.shape[0] + 5
    return _finish(f"long_runs {H}x{W}" + (" per-view vi" if per_view_vi else ""), H, W, g, vi, idx, V, th.randperm(V, generator=g)[:corners.shape[0]],
                   corners, per_view_vi)


@functools.lru_cache(maxsize=None)
def one_wave(H, W, first_row=0):
    """Foreground in rows first_row .. first_row + 3 of every 16-row tile only (0: the first wave's, 12: the last wave's):
    three waves of a workgroup have nothing to scatter, and the wide table kernel keeps them for its barriers."""
    g = _gen(*_seed_of("one_wave", H, W, first_row))
    T = 20
    rows = th.stack([th.stack([_run_ids(W, T, g) for _ in range(H)]) for _ in range(N)])
    y = th.arange(H)
    keep = (y % K_TILE_ROWS >= first_row) & (y % K_TILE_ROWS < first_row + WAVE_ROWS)
    idx = th.where(keep[None, :, None], rows, th.full_like(rows, -1))
    vi, corners = _disjoint(idx, T, H, W, g)
    V = 3 * T + 5
    return _finish(f"one_wave {H}x{W} rows {first_row}..{first_row + WAVE_ROWS - 1}", H, W, g, vi, idx, V, th.randperm(V, generator=g)[:3 * T], corners,
                   first_row=first_row)


@functools.lru_cache(maxsize=None)
def repeated(H, W, per_view_vi=False):
    """Faces that name a vertex twice or three times -- [a,a,b], [a,b,a], [b,a,a], [a,a,a] -- among regular ones over 60
    vertices: two or three corners of ONE lane add to one table entry.  Even rows one face per pixel, odd rows runs of
    3 ... 5 pixels.  Not for render backward (degenerate triangles)."""
    g = _gen(*_seed_of("repeated", H, W, per_view_vi))
    Vn, F = 60, 96
    vi = th.empty(F, 3, dtype=th.int64)
    for f in range(F):
        a, b, c = th.randperm(Vn, generator=g)[:3].tolist()
        vi[f] = th.tensor([[a, b, c], [a, a, b], [a, b, c], [a, b, a], [b, a, a], [a, a, a]][f % 6])
    idx = th.empty(N, H, W, dtype=th.int64)
    for n in range(N):
        dense = th.randint(0, F, (H, W), generator=g)
        dense[th.rand(H, W, generator=g) < 0.05] = -1
        runs = th.stack([_run_ids(W, F, g) for _ in range(H)])
        idx[n] = th.where((th.arange(H) % 2 == 0)[:, None], dense, runs)
    V = Vn + 4
    return _finish(f"repeated {H}x{W}" + (" per-view vi" if per_view_vi else ""), H, W, g, vi, idx, V, th.randperm(V, generator=g)[:Vn],
                   th.rand(Vn, 3, generator=g) + 1, per_view_vi, well_shaped=False)


# ---- the restated table model: which keys a tile holds -----------------------------------------------------------------------
def faces_of(case, n):
    return case.vi[n] if case.vi.ndim == 3 else case.vi


def pixel_keys(case, key="vertex"):
    """[N,H,W,K] int64 keys of every pixel (-1 on the background): its triangle's three vertex ids, or its triangle id."""
    idx = case.idx.long()
    if key == "triangle":
        return idx[..., None]
    out = th.stack([faces_of(case, n).long()[idx[n].clamp(min=0)] for n in range(case.N)])
    return th.where((idx >= 0)[..., None], out, th.full_like(out, -1))


def tile_keys(case, key="vertex", rows=WAVE_ROWS):
    """{(view, tile row, tile column): set of the distinct keys of that 64 x `rows` tile} -- rows = 4: a wave's tile (render
    backward, the register-scan kernel, A^T A values), rows = 16: the workgroup's (the wide kernel's table)."""
    k = pixel_keys(case, key)
    out = {}
    for n in range(case.N):
        for ty in range(-(-case.H // rows)):
            for tx in range(-(-case.W // K_WAVE)):
                t = k[n, ty * rows:(ty + 1) * rows, tx * K_WAVE:(tx + 1) * K_WAVE]
                out[n, ty, tx] = set(t[t >= 0].tolist())
    return out


def must_overflow(keys, slots):
    return len(keys) > slots


def cannot_overflow(keys):
    """At most kTableProbes keys: whatever slots the others took, one of a key's kTableProbes probes is free or its own."""
    return len(keys) <= K_TABLE_PROBES


def without_key_in_tile(case, n, ty, tx, keyid, key="vertex", rows=WAVE_ROWS):
    """The index image with the pixels of one tile whose triangle has key `keyid` set to background."""
    k = pixel_keys(case, key)
    m = th.zeros_like(case.idx, dtype=th.bool)
    m[n, ty * rows:(ty + 1) * rows, tx * K_WAVE:(tx + 1) * K_WAVE] = True
    m &= (k == keyid).any(-1)
    return th.where(m, th.full_like(case.idx, -1), case.idx), int(m.sum())


# ---- inputs and references (computed once per case, shared by the tests, never modified) ----------------------------------------
@functools.lru_cache(maxsize=None)
def render_inputs(case):
    g = _gen(*_seed_of("render_inputs" + case.name))
    return th.rand(case.N, case.H, case.W, generator=g) * 2 - 1, th.rand(case.N, 3, case.H, case.W, generator=g) * 2 - 1


def render_reference(case, idx=None):
    """(float32 oracle, double oracle, accumulated magnitudes) of render backward."""
    import oracle as O

    gd, gb = render_inputs(case)
    idx = case.idx if idx is None else idx
    o32 = O.render_backward(case.v, case.vi, idx, gd, gb)
    o64 = O.render_backward(case.v.double(), case.vi, idx, gd.double(), gb.double())
    with O.accumulated_magnitudes():
        A = O.render_backward(case.v.double(), case.vi, idx, gd.double(), gb.double())
    return o32, o64, A


@functools.lru_cache(maxsize=None)
def render_reference_cached(case):
    return render_reference(case)


@functools.lru_cache(maxsize=None)
def interp_inputs(case, C):
    g = _gen(*_seed_of("interp_inputs" + case.name, C))
    return th.rand(case.N, case.V, C, generator=g), th.rand(case.N, C, case.H, case.W, generator=g) * 2 - 1


def interp_reference(case, C, idx=None, inputs=None):
    """dict a32, b32, a64, b64, aA, bA: interpolate backward's two gradients by the float32 oracle, the double oracle, and
    their accumulated magnitudes (inputs: (attr, grad_out) other than interp_inputs(case, C))."""
    import oracle as O

    attr, go = interp_inputs(case, C) if inputs is None else inputs
    idx = case.idx if idx is None else idx
    a32, b32 = O.interpolate_backward(go, attr, case.vi, idx, case.bary)
    a64, b64 = O.interpolate_backward(go.double(), attr.double(), case.vi, idx, case.bary.double())
    with O.accumulated_magnitudes():
        aA, bA = O.interpolate_backward(go.double(), attr.double(), case.vi, idx, case.bary.double())
    return dict(a32=a32, b32=b32, a64=a64, b64=b64, aA=aA, bA=bA)


@functools.lru_cache(maxsize=None)
def interp_reference_cached(case, C):
    return interp_reference(case, C)


def normal_reference(case, idx=None):
    """dict pair, nnz, v32, v64, gv, g32, g64: the A^T A pattern of the case's topology (oracle.normal_matrix_structure), its
    values by the float32 and the double oracle, a seeded gradient of the values and the bary gradient it gives."""
    import oracle as O

    idx = case.idx if idx is None else idx
    vi3 = case.vi if case.vi.ndim == 3 else case.vi[None].expand(case.N, -1, -1)
    _, col, pair = O.normal_matrix_structure(vi3, case.V)
    nnz = col.numel()
    g = _gen(*_seed_of("normal_inputs" + case.name))
    gv = th.rand(nnz, generator=g) * 2 - 1
    return dict(pair=pair.contiguous(), nnz=nnz, gv=gv,
                v32=O.normal_matrix_values(pair, idx, case.bary, nnz), v64=O.normal_matrix_values(pair, idx, case.bary.double(), nnz),
                g32=O.normal_matrix_values_backward(gv, pair, idx, case.bary),
                g64=O.normal_matrix_values_backward(gv.double(), pair, idx, case.bary.double()))


@functools.lru_cache(maxsize=None)
def normal_reference_cached(case):
    return normal_reference(case)


# ---- which case runs where (shared by the host file, which proves the properties, and the GPU file, which uses them) -----------
def build(spec):
    return globals()[spec[0]](*spec[1:])


def spec_id(spec):
    return "-".join(str(s) for s in spec)


EDGE_SHAPES = SHAPES + [THREE_TILES]
RENDER_SPECS = ([("per_column", H, W) for H, W in EDGE_SHAPES] +
                [("per_column", *DEFAULT, True), ("collide", *DEFAULT, LOG2_SLOTS, "vertex"), ("mixed", *DEFAULT, False, 1), ("mixed", *DEFAULT, True, 1),
                 ("long_runs", *DEFAULT), ("long_runs", 33, 192), ("one_wave", *DEFAULT, 0), ("one_wave", 33, 192, 12)])


# render backward in double also runs the triangle-per-pixel cases (float32: per_column, see there)
RENDER_F64_SPECS = [("per_pixel", H, W) for H, W in EDGE_SHAPES] + [("per_pixel", *DEFAULT, True), ("mixed", *DEFAULT), ("mixed", *DEFAULT, True)]


def interp_specs(log2_slots=LOG2_SLOTS, edges=False):
    """The patterns of one interpolate-backward route; `collide` with ids colliding in that route's table."""
    specs = [("per_pixel", *DEFAULT), ("collide", *DEFAULT, log2_slots, "vertex"), ("mixed", *DEFAULT), ("long_runs", *DEFAULT),
             ("one_wave", *DEFAULT, 0), ("one_wave", 33, 192, 12), ("repeated", *DEFAULT)]
    if edges:
        specs += [("per_pixel", H, W) for H, W in EDGE_SHAPES if (H, W) != DEFAULT] + [("mixed", *DEFAULT, True), ("long_runs", 33, 192), ("repeated", 5, 65, True)]
    return specs


NORMAL_SPECS = [("per_pixel", *DEFAULT), ("per_pixel", 5, 65), ("per_pixel", 33, 192), ("collide", *DEFAULT, LOG2_SLOTS, "triangle"),
                ("mixed", *DEFAULT), ("mixed", *DEFAULT, True), ("long_runs", *DEFAULT), ("repeated", *DEFAULT), ("repeated", 5, 65, True)]

# interpolate backward's routes: (C, dtype, workspace argument, kernel, takes the workgroup table)
REGISTER_SCAN = [(3, th.float32), (10, th.float32), (7, th.float64)]
WIDE_DIRECT = [16, 32, 100]
WIDE_PADDED = [13]
WIDE_TABLE = [12, 13, 20, 37, 99]
WIDE_TABLE_F64 = 12


# ---- the bounds, none of them new -------------------------------------------------------------------------------------------
def vertex_excess(got, o32, o64, A, op, what):
    """tests/f64_distance.py's element-wise bound with the operator's ulps and the floor of tests/test_gpu_f64_distance.py;
    returns (largest excess of `got`, the float32 oracle's own use of the ulps allowance)."""
    from f64_distance import assert_elementwise_within
    from test_gpu_f64_distance import ELEMENT_ULPS, FLOOR

    return assert_elementwise_within(got, o32, o64, A, ELEMENT_ULPS[op], what, floor_rel=FLOOR)


def normal_values_within(got, ref, what):
    """The fuzzers' bound of the float32 A^T A values (tests/f64_distance.py, shared with tests/fuzz_next_ops.py)."""
    from f64_distance import assert_normal_matrix_values_within

    return assert_normal_matrix_values_within(got, ref["v32"], ref["v64"], what)
