"""TEST INFRASTRUCTURE ONLY (not collected by pytest) -- random triangle soups for `rasterize_layers`: deep overdraw,
interpenetration, long runs of exact depth ties, depths at and across the 1/eps cap, screen-filling triangles between
the soup's depths, triangles culled by z or wholly off the canvas, slivers, vertices snapped to pixel centres, per-view
topology.  `capi.rasterize_layers` (K = 8) against tests/layers_oracle.py, index and depth bits, bit for bit.

usage: python tests/fuzz_layers.py [--first S] [--cases K]      random cases make_case(S) .. make_case(S + K - 1)
       python tests/fuzz_layers.py --named                      the named cases of the suite (CASES)
       python tests/fuzz_layers.py --stats                      CPU only: the oracle's figures of the named cases
       ... --lib PATH                                           against a variant build (drtk_amd/build.py --variant)

The named cases are what tests/test_gpu_rasterize_layers_soup.py runs and what tests/test_rasterize_layers_host.py
holds to the conditions the GPU tests rely on.  Their figures, from the CPU oracle with 24 layers (`--stats`):

  name          N     F  H x W    dtype  >=2 frag  >8 frag max frag   full    ties  big behind   oracle
  free          2   300  48x80    f32        85 %      0 %       12    2 %       0           0    0.1 s
  ties          1   600  40x56    f32       100 %     44 %       17   58 %    2810        4229    0.1 s
  cap32         2   500  33x47    f32        97 %      8 %       13   16 %   12904           0    0.1 s
  straddle      2   500  33x47    f32        96 %     10 %       14   18 %    4712           0    0.1 s
  cap64         2   400  50x33    f64        98 %     21 %       16   32 %   16124           0    0.1 s
  heavy_tile    1  2000  32x32    f32       100 %     96 %       24   99 %       0        3042    0.3 s
  wide          1   500  96x128   f32       100 %     91 %       24   95 %       0           0    0.3 s
  tiles64    2100    60  20x24    f32        75 %      0 %       10    0 %       0      585720    3.7 s
  heavy64     256  2000  20x449   f32       100 %     12 %       23   13 %       0       30823    1.3 s
  stack         1   400  40x56    f32       100 %    100 %       24  100 %   14359           0    0.1 s

  >=2 frag, >8 frag   pixels with that many fragments; "max frag" is the most at one pixel, at most the 24 layers kept
  full                pixels whose 8 layers are all filled
  ties                pairs of consecutive filled layers with identical depth bits, within the first 8 layers
  big behind          how often a screen-filling triangle is in a layer >= 1
  oracle              time of the oracle on one CPU thread, with its library loaded already

Per case:
  cap32, cap64   every filled depth is 1e8 / float32(1e16).
  straddle       within the first 8 layers 7 637 depths are at the cap and 8 465 below it.
  tiles64        39 % of the pixels have three layers or more.
  heavy64        only views 0, 128 and 255 hold a soup, confined to one of eight tile columns.  The percentages are over
                 the whole canvas of those three views.  Within the soup's 50 columns 90 % of the pixels have more than 8
                 fragments.
  wide           104 of the 500 triangles touch more than four 32-pixel tiles.
  stack          every depth is within 4 ulps of 2.0.  For 341 of the 400 triangles the peel cull's upper bound of the
                 depth is less than 64 ulps above that, and 289 of those are in some layer >= 1.
"""
import argparse
import functools
import os

os.environ.setdefault("DRTK_CAPI_POISON", "1")  # outputs of the ctypes binding pre-filled with NaN / sentinels (drtk_amd/capi.py _out)
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import layers_oracle as LO  # noqa: E402

DEV = "cuda:0"
K = LO.MAX_LAYERS
STAT_LAYERS = 24  # layers the oracle keeps for the statistics (the first K of them are the GPU tests' reference)
MARGIN = 5.0      # centres: uniform over the canvas and this many pixels around it

# The named cases.  Sized against these constants of drtk_amd/csrc/rasterize.hip (tests/test_rasterize_layers_host.py reads
# the numbers from the source, so a kernel change that un-targets a case shows):
#   kMaxSmallTiles = 4 (:70)           a triangle whose bbox touches more tiles goes to the per-view list of big triangles
#   kSplit4Min = 384 (:321)            a tile whose list is longer is split 2x2, longer than 4 x 384: 4x4 -- but
#   max_split_log (:537)               sub-rectangles are at least 16 px, so a 32-pixel tile is split 2x2 at the most
#   t64 >= 2048 (:339)                 N * ceil(W/64) * ceil(H/64) at or above: 64-pixel tiles, below: 32-pixel tiles
#   kCoopMin = 256 (:952)              a triangle whose bbox clipped to an item has at least that many pixels is shaded
#                                      by the whole workgroup (1024 in a tile whose list has 64 entries or more, :957)
CASES = {
    "free": dict(seed=1, N=2, F=300, H=48, W=80, scale=30.0, depth="free", per_view=True),
    "ties": dict(seed=2, N=1, F=600, H=40, W=56, scale=24.0, depth="quant", big=2),
    "cap32": dict(seed=3, N=2, F=500, H=33, W=47, scale=20.0, depth="sheets", zscale=2e8),
    "straddle": dict(seed=4, N=2, F=500, H=33, W=47, scale=20.0, depth="sheets", zscale=3e7, per_view=True),
    "cap64": dict(seed=5, N=2, F=400, H=50, W=33, scale=26.0, depth="sheets", zscale=2e16, dtype="f64"),
    # one 32-pixel tile with a list far longer than kSplit4Min.  It is split 2x2 and NOT 4x4, whatever its length:
    # max_split_log keeps sub-rectangles at 16 px or more.  The 4x4 split under peeling is heavy64's, below
    "heavy_tile": dict(seed=6, N=1, F=2000, H=32, W=32, scale=12.0, depth="free", big=3),
    "wide": dict(seed=7, N=1, F=500, H=96, W=128, scale=90.0, depth="free"),
    "tiles64": dict(seed=8, N=2100, F=60, H=20, W=24, scale=20.0, depth="free", big=1),
    # 64-pixel tiles AND a list longer than 4 x 384 in one of them (the soup is confined to the second of eight tile
    # columns): the 4x4 split, whose lower sub-rectangles lie off the canvas.  N * F is small enough for split_threshold()
    # (:323-327) to stay at kSplit4Min.  Three views of the batch hold a soup, in the others every vertex is (0, 0, 0) --
    # culled, so the oracle has nothing to do there and every layer is empty
    "heavy64": dict(seed=9, N=3, views=256, F=2000, H=20, W=449, scale=12.0, depth="free", big=2, window=(70.0, 0.0, 50.0, 20.0)),
    # Aimed at the peel cull (:1298-1313), which drops a triangle whose depth upper bound z_hi (z_upper_bound_bits, :208-219)
    # is below `near`, the nearest threshold of the 8x8 blocks it touches.  Here z_hi and `near` are as close as they get:
    # every triangle lies flat at the one depth LEVEL, so from layer 1 on `near` is LEVEL in every block that is covered
    # at all, and z_hi = LEVEL / (1 - delta) + 8 ulps with delta = 40 * 5.97e-8 * ext^2 / |den| + 2e-6, smallest for the
    # triangle of the largest area within its extent: a right isosceles one with legs L along the axes has ext = L + 2,
    # |den| = L^2.  With L >= 14, delta <= 5.2e-6, which is 43 ulps of LEVEL (2^-23 of it each): z_hi <= near + 52 or so.
    # A cull that is wrong within 64 ulps (`z_hi <= near + 64` for `z_hi < near`) empties every layer but the first
    "stack": dict(seed=10, N=1, F=400, H=40, W=56, scale=28.0, depth="level", shape="right"),
}
DTYPES = {"f32": th.float32, "f64": th.float64}
BIG_RANGE = {"free": (1.5, 4.5), "quant": (1.5, 3.5), "level": (1.5, 2.5), "sheets": (2.5, 5.5)}  # where the big triangles' depths go
QUANT_LEVELS = (1.5, 2.5, 3.5)
LEVEL = 2.0  # a power of two: the float32 just above it are the widest apart, relative to it


def make_soup(seed, N, F, H, W, scale, depth="free", zscale=1.0, dtype="f32", big=0, per_view=False, views=None, window=None, shape="any", name=None):
    """dict(v [N,3F,3], vi [F,3] or [N,F,3] int32, ...): F triangles per view, every one with three vertices of its own
    (different in every view); `big_ids`, `culled_ids`, `off_ids` [N, *]: the ids, per view, of the screen-filling
    triangles, of those with a vertex at z <= 0, and of those placed wholly off the canvas.
    With `views`: the N soups are spread over a batch of that many views (`live`: where; the dict's N is then `views`),
    whose other views hold vertices at the origin only; the per-view ids above are those of the live views, in order.
    With `window` = (x0, y0, w, h): the centres are drawn over that part of the canvas (and the margin around it)."""
    g = th.Generator().manual_seed(seed)
    f64 = th.float64
    n = F - big  # the soup proper
    assert n >= 8
    wx, wy, ww, wh = window or (0.0, 0.0, float(W), float(H))
    ctr = th.rand(N, n, 1, 2, generator=g, dtype=f64) * th.tensor([ww + 2 * MARGIN, wh + 2 * MARGIN], dtype=f64) + th.tensor([wx - MARGIN, wy - MARGIN], dtype=f64)
    if shape == "right":  # right isosceles, legs along the axes, scale/2 to scale long: the largest area an extent can hold
        leg = (0.5 + 0.5 * th.rand(N, n, 1, 1, generator=g, dtype=f64)) * scale * (th.randint(0, 2, (N, n, 1, 2), generator=g) * 2 - 1).to(f64)
        xy = ctr + th.tensor([[-0.3, -0.3], [0.7, -0.3], [-0.3, 0.7]], dtype=f64) * leg
    else:
        xy = ctr + (th.rand(N, n, 3, 2, generator=g, dtype=f64) - 0.5) * scale
    ids = th.arange(n)
    sliver = ids % 7 == 3  # the third corner 1.0001 along the first edge
    xy[:, sliver, 2] = xy[:, sliver, 0] + 1.0001 * (xy[:, sliver, 1] - xy[:, sliver, 0])
    snapped = ids % 5 == 2  # vertices on pixel centres (integer coordinates): edges through pixel centres
    xy[:, snapped] = xy[:, snapped].round()
    if depth == "free":  # every vertex its own depth: the triangles interpenetrate
        z = 1.0 + 4.0 * th.rand(N, n, 3, generator=g, dtype=f64)
    elif depth == "quant":  # one depth per triangle, of three: long runs of exact ties
        z = th.tensor(QUANT_LEVELS, dtype=f64)[th.randint(0, 3, (N, n, 1), generator=g)].expand(N, n, 3).clone()
    elif depth == "level":  # one depth for all: every layer of every pixel is decided by id alone
        z = th.full((N, n, 3), LEVEL, dtype=f64)
    elif depth == "sheets":
        z = 2.0 + th.randint(0, 4, (N, n, 1), generator=g).to(f64) + 1e-3 * th.rand(N, n, 3, generator=g, dtype=f64)
    else:
        raise ValueError(depth)
    # two triangles in the middle of the canvas with a vertex at z = 0 / z < 0: dropped whole (near plane), by both sides
    culled = [1, n // 2]
    mid = th.tensor([0.5 * W, 0.5 * H], dtype=f64)
    corners = th.tensor([[-0.3, -0.4], [0.5, -0.1], [-0.1, 0.45]], dtype=f64)
    for j, f in enumerate(culled):
        xy[:, f] = mid + corners * min(scale, 0.8 * min(H, W)) + th.rand(N, 1, 2, generator=g, dtype=f64)
        z[:, f, j] = 0.0 if j == 0 else -1.5
    # two triangles wholly off the canvas (x <= -1, x >= W), inside the margin
    off = [2, n // 2 + 1]
    for j, f in enumerate(off):
        p = th.rand(N, 3, 2, generator=g, dtype=f64) * th.tensor([MARGIN - 1.0, float(H)], dtype=f64)
        p[..., 0] += -MARGIN if j == 0 else float(W)
        xy[:, f] = p
    tri = th.cat([xy, z[..., None]], -1)  # [N, n, 3, 3]
    if big:  # screen-filling triangles between the soup's depths, slightly tilted
        s = 4.0 * max(H, W)
        lo, hi = BIG_RANGE[depth]
        bxy = th.tensor([[-s, -s], [s, -s], [0.0, s]], dtype=f64) + 3.0 * th.rand(N, big, 3, 2, generator=g, dtype=f64)
        bz = lo + (hi - lo) * (th.arange(big, dtype=f64)[None, :, None] + 1.0) / (big + 1.0) + 0.1 * th.rand(N, big, 3, generator=g, dtype=f64)
        tri = th.cat([tri, th.cat([bxy, bz[..., None]], -1)], 1)
    tri[..., 2] *= zscale
    v = tri.reshape(N, 3 * F, 3).to(DTYPES[dtype]).contiguous()
    base = th.arange(3 * F, dtype=th.int32).view(F, 3)
    # ids in another order than the vertices (shared), or in a different order in every view
    perms = th.stack([th.randperm(F, generator=g) for _ in range(N if per_view else 1)])
    vi = (base[perms] if per_view else base[perms[0]]).contiguous()
    inv = th.argsort(perms, dim=1).expand(N, F)  # inv[n, t] = id of triangle t (position in `tri`) in view n
    pick = lambda ts: inv[:, th.tensor(ts, dtype=th.long)].numpy() if ts else np.zeros((N, 0), np.int64)  # noqa: E731
    live = list(range(N))
    if views is not None:
        assert views >= N >= 2 and not per_view
        live = [round(j * (views - 1) / (N - 1)) for j in range(N)]
        full = th.zeros(views, 3 * F, 3, dtype=v.dtype)
        full[live] = v
        v, N = full, views
    return dict(
        name=name or f"seed{seed}", seed=seed, N=N, live=live, F=F, H=H, W=W, scale=scale, depth=depth, zscale=zscale, dtype=dtype, big=big,
        per_view=per_view, window=window, shape=shape, v=v, vi=vi, big_ids=pick(list(range(n, F))), culled_ids=pick(culled), off_ids=pick(off))


def named_case(name):
    return make_soup(name=name, **CASES[name])


def make_case(seed):
    """a random case of the same family (the command line's net; the suite runs the named ones)"""
    g = th.Generator().manual_seed(1000003 * seed + 17)
    r = lambda lo, hi: int(th.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    dtype = "f64" if r(0, 4) == 0 else "f32"
    depth = ("free", "quant", "sheets")[r(0, 2)]
    zscale = (1.0, 1.0, 1.0, 3e7, 2e8)[r(0, 4)] * (1e8 if dtype == "f64" and r(0, 1) else 1.0)
    return make_soup(
        seed, N=r(1, 3), F=(60, 150, 400, 900, 2000)[r(0, 4)], H=r(9, 100), W=r(9, 130), scale=(6.0, 14.0, 30.0, 90.0)[r(0, 3)],
        depth=depth, zscale=zscale, dtype=dtype, big=r(0, 3), per_view=r(0, 2) == 0)


def describe(c):
    return (f"{c['name']}: seed={c['seed']} N={c['N']}{'' if len(c['live']) == c['N'] else ' (live: %s)' % c['live']} F={c['F']} H={c['H']} W={c['W']} scale={c['scale']:g} depth={c['depth']} "
            f"zscale={c['zscale']:g} {c['dtype']} big={c['big']}{'' if c['window'] is None else ' window=%s' % (c['window'],)} vi={'per view' if c['per_view'] else 'shared'}")


def oracle_layers(c, num_layers=None):
    """(depth, index) [len(live),k,H,W] numpy of the live views, k = min(F, STAT_LAYERS) unless given"""
    whole = len(c["live"]) == c["N"]
    v = c["v"] if whole else c["v"][c["live"]].contiguous()
    vi = c["vi"] if whole or c["vi"].ndim == 2 else c["vi"][c["live"]].contiguous()
    return LO.layers(v, vi, c["H"], c["W"], num_layers or min(c["F"], STAT_LAYERS))


def whole_batch(c, depth, index):
    """the live views' layers -> the layers of all N views (the others: empty)"""
    if len(c["live"]) == c["N"]:
        return depth, index
    d = np.zeros((c["N"],) + depth.shape[1:], dtype=np.float32)
    i = np.full((c["N"],) + index.shape[1:], -1, dtype=np.int32)
    d[c["live"]], i[c["live"]] = depth, index
    return d, i


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, depth, index) of a named case (its live views), computed once per process and shared: treat as read-only"""
    c = named_case(name)
    depth, index = oracle_layers(c)
    depth.setflags(write=False)
    index.setflags(write=False)
    return c, depth, index


def statistics(c, depth, index):
    """what the oracle's layers (as many as oracle_layers keeps) say about a case"""
    filled = index >= 0
    count = filled.sum(1)  # fragments per pixel, saturating at the number of layers kept
    bits = np.ascontiguousarray(depth).view(np.uint32)
    k = min(K, index.shape[1])
    tie = filled[:, 1:k] & (bits[:, 1:k] == bits[:, :k - 1])
    big_behind = sum(int(np.isin(index[n, 1:], c["big_ids"][n]).sum()) for n in range(len(c["live"]))) if c["big"] else 0
    return dict(
        ge2=float((count >= 2).mean()), ge3=float((count >= 3).mean()), gt8=float((count > 8).mean()), most=int(count.max()),
        full=float((count >= K).mean()), ties=int(tie.sum()), big_behind=big_behind)


def first_difference(got, want, c=None):
    """None, or a line that names the first layer (then pixel, row-major) at which (depth bits, id) differ, with both keys"""
    (gd, gi), (wd, wi) = [(np.ascontiguousarray(np.asarray(d, dtype=np.float32)), np.asarray(i, dtype=np.int32)) for d, i in (got, want)]
    assert gi.shape == wi.shape and gd.shape == wd.shape, (gi.shape, wi.shape)
    gb, wb = gd.view(np.uint32), wd.view(np.uint32)
    bad = (gi != wi) | (gb != wb)
    if not bad.any():
        return None
    k = int(np.nonzero(bad.any(axis=(0, 2, 3)))[0][0])
    n, y, x = (int(a[0]) for a in np.nonzero(bad[:, k]))
    return (f"{int(bad.sum())} elements differ, {int(bad[:, k].sum())} of them in layer {k} (the first that differs); first: view {n} "
            f"y {y} x {x}: got (depth bits 0x{int(gb[n, k, y, x]):08x} = {float(gd[n, k, y, x])!r}, id {int(gi[n, k, y, x])}), "
            f"want (0x{int(wb[n, k, y, x]):08x} = {float(wd[n, k, y, x])!r}, id {int(wi[n, k, y, x])})" + (f" [{describe(c)}]" if c else ""))


def run_case(c, want=None):
    """capi.rasterize_layers with K layers against the oracle (`want` = its layers of the live views, if already at hand)"""
    from drtk_amd import capi

    if want is None:
        want = oracle_layers(c, K)
    d, i = capi.rasterize_layers(c["v"].to(DEV), c["vi"].to(DEV), c["H"], c["W"], K)
    th.cuda.synchronize()
    want = whole_batch(c, want[0][:, :K], want[1][:, :K])
    diff = first_difference((d.cpu().numpy(), i.cpu().numpy()), want, c)
    assert diff is None, diff
    return float((want[1][:, K - 1] >= 0).mean())


def stats_table():
    oracle_layers(named_case("free"), 1)  # loads the oracle's library, so that the times below are the oracle's alone
    rows = [f"  {'name':<10}{'N':>5}{'F':>6}  {'H x W':<8} {'dtype':<5}{'>=2 frag':>10}{'>8 frag':>9}{'max frag':>9}{'full':>7}{'ties':>8}{'big behind':>12}{'oracle':>9}"]
    for name in CASES:
        t0 = time.time()
        c, depth, index = reference(name)
        t = time.time() - t0
        s = statistics(c, depth, index)
        rows.append(f"  {name:<10}{c['N']:>5}{c['F']:>6}  {str(c['H']) + 'x' + str(c['W']):<8} {c['dtype']:<5}{100 * s['ge2']:>8.0f} %{100 * s['gt8']:>7.0f} %{s['most']:>9}"
                    f"{100 * s['full']:>5.0f} %{s['ties']:>8}{s['big_behind']:>12}{t:>7.1f} s")
    return "\n".join(rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--named", action="store_true")
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.stats:
        print(stats_table())
        sys.exit(0)
    if a.lib:
        from drtk_amd import capi

        capi.use_profiling_library(os.path.abspath(a.lib))
    cases = [named_case(n) for n in CASES] if a.named else [make_case(s) for s in range(a.first, a.first + a.cases)]
    bad, t0, full = 0, time.time(), []
    for c in cases:
        try:
            full.append(run_case(c))
            print(f"ok   {describe(c)}", flush=True)
        except AssertionError as e:
            bad += 1
            print(f"FAIL {describe(c)}: {str(e)[:600]}", flush=True)
    print(f"pixels with all {K} layers filled: min {min(full):.2f} max {max(full):.2f}; {time.time() - t0:.0f} s" if full else "")
    print(f"{len(cases) - bad}/{len(cases)} cases passed")
    sys.exit(1 if bad else 0)
