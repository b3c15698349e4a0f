"""The index images of tests/scatter_table_cases.py have the properties tests/test_gpu_scatter_tables.py relies on -- tables
that must overflow, probe chains that must run out in a nearly empty table, a vertex in a tile that overflows and in one
that cannot, runs cut at the named lanes, tiles with one wave's rows -- decided from the restated table model alone, whatever
order the lanes insert in; the constants of that model are the sources'; the references are finite, non-zero and within
their own bounds; and the bounds reject a vertex that lost one wave tile's contributions (no GPU)."""
import pytest
import torch as th

import scatter_table_cases as P

WAVE, GROUP = P.WAVE_ROWS, P.K_TILE_ROWS
# (tile rows, log2 slots, key) of every table the cases are run through: the wave tables of render backward, of the
# register-scan kernel and (keyed by triangle) of the A^T A values kernel; the wide kernel's workgroup table at every size
TABLES = [(WAVE, P.LOG2_SLOTS, "vertex"), (WAVE, P.LOG2_SLOTS, "triangle")] + [(GROUP, P.wide_log2_slots(C), "vertex") for C in P.WIDE_TABLE]
TABLE_IDS = [f"{r}rows-{1 << s}slots-{k}" for r, s, k in TABLES]


def test_the_constants_are_the_sources():
    assert (P.K_TABLE_SLOTS, P.K_TABLE_PROBES, P.K_TILE_ROWS, P.K_WAVE, P.K_BLOCK, P.WAVE_ROWS) == (64, 6, 16, 64, 256, 4)
    assert P.TABLE_BYTES == 12800 and P.HASH_MULTIPLIER == 2654435761
    assert P.home_slot(1, 6) == (2654435761 >> 26) and P.home_slot(0, 7) == 0
    with pytest.raises(RuntimeError):
        P._constant("segscatter.hpp", r"constexpr\s+int\s+kNoSuchTable\s*=\s*(\d+)\s*;")


def test_the_wide_tables_size_rule():
    assert [P.wide_log2_slots(C) for C in (12, 20, 37, 99, 100)] == [7, 6, 5, 4, 3]
    assert P.wide_log2_slots(13) == 6  # (8 * 13 + 4) * 128 = 13824 bytes: one over
    assert all(P.wide_takes_table(C) for C in P.WIDE_TABLE) and not any(P.wide_takes_table(C) for C in P.WIDE_DIRECT)
    assert P.wide_takes_table(P.WIDE_TABLE_F64, 8) and not P.wide_takes_table(8, 8)
    # the register-scan kernel keeps C <= 10 (float) / 7 (double): every wide case lies above
    assert max(C for C, dt in P.REGISTER_SCAN if dt == th.float32) == P.SMALL_MAXC_F32 < min(P.WIDE_TABLE + P.WIDE_DIRECT + P.WIDE_PADDED)
    assert max(C for C, dt in P.REGISTER_SCAN if dt == th.float64) == P.SMALL_MAXC_F64 < P.WIDE_TABLE_F64 and P.WIDE_TABLE_F64 % 4 == 0


@pytest.mark.parametrize("rows,log2_slots,key", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("shape", P.EDGE_SHAPES, ids=str)
def test_per_pixel_overflows_the_table(shape, rows, log2_slots, key):
    if (rows, key) == (WAVE, "vertex"):  # render backward's stand-in: a triangle per column
        col = P.per_column(*shape)
        assert shape == (1, 1) or max(len(k) for k in P.tile_keys(col, key, rows).values()) > 1 << log2_slots
        assert bool(((col.idx[:, :, 1:] != col.idx[:, :, :-1]) | (col.idx[:, :, 1:] == -1)).all()), "every pixel a run of its own"
    case = P.per_pixel(*shape)
    most = max(len(k) for k in P.tile_keys(case, key, rows).values())
    print(f"{case.name}: at most {most} distinct {key} keys in a 64 x {rows} tile, {1 << log2_slots} slots")
    if shape == (1, 1):
        assert most == (3 if key == "vertex" else 1)  # one pixel: the smallest launch, nothing to overflow
    else:
        assert most > 1 << log2_slots


@pytest.mark.parametrize("rows,log2_slots,key", TABLES, ids=TABLE_IDS)
def test_collide_exhausts_the_probes_of_a_nearly_empty_table(rows, log2_slots, key):
    case = P.collide(*P.DEFAULT, log2_slots, key)
    assert len({P.home_slot(k, log2_slots) for k in case.pool}) == 1 and len(set(case.pool)) == len(case.pool) > P.K_TABLE_PROBES
    tiles = P.tile_keys(case, key, rows)
    full = [k for k in tiles.values() if len(k & set(case.pool)) >= P.K_TABLE_PROBES + 1]
    print(f"{case.name}: {len(case.pool)} keys of home slot {P.home_slot(case.pool[0], log2_slots)}; "
          f"{len(full)} of {len(tiles)} tiles hold more than {P.K_TABLE_PROBES} of them")
    assert len(full) >= len(tiles) // 2
    assert all(len(k) <= (1 << log2_slots) // 2 for k in tiles.values())
    runs = (case.idx[:, :, 1:] != case.idx[:, :, :-1]).sum().item() + case.N * case.H
    assert 3 <= case.idx.numel() / runs <= 5


# (split = 1, one triangle of its own per column, is render backward's variant: vertex keys, wave tiles)
@pytest.mark.parametrize("rows,log2_slots,key,per_view_vi,split", [(*t, pv, 2) for t in TABLES for pv in (False, True)] + [(*TABLES[0], pv, 1) for pv in (False, True)],
                         ids=lambda v: str(v))
def test_mixed_has_a_hot_key_in_a_tile_that_overflows_and_in_one_that_cannot(rows, log2_slots, key, per_view_vi, split):
    case = P.mixed(*P.DEFAULT, per_view_vi, split)
    tiles = P.tile_keys(case, key, rows)
    over = [k for k in tiles.values() if P.must_overflow(k, 1 << log2_slots)]
    calm = [k for k in tiles.values() if k and P.cannot_overflow(k)]
    hot = case.hot_vertices if key == "vertex" else case.hot_triangles
    both = [h for h in hot if any(h in k for k in over) and any(h in k for k in calm)]
    print(f"{case.name}, {key} keys, 64 x {rows} tiles of {1 << log2_slots} slots: {len(over)} overflow, {len(calm)} cannot, {len(both)} hot keys in both")
    assert over and calm and both
    assert len(case.hot_vertices) == 40 and sum(h in set().union(*tiles.values()) for h in case.hot_vertices) >= (30 if key == "vertex" else 0)


@pytest.mark.parametrize("shape", [P.DEFAULT, (33, 192)], ids=str)
def test_long_runs_are_cut_where_they_say(shape):
    case = P.long_runs(*shape)
    idx = case.idx
    seen = set()
    for n in range(case.N):
        for y in range(case.H):
            kind = (y + 2 * n) % 4
            cuts = [c for c in P.RUN_CUTS[kind] if c < case.W]
            row = idx[n, y]
            heads = set((1 + (row[1:] != row[:-1]).nonzero().flatten()).tolist())
            want = set(cuts) | ({P.RUN_GAP[0], P.RUN_GAP[1]} if kind == 2 else set())
            assert heads == want, (n, y, kind, sorted(heads))
            if kind == 0:
                assert int(row.min()) == int(row.max()) >= 0  # one run over all 64 lanes of every tile of the row
            if kind == 2:
                assert bool((row[P.RUN_GAP[0]:P.RUN_GAP[1]] == -1).all()) and int((row == -1).sum()) == P.RUN_GAP[1] - P.RUN_GAP[0]
            seen.add(kind)
    assert seen == {0, 1, 2, 3}
    assert {15, 16, 17, 32, 63, 64} <= {c for cuts in P.RUN_CUTS.values() for c in cuts} | set(P.RUN_GAP)
    assert P.faces_of(case, 0).unique().numel() == 3 * case.F  # every run of a row a triangle with vertices of its own


@pytest.mark.parametrize("shape,first_row", [(P.DEFAULT, 0), ((33, 192), 12)], ids=str)
def test_one_wave_leaves_three_waves_of_a_tile_without_foreground(shape, first_row):
    case = P.one_wave(*shape, first_row)
    fg = case.idx >= 0
    whole = 0
    for n in range(case.N):
        for ty in range(-(-case.H // GROUP)):
            for tx in range(-(-case.W // P.K_WAVE)):
                t = fg[n, ty * GROUP:(ty + 1) * GROUP, tx * P.K_WAVE:(tx + 1) * P.K_WAVE]
                groups = [bool(t[r:r + WAVE].any()) for r in range(0, t.shape[0], WAVE)]
                if t.shape[0] > first_row:  # the tile has the rows: exactly that wave has foreground
                    assert groups == [r == first_row // WAVE for r in range(len(groups))], (n, ty, tx, groups)
                    whole += 1
                else:                       # (the canvas ends above them: a tile of background)
                    assert not any(groups)
    assert whole >= case.N * -(-case.W // P.K_WAVE)


def test_repeated_faces_name_a_vertex_twice_and_three_times():
    for case in (P.repeated(*P.DEFAULT), P.repeated(5, 65, True)):
        used = P.faces_of(case, 0).long()[case.idx[case.idx >= 0].unique().long()]
        distinct = th.tensor([row.unique().numel() for row in used])
        assert {1, 2, 3} == set(distinct.tolist())
        two = used[distinct == 2]
        assert bool((two[:, 0] == two[:, 1]).any()) and bool((two[:, 0] == two[:, 2]).any()) and bool((two[:, 1] == two[:, 2]).any())
        rows = case.idx[0]
        assert float((rows[0::2, 1:] != rows[0::2, :-1]).float().mean()) > 0.9 > 0.4 > float((rows[1::2, 1:] != rows[1::2, :-1]).float().mean())


def test_shapes_cover_the_tile_counts_and_ragged_edges():
    tiles = sorted({-(-H // GROUP) * -(-W // P.K_WAVE) for H, W in P.EDGE_SHAPES})
    assert tiles == [1, 2, 3, 6, 9]
    assert any(W % P.K_WAVE for _, W in P.EDGE_SHAPES)
    assert any(H % GROUP and H % WAVE for H, _ in P.EDGE_SHAPES) and any(H % GROUP and not H % WAVE for H, _ in P.EDGE_SHAPES)
    for spec in P.RENDER_SPECS + P.RENDER_F64_SPECS + P.interp_specs(edges=True) + P.NORMAL_SPECS:
        case = P.build(spec)
        assert case.N == 2 and case.idx.dtype == th.int32 and case.vi.dtype == th.int32 and (case.vi.ndim == 3) == case.per_view_vi
        used = th.zeros(case.V, dtype=th.bool)
        for n in range(case.N):
            used[P.faces_of(case, n).long()[case.idx[n][case.idx[n] >= 0].long()].flatten()] = True
        assert not bool(used.all()), f"{case.name}: some vertex must be referenced by no pixel"
        assert float((case.bary.sum(1) - 1).abs().max()) < 1e-6 and float(case.bary.min()) > 0
    for specs in (P.RENDER_SPECS, P.interp_specs(edges=True), P.NORMAL_SPECS):
        assert any(P.build(s).per_view_vi for s in specs) and not all(P.build(s).per_view_vi for s in specs)


# ---- references ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", P.RENDER_SPECS, ids=P.spec_id)
def test_render_reference_is_sane_and_within_its_own_bound(spec):
    case = P.build(spec)
    assert case.well_shaped
    o32, o64, A = P.render_reference_cached(case)
    assert bool(th.isfinite(o64).all()) and float(o64.abs().max()) > 0
    excess, own = P.vertex_excess(o32, o32, o64, A, "render", case.name)
    print(f"{case.name}: max|f64| = {float(o64.abs().max()):.3e}; the float32 oracle uses {own:.2f} of the ulps allowance (excess {excess:.2f})")
    assert own <= 0.5, "the float32 oracle needs the bound's allowance for itself: the case's scale decides, not the summation -- change the inputs"


@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("spec", P.interp_specs(edges=True), ids=P.spec_id)
def test_interpolate_reference_is_sane_and_within_its_own_bound(spec, C):
    case = P.build(spec)
    r = P.interp_reference_cached(case, C)
    for k in ("a64", "b64"):
        assert bool(th.isfinite(r[k]).all()) and float(r[k].abs().max()) > 0
    excess, own = P.vertex_excess(r["a32"], r["a32"], r["a64"], r["aA"], "interpolate", case.name)
    print(f"{case.name} C={C}: max|f64| = {float(r['a64'].abs().max()):.3e}; the float32 oracle uses {own:.2f} of the ulps allowance")
    assert float((r["b32"].double() - r["b64"]).abs().max()) <= 1e-6 * float(r["b64"].abs().max())
    assert own <= 2.0


@pytest.mark.parametrize("spec", P.NORMAL_SPECS, ids=P.spec_id)
def test_normal_matrix_reference_is_sane_and_within_its_own_bound(spec):
    case = P.build(spec)
    r = P.normal_reference_cached(case)
    for k in ("v64", "g64"):
        assert bool(th.isfinite(r[k]).all()) and float(r[k].abs().max()) > 0
    err, own = P.normal_values_within(r["v32"], r, case.name)
    print(f"{case.name}: nnz = {r['nnz']}, max|f64| = {float(r['v64'].abs().max()):.3e}, |oracle_f32 - f64| = {own:.3e}")
    assert float((r["g32"].double() - r["g64"]).abs().max()) <= 1e-5 + 1e-5 * float(r["g64"].abs().max())


# ---- sensitivity --------------------------------------------------------------------------------------------------------------
def _lost_tile(case, key, hot):
    """A wave tile that must overflow and holds hot key `hot`, and the index image without that key's pixels in it."""
    for (n, ty, tx), keys in sorted(P.tile_keys(case, key, WAVE).items()):
        if hot in keys and P.must_overflow(keys, P.K_TABLE_SLOTS):
            idx, count = P.without_key_in_tile(case, n, ty, tx, hot, key, WAVE)
            assert count > 0
            return (n, ty, tx), idx, count
    return None


@pytest.mark.parametrize("op", ["render", "interpolate"])
def test_the_bound_sees_a_hot_vertex_that_lost_one_wave_tiles_contributions(op):
    """The double oracle's own result with the contributions of ONE overflowing wave tile's pixels to ONE hot vertex removed
    (recomputed with those pixels as background) must fail the element-wise bound at that vertex -- what a fallback that
    drops, or a table that forgets, a key would produce.  These losses are gross (1e3 ... 1e6 x the element's bound, and
    visible to the max-norm bound of tests/f64_distance.py as well: the count is printed); the loss that ONLY the
    element-wise bound sees is the next test's."""
    from f64_distance import elementwise_excess, f64_distance_bound
    from test_gpu_f64_distance import ELEMENT_ULPS, FLOOR

    case = P.mixed(*P.DEFAULT, False, 1 if op == "render" else 2)
    if op == "render":
        o32, o64, A = P.render_reference_cached(case)
        lost = lambda idx: P.render_reference(case, idx)[1]  # noqa: E731
    else:
        r = P.interp_reference_cached(case, 3)
        o32, o64, A = r["a32"], r["a64"], r["aA"]
        lost = lambda idx: P.interp_reference(case, 3, idx)["a64"]  # noqa: E731
    assert elementwise_excess(o64, o32, o64, A, ELEMENT_ULPS[op], floor_rel=FLOOR)[0] <= 1.0
    blind = 0
    found = [(hot, t) for hot in case.hot_vertices for t in [_lost_tile(case, "vertex", hot)] if t is not None][:8]
    assert len(found) == 8
    for hot, ((n, ty, tx), idx, count) in found:
        mutated = o64.clone()
        mutated[:, hot] = lost(idx)[:, hot]
        assert bool((mutated[n, hot] != o64[n, hot]).any()) and th.equal(mutated[1 - n], o64[1 - n])
        excess, worst, _ = elementwise_excess(mutated.float(), o32, o64, A, ELEMENT_ULPS[op], floor_rel=FLOOR)
        assert excess > 1.0 and worst // o64.shape[-1] == n * case.V + hot, f"{op}: vertex {hot} lost {count} pixels of tile {(n, ty, tx)} and passes"
        bound, _ = f64_distance_bound(o32, o64)
        gone = float((mutated - o64).abs().max())
        if gone <= bound:
            blind += 1
        print(f"{op}: vertex {hot} without {count} pixels of wave tile {(n, ty, tx)}: off by {gone:.3e} = {excess:.0f} x its bound; max-norm bound {bound:.3e}")
    print(f"{op}: {blind} of 8 losses would pass the max-norm bound")


def test_the_elementwise_bound_sees_a_small_vertex_whose_only_atomic_was_lost():
    """tests/test_gpu_f64_distance.py's test_the_elementwise_bound_sees_a_small_vertex_that_lost_a_contribution, on these
    inputs: in per_pixel every element of interpolate backward's attribute gradient is ONE term, added by a direct global
    atomic wherever the wave tile's table was full (every tile's is), and a few of them are small -- above 20 x the floor,
    below what the max-norm bar resolves.  The element with the smallest such accumulated magnitude loses half of it: the
    max-norm bound of tests/f64_distance.py still passes (the blind spot), the element-wise bound fails at that element.
    (Render backward's cases offer no such element -- their smallest accumulated magnitude is 0.02 against a window that
    ends near 1e-4 -- so the demonstration is interpolate's.)"""
    from f64_distance import elementwise_excess, f64_distance_bound
    from test_gpu_f64_distance import ELEMENT_ULPS, FLOOR

    case, C = P.per_pixel(33, 192), 20
    assert all(P.must_overflow(k, P.K_TABLE_SLOTS) for k in P.tile_keys(case, "vertex", WAVE).values())
    r = P.interp_reference_cached(case, C)
    o32, o64, A, ulps = r["a32"], r["a64"], r["aA"], ELEMENT_ULPS["interpolate"]
    Af, scale = A.double().flatten(), float(o64.abs().max())
    cand = th.where((Af > 20 * FLOOR * scale) & (Af < 0.2 * 1e-5 * scale / 0.5), Af, th.full_like(Af, float("inf")))
    i = int(cand.argmin())
    assert bool(th.isfinite(cand[i])), "no low-magnitude element on this case: pick another"
    got = o32.clone()
    assert elementwise_excess(got, o32, o64, A, ulps, floor_rel=FLOOR)[0] <= 1.0
    g = got.flatten()
    g[i] = g[i] - 0.5 * float(Af[i]) * (1.0 if float(o64.flatten()[i]) >= 0 else -1.0)
    bound, _ = f64_distance_bound(o32, o64)
    assert float((got.double() - o64).abs().max()) <= bound, "the mutation is visible to the max-norm bound already"
    excess, worst, _ = elementwise_excess(got, o32, o64, A, ulps, floor_rel=FLOOR)
    print(f"element {i}: accumulated {float(Af[i]):.3e} of max|f64| = {scale:.3e}; max-norm bound {bound:.3e} passes, element-wise excess {excess:.1f}")
    assert excess > 1.0 and worst == i


@pytest.mark.parametrize("spec", P.RENDER_F64_SPECS, ids=P.spec_id)
def test_render_reference_of_the_double_only_cases_is_sane(spec):
    case = P.build(spec)
    _, o64, _ = P.render_reference_cached(case)
    assert case.well_shaped and bool(th.isfinite(o64).all()) and float(o64.abs().max()) > 0


def test_the_normal_matrix_bound_sees_a_triangle_that_lost_one_wave_tiles_contributions():
    from f64_distance import f64_distance_bound

    case = P.mixed(*P.DEFAULT)
    r = P.normal_reference_cached(case)
    hot = next(h for h in case.hot_triangles if any(h in k and P.must_overflow(k, P.K_TABLE_SLOTS) for k in P.tile_keys(case, "triangle", WAVE).values()))
    _, idx, count = _lost_tile(case, "triangle", hot)
    mutated = P.normal_reference(case, idx)["v64"]
    changed = (mutated != r["v64"]).nonzero().flatten()
    assert 6 <= changed.numel() <= 9  # the triangle's entries of A^T A (its three diagonal ones and the pairs, both ways)
    P.normal_values_within(r["v64"], r, case.name)
    with pytest.raises(AssertionError):
        P.normal_values_within(mutated.float(), r, case.name)
    acc = float(r["v64"].abs().max())
    bound = f64_distance_bound(r["v32"], r["v64"], acc_magnitude=acc)[0]
    print(f"triangle {hot} without {count} pixels: off by {float((mutated - r['v64']).abs().max()):.3e}, bound {bound:.3e}")
