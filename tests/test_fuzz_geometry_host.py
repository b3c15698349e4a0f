"""CPU: tests/fuzz_geometry.py, seeds 0 .. 239 (tests/test_gpu_fuzz_geometry.py), from the drawn numbers and the inputs made
from them on the CPU: the 240 seeds hold the crossings the fuzzer is for, every draw meets the four conditions its bounds
rest on -- otherwise the GPU test would pass by accident of the draw --, the constants the "near" lists are made of are the
kernels', and every case passes its own comparison code against the CPU formulation."""
import collections
import functools
import os
import re

import torch as th
from conftest import ROOT

import fuzz_geometry as F

PER_BLOCK, BLOCKS = 40, 6  # those of tests/test_gpu_fuzz_geometry.py (asserted below)


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(F.make_case(seed) for seed in range(PER_BLOCK * BLOCKS))


def all_runs():
    return [run for c in cases() for run in F.runs(c)]


def longest_row(idx, rows):
    """the most (face, corner) entries a row of the incidence of idx ([F,3] or [B,F,3]) over `rows` vertices has"""
    t = idx.long() if idx.dim() == 3 else idx.long()[None]
    return max(int(th.bincount(b.reshape(-1), minlength=rows).max()) for b in t)


def test_the_near_lists_follow_the_kernels():
    header = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    common = open(os.path.join(ROOT, "drtk_amd", "csrc", "common.hpp")).read()
    kernels = open(os.path.join(ROOT, "drtk_amd", "csrc", "geometry.hip")).read()
    from drtk_amd import capi

    assert int(re.search(r"#define\s+DRTK_GEOMETRY_CHUNK\s+(\d+)", header).group(1)) == F.CHUNK == capi.GEOMETRY_CHUNK
    assert int(re.search(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", common).group(1)) == F.BLOCK
    assert "constexpr int kChunk = DRTK_GEOMETRY_CHUNK;" in kernels and "grid_1d(N * F), dim3(kBlock)" in kernels and "grid_1d(N * V), dim3(kBlock)" in kernels
    assert F.NEAR_VALENCE == (F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 300, 2 * F.CHUNK - 1, 2 * F.CHUNK, 2 * F.CHUNK + 1)
    assert F.NEAR_LANES == (F.BLOCK - 1, F.BLOCK, F.BLOCK + 1, 2 * F.BLOCK - 1, 2 * F.BLOCK, 2 * F.BLOCK + 1)


def test_the_cases_are_seeded_plain_numbers():
    import test_gpu_fuzz_geometry as G

    assert (G.PER_BLOCK, G.BLOCKS) == (PER_BLOCK, BLOCKS) and len(cases()) == 240
    F.make_case.cache_clear()
    assert list(cases()) == [F.make_case(seed) for seed in range(240)]  # seeded

    def plain(v):
        return all(plain(e) for e in v) if isinstance(v, tuple) else v is None or isinstance(v, (bool, int, float, str))

    for c in cases():
        assert all(plain(v) for v in c.values()), c
        assert F.describe(c).startswith(f"seed={c['seed']} attempt={c['attempt']}") and 0 <= c["attempt"] < F.MAX_ATTEMPTS
        assert c == F.draw(c["seed"], c["attempt"])
        assert all(F.missed_condition(F.draw(c["seed"], a)) is not None for a in range(c["attempt"])), c  # the first that meets them


def test_what_the_240_seeds_hold():
    drawn, runs = cases(), all_runs()
    assert len(runs) >= 200  # every run goes through all six functions (fuzz_geometry.apply): each of them at least 200 times
    keys = collections.Counter(k for run in runs for k in F.oracles(run)[0])
    for name in ("face_info_grad_v", "vert_normals", "vert_normals_fnorms", "face_attribute_to_vert", "face_dpdt", "vert_binormals"):
        assert keys[name] >= (100 if name == "face_info_grad_v" else 200), (name, keys[name])
    uv = collections.Counter(c["uv"] for c in drawn)
    assert set(uv) == set(F.UV) and min(uv.values()) >= 30, uv
    chunked_few, chunked_A, lanes_f, lanes_v = 0, set(), set(), set()
    for run in runs:
        t = F.inputs(run)
        N, V, F_, T = run["N"], t["v"].shape[1], t["vti"].shape[0], t["vt"].shape[1]
        assert t["v"].shape == (N, V, 3) and t["vt"].shape == (N, T, 2) and t["vi"].shape[-2:] == (F_, 3) and t["vi_shared"].shape == (F_, 3)
        assert t["attr"].shape == (N, F_, run["A"]) and 1 <= N <= 4 and 1 <= run["A"] <= 9
        for k in ("vi", "vi_shared", "vti"):
            assert str(t[k].dtype) == "torch." + run["vi_dtype"] and 0 <= int(t[k].min()) and int(t[k].max()) < (T if k == "vti" else V)
        if run["dtype"] == "f32":
            assert all(th.equal(x, x.float().double()) for x in t.values() if x.is_floating_point())
        assert (t["vi"].dim() == 3 and t["vi"].shape[0] > 1 and t["vi"].stride(0) == 0) == (run["topology"] == "NF3_expand" and N > 1)
        same_lists = t["vi"].dim() == 2 or all(th.equal(t["vi"][n], t["vi_shared"]) for n in range(t["vi"].shape[0]))
        assert same_lists == (run["topology"] != "NF3"), run
        assert {"same": T == V and th.equal(t["vti"], t["vi_shared"]), "seam": T > V, "corners": T == 3 * F_, "few": 3 <= T <= 6}[run["uv"]], run
        uv_row, pos_row = longest_row(t["vti"], T), longest_row(t["vi"], V)
        if run["uv"] == "few" and F_ >= 500:
            chunked_few += uv_row > F.CHUNK
        if uv_row > F.CHUNK:
            chunked_A.add(2)
        if pos_row > F.CHUNK:
            chunked_A.add(run["A"])
        if run["mesh"] == "fan":
            assert pos_row == run["valence"] + int(run["degenerate"]), run  # (the duplicate-corner face holds vertex 0 too)
        lanes_f.add(N * F_)
        lanes_v.add(N * V)
    assert sum(c["uv"] == "few" and F.inputs(F.runs(c)[0])["vti"].shape[0] >= 500 for c in drawn) >= 30  # one case in eight
    assert chunked_few >= 20, chunked_few
    assert {1, 2, 5, 9} <= chunked_A, chunked_A
    assert set(F.NEAR_LANES) <= lanes_f and set(F.NEAR_LANES) <= lanes_v, (sorted(lanes_f & set(F.NEAR_LANES)), sorted(lanes_v & set(F.NEAR_LANES)))
    assert set(F.NEAR_VALENCE) <= {run["valence"] for run in runs if run["mesh"] == "fan"}
    assert sum(c["topology"] == "NF3" for c in drawn) >= 30
    for key, values in (("vi_dtype", ("int32", "int64")), ("dtype", ("f32", "f64")), ("layout", F.LAYOUTS), ("topology", F.TOPOLOGY),
                        ("mesh", set(F.MESHES)), ("N", (1, 2, 3, 4)), ("degenerate", (False, True))):
        assert {c[key] for c in drawn} == set(values), key
    assert any(c["degenerate"] and c["topology"] == "NF3" for c in drawn)
    for names, key in ((F.NEEDS, "needs"), (F.KINDS, "kinds"), (F.KINDS, "upstream")):
        for name in names:
            assert {name in c[key] for c in drawn} == {False, True}, (key, name)
        assert all(c[key] for c in drawn)
    assert all(set(c["upstream"]) <= set(c["kinds"]) for c in drawn)


def test_every_draw_meets_the_four_conditions():
    """(a) .. (d) of fuzz_geometry's docstring, from the CPU formulation alone, written out again here"""
    import drtk_amd.geometry as G
    import test_gpu_geometry as T

    for run in all_runs():
        t = F.inputs(run)
        N, V = t["v"].shape[:2]
        for k in ("vi", "vi_shared"):
            two_area = 2 * G.face_info(t["v"], t[k], ["areas"])[..., 0]
            assert not bool(((two_area > 0) & (two_area < 1e-6)).any()), ("a", run)
        det, scale = F.uv_determinants(t)
        assert bool((det >= 1e-3 * scale).all()), ("b", run)
        faces, verts = F.degenerate_sets(run, t)
        assert faces.shape == (N, t["vi"].shape[-2]) and verts.shape == (N, V)
        assert th.equal(faces, 2 * G.face_info(t["v"], t["vi"], ["areas"])[..., 0] == 0), ("a", run)  # exactly degenerate
        assert int(faces.sum()) == (2 * N if run["degenerate"] else 0), ("d", run)
        assert float(faces.double().mean(1).max()) <= 0.02 and float(verts.double().mean(1).max()) <= 0.10, ("d", run)
        o64, o32 = F.oracles(run)
        assert (o32 is not None) == (run["dtype"] == "f32")
        for k, ref in o64.items():
            assert bool(th.isfinite(ref).all()), (k, run)
            name, f, vs = F.sets_of(k, ref, faces, verts)
            kept, apart = T._split(name, ref, f, vs)
            if name in T._VERT_C:
                assert kept.numel() >= 0.9 * ref.numel(), ("d", k, run)
            if o32 is not None and kept.numel():
                own = float((T._split(name, o32[k].double(), f, vs)[0] - kept).abs().max())
                assert 3 * own <= 1e-3 * float(kept.abs().max()), ("c", k, own, run)


def test_every_case_passes_its_own_comparison_on_the_cpu():
    """run_case with the device replaced by the CPU formulation in float64: the comparison code on every seed"""
    for c in cases():
        try:
            F.run_case(c, dev="cpu")
        except AssertionError as e:
            raise AssertionError(f"{F.describe(c)}: {e}") from e
