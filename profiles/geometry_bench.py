#!/usr/bin/env python3
"""vert_normals forward + backward, float32, 8 views: the HIP route (csrc/geometry.hip, four launches) against the
PyTorch formulation of drtk_amd/geometry.py on the same device, timed with device events after warm-up, at configs[2]'s
mesh (MESH_SIZES["100k"]) and the 1 002 528-triangle mesh (["1M"]); the algorithmic bytes of each kernel from the
shapes; and a fan with one vertex of valence 65 536 against a uniform mesh with the same F (the vertex pass's longest
row).  Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python profiles/geometry_bench.py`.

    python profiles/geometry_bench.py [--iters 50] [--json out.json]
"""
import argparse
import json
import math
import os
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drtk_amd.geometry as G  # noqa: E402
from drtk_amd import synthetic as S  # noqa: E402

DEV = "cuda:0"


def composite(x, vi):
    fn = G._face_info_torch(x, vi, {"normals"})["normals"]
    return th.nn.functional.normalize(G._face_attribute_to_vert_torch(x, vi, fn), dim=-1)


def time_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    th.cuda.synchronize()
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / iters


def step(normals, v, vi, g):
    x = v.detach().requires_grad_(True)
    normals(x, vi).backward(g)
    return x.grad


def algorithmic_bytes(N, V, F, es=4, idx=4):
    """per launch, from the shapes: what it must read and write at least once (shared [F,3] topology)"""
    inc = (V + 1) * idx + 3 * F * idx  # crow + entries
    return {
        "geom_face_forward_kernel (normals)": 3 * F * idx + N * V * 3 * es + N * F * 3 * es,
        "geom_vertex_gather_kernel (normalize)": inc + N * F * 3 * es + 2 * N * V * 3 * es,
        "geom_face_backward_kernel": 3 * F * idx + 3 * N * V * 3 * es + N * F * 9 * es,
        "geom_vertex_gather_kernel (per corner)": inc + N * F * 9 * es + N * V * 3 * es,
    }


def bench_mesh(size, iters):
    N = 8
    v0, vi = S.uv_sphere(*S.MESH_SIZES[size], lobes=0.15, device=DEV)
    v = (v0[None] * th.linspace(1, 1.5, N, device=DEV)[:, None, None]).contiguous()
    g = th.randn_like(v)
    hip = time_ms(lambda: step(G.vert_normals, v, vi, g), iters)
    comp = time_ms(lambda: step(composite, v, vi, g), max(3, iters // 5))
    F, V = vi.shape[0], v.shape[1]
    by = algorithmic_bytes(N, V, F)
    return {"mesh": size, "N": N, "V": V, "F": F, "hip_ms": hip, "composite_ms": comp, "speedup": comp / hip,
            "algorithmic_bytes": by, "total_MB": sum(by.values()) / 1e6,
            "floor_us_at_8TBps": sum(by.values()) / 8e12 * 1e6}


def bench_fan(iters, F=65536, N=8):
    ang = th.arange(F + 1, dtype=th.float64) * (2 * math.pi / F)
    ring = th.stack([th.cos(ang), th.sin(ang), 0.2 * th.sin(7 * ang)], -1)
    v0 = th.cat([th.zeros(1, 3, dtype=th.float64), ring]).float().to(DEV)
    vi = th.stack([th.zeros(F, dtype=th.long), th.arange(1, F + 1), th.arange(2, F + 2)], -1).int().to(DEV)
    v = (v0[None] * th.linspace(1, 1.5, N, device=DEV)[:, None, None]).contiguous()
    n = int(math.sqrt(F / 2))
    u0, ui = S.uv_sphere(n, F // (2 * n), device=DEV)
    u = (u0[None] * th.linspace(1, 1.5, N, device=DEV)[:, None, None]).contiguous()
    fan = time_ms(lambda: step(G.vert_normals, v, vi, th.ones_like(v)), iters)
    uni = time_ms(lambda: step(G.vert_normals, u, ui, th.ones_like(u)), iters)
    return {"fan_F": F, "uniform_F": ui.shape[0], "fan_ms": fan, "uniform_ms": uni, "fan_over_uniform": fan / uni}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"meshes": [bench_mesh(s, a.iters) for s in ("100k", "1M")], "fan": bench_fan(a.iters)}
    for m in out["meshes"]:
        print(f"[geometry] {m['mesh']}: N={m['N']} V={m['V']} F={m['F']}  HIP {m['hip_ms']:.3f} ms  composite "
              f"{m['composite_ms']:.3f} ms  ({m['speedup']:.1f}x)  algorithmic {m['total_MB']:.1f} MB, floor "
              f"{m['floor_us_at_8TBps']:.1f} us at 8 TB/s")
        for k, b in m["algorithmic_bytes"].items():
            print(f"    {k:42s} {b / 1e6:8.2f} MB  (0.4 x 8 TB/s -> {b / 3.2e12 * 1e6:7.1f} us)")
    f = out["fan"]
    print(f"[geometry] fan of valence {f['fan_F']}: {f['fan_ms']:.3f} ms; uniform F={f['uniform_F']}: "
          f"{f['uniform_ms']:.3f} ms; ratio {f['fan_over_uniform']:.2f}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
