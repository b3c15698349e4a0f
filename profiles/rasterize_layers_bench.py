#!/usr/bin/env python3
"""rasterize_layers at K = 1, 2, 4, 8 against rasterize and against K sequential rasterize calls (the same coverage work
with the bins rebuilt every time), through the C ABI with outputs and workspace allocated once, on the geometry of
BASELINE.json configs[2] (8 views, 100 352 triangles, 2048^2) and configs[4] (2 views, 1 002 528 triangles, 4096^2) as
bench.py builds them.  Every figure is the median of `--reps` single calls, each bracketed by device events, after
`--warmup` calls.  Bytes: what a call must move at least -- 8 B per pixel and layer of output, 8 B per pixel of every
layer k >= 1 for the previous layer read back as the threshold, the bins once -- against the 8 TB/s peak.
Kernel times: run it again under `rocprofv3 --kernel-trace --stats -- python profiles/rasterize_layers_bench.py`.

    python profiles/rasterize_layers_bench.py [--reps 30] [--warmup 5] [--scenes 100k,1M] [--layers 1,2,4,8] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drtk_amd import capi  # noqa: E402
from drtk_amd import synthetic as S  # noqa: E402
from drtk_amd.transform import transform  # noqa: E402

DEV = "cuda:0"
SCENES = {"100k": ("100k", 2048, 8), "250k": ("250k", 2048, 8), "1M": ("1M", 4096, 2)}
HBM_PEAK = 8e12


def scene(name):
    mesh, res, views = SCENES[name]
    v_world, vi = S.uv_sphere(*S.MESH_SIZES[mesh], lobes=0.05, device=DEV)
    campos, camrot, focal, princpt = S.ring_cameras(views, res, res, device=DEV)
    return transform(v_world[None], campos, camrot, focal, princpt).contiguous(), vi, res


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    th.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return statistics.median(times), times[len(times) // 10], times[-1 - len(times) // 10]


def bench_scene(name, reps, warmup, layer_counts=(1, 2, 4, 8)):
    v, vi, res = scene(name)
    N, F = v.shape[0], vi.shape[0]
    px = N * res * res
    ws = th.empty(capi.rasterize_workspace_bytes(N, F, res, res), dtype=th.uint8, device=DEV)
    out1 = (th.empty(N, res, res, device=DEV), th.empty(N, res, res, dtype=th.int32, device=DEV))
    bins_bytes = 28 * N * F  # ~28 B per triangle
    rows = []
    base, lo, hi = median_ms(lambda: capi.rasterize(v, vi, res, res, workspace=ws, out=out1), reps, warmup)
    rows.append({"what": "rasterize", "K": 1, "ms": base, "p10_ms": lo, "p90_ms": hi})
    for K in layer_counts:
        outk = (th.empty(N, K, res, res, device=DEV), th.empty(N, K, res, res, dtype=th.int32, device=DEV))
        ms, lo, hi = median_ms(lambda: capi.rasterize_layers(v, vi, res, res, K, workspace=ws, out=outk), reps, warmup)

        def sequential():
            for _ in range(K):
                capi.rasterize(v, vi, res, res, workspace=ws, out=out1)

        seq, _, _ = median_ms(sequential, reps, warmup) if K > 1 else (base, 0, 0)
        filled = [int((outk[1][:, k] >= 0).sum()) for k in range(K)]
        moved = 8 * px * K + 8 * px * (K - 1) + bins_bytes
        rows.append({
            "what": "rasterize_layers", "K": K, "ms": ms, "p10_ms": lo, "p90_ms": hi, "over_rasterize": ms / base,
            "sequential_rasterize_ms": seq, "over_sequential": ms / seq, "filled_px_per_layer": filled,
            "bytes_per_px_layer": moved / (px * K), "GBps": moved / (ms * 1e-3) / 1e9, "of_peak": moved / (ms * 1e-3) / HBM_PEAK,
            "us_per_layer": ms * 1e3 / K})
        del outk
    return {"scene": name, "N": N, "F": F, "res": res, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scenes", default="100k,1M")
    ap.add_argument("--layers", default="1,2,4,8", help="the K to measure (one K alone gives a kernel trace per layer count)")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert a.reps >= 20, "medians over at least 20 repetitions"
    out = [bench_scene(s, a.reps, a.warmup, [int(k) for k in a.layers.split(",")]) for s in a.scenes.split(",")]
    for sc in out:
        print(f"[layers] {sc['scene']}: {sc['N']} views x {sc['res']}^2, {sc['F']} triangles", flush=True)
        for r in sc["rows"]:
            if r["what"] == "rasterize":
                print(f"    rasterize             {r['ms']:7.3f} ms  (p10 {r['p10_ms']:.3f}, p90 {r['p90_ms']:.3f})")
            else:
                print(f"    rasterize_layers K={r['K']}  {r['ms']:7.3f} ms  (p10 {r['p10_ms']:.3f}, p90 {r['p90_ms']:.3f})  "
                      f"{r['over_rasterize']:.2f} x rasterize, {r['over_sequential']:.2f} x {r['K']} sequential rasterize "
                      f"({r['sequential_rasterize_ms']:.3f} ms); {r['bytes_per_px_layer']:.1f} B/px/layer moved at least, "
                      f"{r['GBps']:.0f} GB/s = {100 * r['of_peak']:.1f} % of 8 TB/s; filled px per layer {r['filled_px_per_layer']}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
