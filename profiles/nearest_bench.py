#!/usr/bin/env python3
"""drtk_amd.nearest_points (forward, and forward + backward to both point sets), float32, 8 views, four shapes of a
registration step -- mesh against mesh, a head-model-sized mesh against a scan and the reverse, scan against scan -- on the
HIP route (csrc/nearest.hip) next to the loop users write today, on the same card in the same run:

  cdist loop   under no_grad, chunks of queries against all targets: `torch.cdist(p[:, i0:i1], q).min(-1)`, the chunk sized so
               that one [N, chunk, M] float32 distance block is `--block-gib` GiB (stated in the output); then, for the
               backward, the distance formed again from the gathered targets, differentiably (the gather's backward is an
               index_add with float atomics).  Its indices differ from the definition's where cdist's matrix-multiply form
               rounds differently; the share of equal indices is reported.

Whole calls are timed with device events after warm-up, alternating HIP and the loop, `--rounds` windows each; reported
are the median and the spread (min ... max) of the windows, and pairs per second (N * P * M over the median).  Then each
kernel's time from the library's own timing collection, the forward kernel's pairs per second and its share of the VALU
issue peak: 256 CUs x 4 SIMDs x one wave64 instruction per 2 cycles at 2.4 GHz = 1228.8 G wave-instructions/s; the float32
inner loop spends VALU_PER_PAIR vector instructions per pair and lane (counted off the kernel's disassembly, see below), so
the peak is 1228.8e9 * 64 / VALU_PER_PAIR pairs/s.

One process per shape, each under its own time limit, the next only if the one before ended well:

    for c in mesh_mesh mesh_scan scan_mesh scan_scan; do timeout -k 10 240 python profiles/nearest_bench.py --case $c || break; done
"""
import argparse
import os
import statistics
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drtk_amd  # noqa: E402
from drtk_amd import capi  # noqa: E402

DEV = "cuda:0"
N = 8
CASES = {"mesh_mesh": (16384, 16384), "mesh_scan": (5023, 100000), "scan_mesh": (100000, 5023), "scan_scan": (100000, 100000)}
# The float32 forward kernel's inner loop (hipcc --save-temps, gfx950): a group of 8 targets against a lane's 4 queries, 32
# pairs, is 80 v_pk_add_f32 + 48 v_pk_mul_f32 + 12 v_min3_f32 + 4 v_min_f32 + 4 v_cmp_lt_f32 + 9 v_mov_b32 = 157 vector
# instructions (plus 8 ds_read_b96 and the scalar loop control); the rescan of a group that improves some query is not counted.
VALU_PER_PAIR = 157 / 32
VALU_ISSUE = 256 * 4 * 2.4e9 / 2  # wave-instructions per second


def _window_ms(fn, iters):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b)


def windows(fns, window_ms, rounds, warmup=2):
    """{name: [ms per call of each window]}, the functions alternating; windows of about `window_ms` sized from a probe"""
    iters = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        th.cuda.synchronize()
        iters[k] = max(1, min(2000, int(window_ms / max(_window_ms(fn, 1), 1e-3))))
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(_window_ms(fn, iters[k]) / iters[k])
    return out


def cdist_loop(p, q, chunk):
    """(dist2, idx) the way it is written today; differentiable in p and q through the gather"""
    with th.no_grad():
        idx = th.empty(p.shape[0], p.shape[1], dtype=th.int64, device=p.device)
        for i0 in range(0, p.shape[1], chunk):
            idx[:, i0:i0 + chunk] = th.cdist(p[:, i0:i0 + chunk], q).min(-1).indices
    chosen = th.gather(q, 1, idx[..., None].expand(-1, -1, 3))
    return (p - chosen).square().sum(-1), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=list(CASES), required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--block-gib", type=float, default=2.0)
    a = ap.parse_args()
    P, M = CASES[a.case]
    pairs = N * P * M
    gen = th.Generator().manual_seed(1)
    # a scan of a unit-sized object and a mesh near it: the state of a fit that is under way
    q = th.randn(N, M, 3, generator=gen).to(DEV)
    p = (th.randn(N, P, 3, generator=gen) * 1.05 + 0.02).to(DEV)
    g = th.randn(N, P, generator=gen).to(DEV)
    chunk = max(1, int(a.block_gib * 2 ** 30 / 4 / (N * M)))
    print(f"== {a.case}: N = {N}, P = {P}, M = {M}, float32, {pairs:.3e} pairs; S = {capi.nearest_split(N, P, M)[0]} ranges; "
          f"cdist loop: {chunk} queries per chunk ({-(-P // chunk)} chunks, one [N, chunk, M] block = {N * chunk * M * 4 / 2 ** 30:.2f} GiB)")

    pr, qr = p.clone().requires_grad_(True), q.clone().requires_grad_(True)

    def hip_fwd():
        return drtk_amd.nearest_points(p, q)

    def hip_fb():
        d, _ = drtk_amd.nearest_points(pr, qr)
        th.autograd.grad(d, (pr, qr), g)

    def loop_fwd():
        with th.no_grad():
            return cdist_loop(p, q, chunk)

    def loop_fb():
        d, _ = cdist_loop(pr, qr, chunk)
        th.autograd.grad(d, (pr, qr), g)

    d_hip, i_hip = hip_fwd()
    d_loop, i_loop = loop_fwd()
    same = float((i_hip == i_loop).float().mean())
    rel = float(((d_hip - d_loop).abs() / d_hip.clamp(min=1e-30)).max())
    print(f"indices equal to the cdist loop's: {100 * same:.4f} %; largest relative difference of dist2: {rel:.2e}")

    res = windows({"hip fwd": hip_fwd, "loop fwd": loop_fwd, "hip fwd+bwd": hip_fb, "loop fwd+bwd": loop_fb}, a.window_ms, a.rounds)
    for k, w in res.items():
        med = statistics.median(w)
        print(f"{k:14s} {med:10.3f} ms  ({min(w):.3f} ... {max(w):.3f})  {pairs / med * 1e3:.3e} pairs/s")
    for what in ("fwd", "fwd+bwd"):
        h, l = res["hip " + what], res["loop " + what]
        verdict = "faster in every window" if max(h) < min(l) else ("SLOWER in every window" if min(h) > max(l) else "windows overlap")
        print(f"{what}: cdist loop / hip = {statistics.median(l) / statistics.median(h):.1f} x ({verdict})")

    # kernels, from the library's own timing collection (events around every launch)
    th.cuda.synchronize()
    reps = 5
    capi.kernel_timing_begin()
    for _ in range(reps):
        hip_fb()
    th.cuda.synchronize()
    rep = capi.kernel_timing_report()
    for name, (launches, ms) in rep.items():
        per = ms / launches
        line = f"  {name.split('(')[-1].strip('()'):44s} {launches:3d} launches  {per:9.4f} ms each"
        if "nearest_forward_kernel" in name:
            rate = pairs / per * 1e3
            peak = VALU_ISSUE * 64 / VALU_PER_PAIR
            line += f"  {rate:.3e} pairs/s = {100 * rate / peak:.1f} % of the VALU issue peak ({VALU_PER_PAIR:.2f} vector instructions per pair: {peak:.3e} pairs/s)"
        print(line)


if __name__ == "__main__":
    main()
