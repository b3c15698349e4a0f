#!/usr/bin/env python3
"""mesh_laplacian (forward, forward + backward to x and weights) and cotangent_weights (forward + backward), float32,
C = 3, 8 views, one mesh per run: the HIP route (csrc/geometry.hip) against two baselines on the same card in the same
run --

  formulation   the package's own PyTorch formulation (drtk_amd/geometry.py: gather / scatter_add), and
  padded        what users of the reference write today (its hand-fitting tutorial): a neighbour table padded to the
                largest valence, built once, applied as (w[None, :, :, None] * d[:, idx, :]).sum(2); written afresh here
                with torch (coalesced sparse matrix -> padded rows); no autograd to the weights, so its backward is to x.

The three are timed with device events after warm-up, alternating, `--rounds` times each; reported are the median and
the spread (min ... max) of the rounds, and HIP counts as "not slower" than a baseline only when its slowest round beats
the baseline's fastest.  Then each kernel's time from the library's own timing collection, with the bytes the algorithm
must move at least once (from the shapes) and their rate as a fraction of the 8 TB/s HBM figure.

One process per mesh, each under its own time limit, the second only if the first ended well:

    timeout -k 10 300 python profiles/laplacian_bench.py --mesh 100k && \\
    timeout -k 10 500 python profiles/laplacian_bench.py --mesh 1M
"""
import argparse
import os
import statistics
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drtk_amd  # noqa: E402
import drtk_amd.geometry as G  # noqa: E402
from drtk_amd import capi  # noqa: E402
from drtk_amd import synthetic as S  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12


def padded_table(vi, w, V):
    """(idx [V,K] int64, weights [V,K]) of L = sum_j w_ij (x_j - x_i), diagonal included, rows padded with (0, 0.0)"""
    rows, cols, vals = [], [], []
    for k in range(3):
        i, j = vi[:, (k + 1) % 3], vi[:, (k + 2) % 3]
        for r, c, s in ((i, j, 1.0), (j, i, 1.0), (i, i, -1.0), (j, j, -1.0)):
            rows.append(r), cols.append(c), vals.append(s * w[:, k])
    m = th.sparse_coo_tensor(th.stack([th.cat(rows), th.cat(cols)]), th.cat(vals), (V, V)).coalesce()
    r, c = m.indices()
    count = th.bincount(r, minlength=V)
    start = th.cumsum(count, 0) - count
    slot = th.arange(r.numel(), device=r.device) - start[r]
    K = int(count.max())
    idx = th.zeros(V, K, dtype=th.long, device=r.device)
    wt = th.zeros(V, K, dtype=w.dtype, device=r.device)
    idx[r, slot], wt[r, slot] = c, m.values()
    return idx, wt


def _window_ms(fn, iters):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b)


def time_ms(fn, window_ms, warmup=3):
    """ms per call over a timed window of about `window_ms` (sized from a short probe): a window of a few calls would
    measure the clock and the scheduler as much as the kernels"""
    for _ in range(warmup):
        fn()
    th.cuda.synchronize()
    iters = max(10, min(5000, int(window_ms / max(_window_ms(fn, 5) / 5, 1e-3))))
    return _window_ms(fn, iters) / iters


def algorithmic_bytes(N, V, F, C, es=4, idx=4):
    """per launch, from the shapes: what it must read and write at least once (shared [F,3] topology and weights)"""
    inc = (V + 1) * idx + 3 * F * idx  # crow + entries
    return {
        "laplacian_vertex_kernel": inc + 3 * F * idx + 3 * F * es + 2 * N * V * C * es,
        "laplacian_grad_weights_kernel": 3 * F * idx + 2 * N * V * C * es + 3 * F * es,
        "cot_weights_face_kernel": 3 * F * idx + N * V * 3 * es + N * F * 3 * es,
        "cot_weights_face_backward_kernel": 3 * F * idx + N * V * 3 * es + N * F * 3 * es + N * F * 9 * es,
        "geom_vertex_gather_kernel": inc + N * F * 9 * es + N * V * 3 * es,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="100k", choices=["100k", "1M"])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--window-ms", type=float, default=250.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert th.cuda.is_available(), "laplacian_bench.py measures on the GPU; there is no CPU fall-back"
    N, C = a.views, 3
    v0, vi = S.uv_sphere(*S.MESH_SIZES[a.mesh], dtype=th.float64)
    V, F = v0.shape[0], vi.shape[0]
    vi = vi.to(DEV)
    k = th.arange(N, dtype=th.float64)
    v = (v0[None] * (1 + 0.1 * k)[:, None, None]).float().to(DEV)
    gen = th.Generator(DEV).manual_seed(1)
    x = th.randn(N, V, C, device=DEV, generator=gen)
    g = th.randn(N, V, C, device=DEV, generator=gen)
    gw = th.randn(N, F, 3, device=DEV, generator=gen)
    w = drtk_amd.cotangent_weights(v[:1], vi)[0].clamp(-10, 10)  # shared [F,3], as the tutorial's table is
    idx, wt = padded_table(vi.long(), w, V)
    print(f"mesh {a.mesh}: V = {V}, F = {F}, {N} views, C = {C}, float32; padded table {tuple(idx.shape)}")

    def padded(d, _vi, _w):
        return (wt[None, :, :, None] * d[:, idx, :]).sum(2)

    # one set of inputs, three routes: the same numbers up to rounding
    ref = G._mesh_laplacian_torch(x.double(), vi, w.double())
    for name, fn in (("hip", drtk_amd.mesh_laplacian), ("formulation", G._mesh_laplacian_torch), ("padded", padded)):
        err = float((fn(x, vi, w).double() - ref).abs().max() / ref.abs().max())
        print(f"  {name:12s} max |out - f64| / max|f64| = {err:.2e}")
        assert err < 1e-4, name

    def lap_fwd(fn):
        return lambda: fn(x, vi, w)

    def lap_fwd_bwd(fn, weights_too):
        def run():
            xx = x.detach().requires_grad_(True)
            ww = w.detach().requires_grad_(weights_too)
            fn(xx, vi, ww).backward(g)
        return run

    def cot_fwd_bwd(fn):
        def run():
            vv = v.detach().requires_grad_(True)
            fn(vv, vi).backward(gw)
        return run

    rows = [
        ("mesh_laplacian forward", {"hip": lap_fwd(drtk_amd.mesh_laplacian), "formulation": lap_fwd(G._mesh_laplacian_torch), "padded": lap_fwd(padded)}),
        ("mesh_laplacian forward + backward (x)", {"hip": lap_fwd_bwd(drtk_amd.mesh_laplacian, False), "formulation": lap_fwd_bwd(G._mesh_laplacian_torch, False), "padded": lap_fwd_bwd(padded, False)}),
        ("mesh_laplacian forward + backward (x, weights)", {"hip": lap_fwd_bwd(drtk_amd.mesh_laplacian, True), "formulation": lap_fwd_bwd(G._mesh_laplacian_torch, True)}),
        ("cotangent_weights forward + backward", {"hip": cot_fwd_bwd(drtk_amd.cotangent_weights), "formulation": cot_fwd_bwd(G._cotangent_weights_torch)}),
    ]
    ok = True
    for what, routes in rows:
        times = {name: [] for name in routes}
        for _ in range(a.rounds):  # alternating: a drift of the machine hits every route alike
            for name, fn in routes.items():
                times[name].append(time_ms(fn, a.window_ms))
        print(what)
        for name, t in times.items():
            print(f"  {name:12s} median {statistics.median(t):8.3f} ms   spread {min(t):8.3f} ... {max(t):8.3f} ms")
        for name, t in times.items():
            if name != "hip":
                faster = max(times["hip"]) < min(t)
                ok &= faster
                print(f"  hip vs {name}: {statistics.median(t) / statistics.median(times['hip']):.2f}x, "
                      f"{'not slower beyond the spread' if faster else 'NOT separated from it by the spread'}")

    # per kernel: the library's own event timing around a few steps
    steps = 10
    th.cuda.synchronize()
    capi.kernel_timing_begin()
    for _ in range(steps):
        lap_fwd_bwd(drtk_amd.mesh_laplacian, True)()
        cot_fwd_bwd(drtk_amd.cotangent_weights)()
    th.cuda.synchronize()
    rep = capi.kernel_timing_report()
    need = algorithmic_bytes(N, V, F, C)
    print("kernels (per launch; bytes: what the algorithm must move at least once)")
    for name, (count, ms) in rep.items():
        base = name.split("<")[0]
        per = ms / count
        nbytes = need.get(base)
        frac = f"{nbytes / (per * 1e-3) / HBM:5.2f} of 8 TB/s on {nbytes / 1e6:8.1f} MB" if nbytes else ""
        print(f"  {name:48s} {count:4d} launches  {per * 1e3:9.1f} us  {frac}")
    print("verdict:", "HIP not slower than either baseline beyond the spread" if ok else "see the rows marked NOT")


if __name__ == "__main__":
    main()
