#!/usr/bin/env python3
"""drtk_amd.skin (forward, forward + backward to the rest pose, the weights and the transforms), float32, 8 views, one
mesh per run and (J, K) = (24, 4) and (128, 8): the HIP route (csrc/skin.hip) against two baselines on the same card in
the same run --

  dense      what a rig with a dense [V,J] matrix writes: einsum('vj,njab->nvab', W, T) (an [N,V,12] intermediate) followed
             by a batched apply, and
  gather     the package's own PyTorch formulation (drtk_amd/skin.py: T[:, idx] of shape [N,V,K,3,4], blended, applied),
             whose backward to the transforms is an index_put with accumulation.

The three are timed as whole calls with device events after warm-up, alternating, `--rounds` windows each; reported are
the median and the spread (min ... max) of the windows, and HIP counts as "not slower" than the baselines only when its
slowest window beats the faster baseline's fastest.  Then each kernel's time from the library's own timing collection,
with the bytes the algorithm must move at least once (from the shapes) and their rate as a fraction of the 8 TB/s HBM
figure.

One process per mesh, each under its own time limit, the second only if the first ended well:

    timeout -k 10 300 python profiles/skin_bench.py --mesh 100k && \\
    timeout -k 10 500 python profiles/skin_bench.py --mesh 1M
"""
import argparse
import os
import statistics
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drtk_amd  # noqa: E402
from drtk_amd import capi  # noqa: E402
from drtk_amd import synthetic as S  # noqa: E402
from drtk_amd.skin import _skin_torch  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12


def _window_ms(fn, iters):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b)


def time_ms(fn, window_ms, warmup=3):
    """ms per call over a timed window of about `window_ms` (sized from a short probe)"""
    for _ in range(warmup):
        fn()
    th.cuda.synchronize()
    iters = max(5, min(5000, int(window_ms / max(_window_ms(fn, 3) / 3, 1e-3))))
    return _window_ms(fn, iters) / iters


def rig(V, J, K, gen):
    """Skewed like a body rig: joint 0 (the root) in a slot of half the vertices, the others spread over the mesh in
    contiguous patches with random neighbours; weights a softmax per vertex."""
    patch = (th.arange(V, device=DEV) * (J - 1) // V + 1)[:, None]
    idx = (patch + th.randint(-2, 3, (V, K), device=DEV, generator=gen)).clamp(1, J - 1)
    idx[:, 0] = patch[:, 0]
    root = th.rand(V, device=DEV, generator=gen) < 0.5
    idx[root, K - 1] = 0
    w = th.softmax(th.randn(V, K, device=DEV, generator=gen), 1)
    return idx, w


def algorithmic_bytes(N, V, J, K, es=4, idx=4):
    """per launch, from the shapes: what it must read and write at least once"""
    row = V * K * (idx + es)
    tr = N * J * 12 * es
    return {
        "skin_forward_kernel": 2 * N * V * 3 * es + row + tr,
        "skin_vertex_backward_kernel": 3 * N * V * 3 * es + row + V * K * es + tr,
        "skin_joint_chunk_kernel": V * K * (idx + es) + 2 * N * V * 3 * es,
        "skin_joint_sum_kernel": tr,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="100k", choices=list(S.MESH_SIZES))
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--window-ms", type=float, default=200.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert th.cuda.is_available(), "skin_bench.py measures on the GPU; there is no CPU fall-back"
    N = a.views
    v0, _ = S.uv_sphere(*S.MESH_SIZES[a.mesh], dtype=th.float64)
    V = v0.shape[0]
    gen = th.Generator(DEV).manual_seed(1)
    v = (v0[None] * (1 + 0.1 * th.arange(N, dtype=th.float64))[:, None, None]).float().to(DEV)
    g = th.randn(N, V, 3, device=DEV, generator=gen)
    ok = True
    for J, K in ((24, 4), (128, 8)):
        idx, w = rig(V, J, K, gen)
        t = (th.eye(4, device=DEV)[:3] + 0.1 * th.randn(N, J, 3, 4, device=DEV, generator=gen)).contiguous()
        dense_w = th.zeros(V, J, device=DEV).index_put((th.arange(V, device=DEV)[:, None].expand(V, K), idx), w, accumulate=True)
        counts = th.bincount(idx.reshape(-1), minlength=J)
        print(f"mesh {a.mesh}: V = {V}, {N} views, J = {J}, K = {K}, float32; slots per joint: median {int(counts.median())}, max {int(counts.max())}")

        def dense(vv, _idx, ww, tt):
            m = th.einsum("vj,njab->nvab", ww, tt)
            return th.einsum("nvab,nvb->nva", m[..., :3], vv) + m[..., 3]

        routes = {"hip": (drtk_amd.skin, w), "dense": (dense, dense_w), "gather": (_skin_torch, w)}
        ref = _skin_torch(v.double(), idx, w.double(), t.double())
        for name, (fn, ww) in routes.items():
            err = float((fn(v, idx, ww, t).double() - ref).abs().max() / ref.abs().max())
            print(f"  {name:8s} max |out - f64| / max|f64| = {err:.2e}")
            assert err < 1e-4, name

        def fwd(fn, ww):
            return lambda: fn(v, idx, ww, t)

        def fwd_bwd(fn, ww):
            def run():
                vv, w2, tt = v.detach().requires_grad_(True), ww.detach().requires_grad_(True), t.detach().requires_grad_(True)
                fn(vv, idx, w2, tt).backward(g)
            return run

        for what, make in (("skin forward", fwd), ("skin forward + backward (v, weights, transforms)", fwd_bwd)):
            times = {name: [] for name in routes}
            for _ in range(a.rounds):  # alternating: a drift of the machine hits every route alike
                for name, (fn, ww) in routes.items():
                    times[name].append(time_ms(make(fn, ww), a.window_ms))
            print(what)
            for name, tm in times.items():
                print(f"  {name:8s} median {statistics.median(tm):8.3f} ms   spread {min(tm):8.3f} ... {max(tm):8.3f} ms")
            best = min((n for n in times if n != "hip"), key=lambda n: min(times[n]))
            faster = max(times["hip"]) < min(times[best])
            ok &= faster
            print(f"  hip vs the faster baseline ({best}): {statistics.median(times[best]) / statistics.median(times['hip']):.2f}x, "
                  f"{'slowest hip window beats its fastest' if faster else 'NOT separated from it by the spread'}")

        steps = 10
        th.cuda.synchronize()
        capi.kernel_timing_begin()
        for _ in range(steps):
            fwd_bwd(drtk_amd.skin, w)()
        th.cuda.synchronize()
        rep = capi.kernel_timing_report()
        need = algorithmic_bytes(N, V, J, K)
        print("kernels (per launch; bytes: what the algorithm must move at least once)")
        for name, (count, ms) in rep.items():
            per = ms / count
            nbytes = need.get(name.split("<")[0])
            frac = f"{nbytes / (per * 1e-3) / HBM:5.2f} of 8 TB/s on {nbytes / 1e6:8.1f} MB" if nbytes else ""
            print(f"  {name:52s} {count:4d} launches  {per * 1e3:9.1f} us  {frac}")
    print("verdict:", "HIP beats the faster baseline beyond the spread in every row" if ok else "see the rows marked NOT")


if __name__ == "__main__":
    main()
