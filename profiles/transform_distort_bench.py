#!/usr/bin/env python3
"""transform with a distortion camera model: 8 views of 100 000 SHARED world-space vertices ([1,V,3]), float32, with the
fisheye model (4 coefficients) and the radial-tangential model (8 coefficients), fov given -- the fused route
(drtk_amd_ext::transform_distort: one kernel each way) against the package's own PyTorch formulation of the same models
(drtk_amd.transform._transform_torch_route: what `transform` falls back to when a camera parameter requires a gradient),
on the same card, in the same process, in alternating windows.

    python profiles/transform_distort_bench.py [--iters 50] [--rounds 7] [--small]

The script is a driver: each GPU step -- (model) x (`forward`, `forward+backward`) -- runs in a child process of its own
under `timeout`, one after the other, and the driver stops at the first child that fails.  A child warms both routes up,
checks that they agree, then times `rounds` pairs of windows (fused: 10 x `iters` calls, PyTorch: `iters` calls; device
events around each window) and prints the median window of each route with min - max, the spread a difference has to
be read against.  `forward+backward` is `transform(v)` under autograd followed by `backward` of a fixed upstream gradient
into the shared vertices.  Also printed, from shapes: the least memory traffic of the fused call (the vertices read once,
v_pix written; backward: the vertices and the upstream gradient read, the [1,V,3] gradient written) over its time as a
share of the 8 TB/s HBM figure.  There is no pass / fail time.  A separate tool: bench.py does not call it."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E, nominal
MODELS = {
    "fisheye": ("fisheye", (-0.03, 0.02, -0.01, 0.004)),
    "rt8": ("radial-tangential", (-0.25, 0.08, 2e-3, -3e-3, -0.02, 0.05, -0.01, 0.002)),
}
STEPS = [(m, s) for m in MODELS for s in ("forward", "forward+backward")]
LIMIT = 240  # time limit of a child, seconds


def make(model, small):
    import torch as th

    sys.path.insert(0, ROOT)
    from drtk_amd import synthetic as S

    dev = "cuda:0"
    N, V = (3, 1000) if small else (8, 100_000)
    g = th.Generator().manual_seed(1)
    v = (th.rand(1, V, 3, generator=g) * 2 - 1) * th.tensor([1.6, 1.2, 1.0])  # a box around the origin, seen from distance 3
    cams = S.ring_cameras(N, 2048, 1334)
    mode, row = MODELS[model]
    D = th.tensor(row)[None].repeat(N, 1) * th.linspace(0.9, 1.1, N)[:, None]
    fov = th.linspace(0.35, 0.6, N)[:, None]  # the box reaches |x/z| ~ 0.8: part of every view lies beyond fov
    gout = th.rand(N, V, 3, generator=g) * 2 - 1
    kw = dict(distortion_mode=mode, distortion_coeff=D.to(dev), fov=fov.to(dev))
    return v.to(dev), tuple(c.to(dev) for c in cams), kw, gout.to(dev)


def window(fn, iters):
    import torch as th

    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    th.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def child(model, step, iters, rounds, small):
    import torch as th

    assert th.cuda.is_available(), "transform_distort_bench needs a GPU: there is no CPU path to time"
    v, cams, kw, gout = make(model, small)
    from drtk_amd.transform import _transform_torch_route, transform

    backward = step == "forward+backward"
    v.requires_grad_(backward)

    def fused():
        out = transform(v, *cams, **kw)
        if backward:
            v.grad = None
            out.backward(gout)
        return out

    def torch_route():
        out = _transform_torch_route(v, *cams, **kw)[0]
        if backward:
            v.grad = None
            out.backward(gout)
        return out

    results = []
    for fn in (fused, torch_route):
        for _ in range(3):
            out = fn()
        results.append((out.detach().clone(), v.grad.clone() if backward else None))
    (a, ga), (b, gb) = results
    scale = float(b.abs().max())
    print(f"{model} {step}: {v.shape[1]} shared vertices x {cams[0].shape[0]} views, float32; routes agree within "
          f"{float((a - b).abs().max()) / scale:.1e} of max|v_pix|" + (f", {float((ga - gb).abs().max()) / float(gb.abs().max()):.1e} of max|grad v|" if backward else ""))
    assert float((a - b).abs().max()) <= 1e-4 * scale, "the two routes disagree: nothing is timed"
    tf, tt = [], []
    for _ in range(rounds):  # alternating: whatever else the card is doing falls on both routes
        tf.append(window(fused, 10 * iters))
        tt.append(window(torch_route, iters))
    tf.sort(), tt.sort()
    mf, mt = tf[len(tf) // 2], tt[len(tt) // 2]
    N, V = cams[0].shape[0], v.shape[1]
    traffic = (V * 3 + N * V * 3) * 4 + ((V * 3 + N * V * 3 + V * 3) * 4 if backward else 0)
    print(f"  fused   {mf * 1e3:9.1f} us ({tf[0] * 1e3:.1f} - {tf[-1] * 1e3:.1f}), median (min - max) of {rounds} windows of {10 * iters} calls; "
          f"least traffic {traffic / 1e6:.1f} MB -> {100 * traffic / (mf * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s")
    print(f"  PyTorch {mt * 1e3:9.1f} us ({tt[0] * 1e3:.1f} - {tt[-1] * 1e3:.1f}), median (min - max) of {rounds} windows of {iters} calls")
    print(f"  ratio   {mt / mf:9.1f} x (PyTorch / fused, medians)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--step", default=None, help="(internal) run one step, `model:step`, in this process")
    a = ap.parse_args()
    if a.step:
        model, step = a.step.split(":")
        return child(model, step, a.iters, a.rounds, a.small)
    for model, step in STEPS:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", f"{model}:{step}",
               "--iters", str(a.iters), "--rounds", str(a.rounds)] + (["--small"] if a.small else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"transform_distort_bench: step '{model} {step}' ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
