#!/usr/bin/env python3
"""msi on one background view: 1024 x 1024 pinhole rays from an origin off-centre inside the unit sphere through a
32 x 4 x 512 x 1024 float32 multi-sphere image, sub_step_count = 2, min_inv_r = 1, max_inv_r = 0, stop_thresh = 1e-7
(64 spheres per ray, all of them hit, no ray stops early: sigma is drawn in [0, 2]).

    python profiles/msi_bench.py [--iters 10] [--rounds 5] [--small]

The script is a driver: each GPU step -- `forward`, `forward+backward` -- runs in a child process of its own under
`timeout`, one after the other, and the driver stops at the first child that fails.  A child warms the shape up, then times
`rounds` windows of `iters` back-to-back calls of the C ABI binding (drtk_amd.capi.msi_forward / msi_backward: the entry
points the operator calls; the gradient's zero fill included) with device events;
the median window is printed with min - max, the spread a difference has to be read against.
Also printed, from shapes:
  gathered     bytes the sixteen taps of every sample ask for (rays x spheres x 16 x 4 channels), over the time: what the
               caches serve, not HBM traffic -- compared with the 8 TB/s HBM figure of BASELINE.md it says how far above
               a stream from memory the gather runs;
  compulsory   the texture read once, the rays and the output (forward), plus the gradient
               zero-filled and written (backward): the least HBM traffic, over the time, as a share of 8 TB/s;
  atomics      bytes the backward adds to the gradient (one float atomic per tap and channel), over its time.
There is no pass / fail time: nothing else computes this on PyTorch-ROCm.  A separate tool: bench.py does not call it."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E, nominal
STEPS = {"forward": 120, "forward+backward": 300}  # step -> time limit of its child, seconds


def make(small):
    import torch as th

    dev = "cuda:0"
    S, (L, H, W) = (128, (8, 64, 128)) if small else (1024, (32, 512, 1024))
    g = th.Generator().manual_seed(1)
    tex = th.rand(L, 4, H, W, generator=g)
    tex[:, 3] *= 2.0
    # a pinhole camera: focal = S (a field of view of 53 degrees), principal point at the centre, rotated off the axes
    ys, xs = th.meshgrid(th.arange(S, dtype=th.float32) + 0.5, th.arange(S, dtype=th.float32) + 0.5, indexing="ij")
    d_cam = th.stack([(xs - S / 2) / S, (ys - S / 2) / S, th.ones_like(xs)], -1).reshape(-1, 3)
    a, b = 0.4, 0.25
    ry = th.tensor([[th.cos(th.tensor(a)), 0, th.sin(th.tensor(a))], [0, 1, 0], [-th.sin(th.tensor(a)), 0, th.cos(th.tensor(a))]])
    rx = th.tensor([[1, 0, 0], [0, th.cos(th.tensor(b)), -th.sin(th.tensor(b))], [0, th.sin(th.tensor(b)), th.cos(th.tensor(b))]])
    camrot = rx @ ry
    ray_d = d_cam @ camrot  # world = camrot^T cam
    ray_o = th.tensor([0.3, 0.1, -0.2]).expand_as(ray_d).contiguous()
    gout = th.rand(S * S, 4, generator=g) * 2 - 1
    return ray_o.to(dev), ray_d.contiguous().to(dev), tex.to(dev), gout.to(dev)


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


def child(step, iters, rounds, small):
    import torch as th

    sys.path.insert(0, ROOT)
    from drtk_amd import capi

    assert th.cuda.is_available(), "msi_bench needs a GPU: there is no CPU path to time"
    o, d, tex, gout = make(small)
    N, (L, _, H, W) = o.shape[0], tex.shape
    n = 2 * L
    out = capi.msi_forward(o, d, tex)
    stopped = int((out[:, 3] == -1000).sum())
    assert bool(th.isfinite(out).all()) and stopped == 0, f"{stopped} rays stopped early: the byte counts below assume none"

    def run():
        res = capi.msi_forward(o, d, tex)
        if step == "forward+backward":
            capi.msi_backward(gout, res, o, d, tex)

    for _ in range(3):
        run()
    t = sorted(window(run, iters) for _ in range(rounds))
    ms = t[len(t) // 2]
    gathered = N * n * 16 * 4 * 4
    compulsory = tex.numel() * 4 + N * (6 + 4) * 4
    passes = 1
    if step == "forward+backward":
        passes, compulsory = 2, 2 * compulsory + 2 * tex.numel() * 4 + N * 8 * 4
    print(f"{step}: {ms:.3f} ms ({t[0]:.3f} - {t[-1]:.3f}), median (min - max) of {rounds} windows of {iters} calls; "
          f"{N} rays x {n} spheres, texture {L} x 4 x {H} x {W} float32")
    print(f"  gathered {passes * gathered / 1e9:.2f} GB -> {passes * gathered / (ms * 1e-3) / 1e12:.2f} TB/s ({passes * gathered / (ms * 1e-3) / HBM_BYTES_PER_S:.2f} x the HBM figure); "
          f"compulsory {compulsory / 1e6:.0f} MB -> {compulsory / (ms * 1e-3) / 1e12:.3f} TB/s ({100 * compulsory / (ms * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s)")
    if step == "forward+backward":
        print(f"  atomics {gathered / 1e9:.2f} GB added to the gradient per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--step", choices=list(STEPS), default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.iters, a.rounds, a.small)
    for step, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters),
               "--rounds", str(a.rounds)] + (["--small"] if a.small else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"msi_bench: step '{step}' ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
