#!/usr/bin/env python3
"""filter2d on 8 x 16 x 1024 x 1024 images, float32 and float16: `upsample` x 2, `downsample` x 2 and `low_pass_filter`, 6
taps each (Kaiser, reflection padding: the defaults), forward and forward+backward -- each leg next to the formulation a
user of PyTorch-ROCm would otherwise call on the same card in the same run: pad, zero insertion, crop and two grouped
`conv2d` calls (torch_resample below), under autograd for the backward.

    python profiles/filter2d_bench.py [--iters 5] [--rounds 3] [--small] [--only upsample,downsample,low_pass_filter]

The script is a driver: every leg runs in a child process of its own under `timeout`, one after the other, and the driver
stops at the first child that fails.  A child checks that the two formulations agree on its shape, warms both up, then times
`rounds` windows of `iters` back-to-back calls with device events; the median window is printed with min - max, the spread
a difference has to be read against.  Also printed, from shapes: the bytes of the input plus the output (twice for
forward+backward: the gradient pass reads an output-sized image and writes an input-sized one), over the time, and that as a
share of the 8 TB/s HBM figure of BASELINE.md.  No ratio is fixed in advance.  A separate tool: bench.py does not call it."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E, nominal
OPS = {"upsample": (2, 1), "downsample": (1, 2), "low_pass_filter": (1, 1)}
DTYPES = ("float32", "float16")
STEPS = ("forward", "forward+backward")
LIMIT = 300  # seconds per child


def torch_resample(x, f, up, down, reflect):
    """The same operator from PyTorch's own pieces.  pad0 / pad1: drtk/filter2d_ref.py's padding rule."""
    import torch.nn.functional as F

    k, C = f.numel(), x.shape[1]
    if up == 1 and down == 1:
        p0, p1 = k // 2, (k - 1) // 2
    elif down != 1:
        p0, p1 = (k - down + 1) // 2, (k - down) // 2
    else:
        p0, p1 = (k + up - 1) // 2, (k - up) // 2

    def stuff(t):
        if up == 1:
            return t
        z = t.new_zeros(t.shape[0], t.shape[1], t.shape[2] * up, t.shape[3] * up)
        z[:, :, ::up, ::up] = t
        return z

    if reflect:
        q0, q1 = -(-p0 // up), -(-p1 // up)
        x = stuff(F.pad(x, [q0, q1, q0, q1], mode="reflect"))
        c0, c1 = q0 * up - p0, q1 * up - p1
        x = x[:, :, c0:x.shape[2] - c1, c0:x.shape[3] - c1]
    else:
        x = F.pad(stuff(x), [p0, p1, p0, p1])
    w = f.flip(0).to(x.dtype).reshape(1, 1, 1, k).repeat(C, 1, 1, 1)
    x = F.conv2d(x, w, groups=C, stride=(1, down))
    return F.conv2d(x, w.reshape(C, 1, k, 1), groups=C, stride=(down, 1))


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


def child(op, dtype_name, step, iters, rounds, small):
    import torch as th

    sys.path.insert(0, ROOT)
    import drtk_amd

    assert th.cuda.is_available(), "filter2d_bench needs a GPU: there is no CPU path to time"
    dev = "cuda:0"
    dtype = getattr(th, dtype_name)
    N, C, S = (2, 4, 128) if small else (8, 16, 1024)
    up, down = OPS[op]
    m = max(up, down)
    opt = drtk_amd.FilterOptions(6)
    f = drtk_amd.make_resampling_kernel(opt, m, 1.0, float(up), device=th.device(dev))
    g = th.Generator().manual_seed(1)
    x = (th.rand(N, C, S, S, generator=g) * 2 - 1).to(dev, dtype)
    backward = step == "forward+backward"
    x.requires_grad_(backward)

    def ours():
        if op == "upsample":
            return drtk_amd.upsample(x, opt, 2)
        if op == "downsample":
            return drtk_amd.downsample(x, opt, 2)
        return drtk_amd.low_pass_filter(x, opt)

    def torchs():
        return torch_resample(x, f, up, down, True)

    ya, yb = ours(), torchs()
    assert ya.shape == yb.shape and ya.dtype == yb.dtype == dtype
    tol = 1e-5 if dtype == th.float32 else 4e-3
    err = float((ya.detach().float() - yb.detach().float()).abs().max())
    assert err <= tol * float(yb.detach().float().abs().max()), f"the two formulations disagree: {err}"
    gout = (th.rand(ya.shape, generator=g) * 2 - 1).to(dev, dtype)
    del ya, yb

    def run(fn):
        def go():
            y = fn()
            if backward:
                x.grad = None
                y.backward(gout)
        return go

    moved = (x.numel() + gout.numel()) * x.element_size() * (2 if backward else 1)
    res = {}
    for who, fn in (("drtk_amd", run(ours)), ("pytorch", run(torchs))):
        for _ in range(2):
            fn()
        t = sorted(window(fn, iters) for _ in range(rounds))
        res[who] = t[len(t) // 2]
        ms = res[who]
        print(f"{op} {dtype_name} {step} {who}: {ms:.3f} ms ({t[0]:.3f} - {t[-1]:.3f}), median (min - max) of {rounds} windows of {iters} "
              f"calls; {moved / 1e9:.2f} GB in + out -> {moved / (ms * 1e-3) / 1e9:.0f} GB/s ({100 * moved / (ms * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s)")
    print(f"{op} {dtype_name} {step}: pytorch / drtk_amd = {res['pytorch'] / res['drtk_amd']:.2f}  ({N} x {C} x {S} x {S}, {f.numel()} filter values)",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--only", default=",".join(OPS), help="comma-separated subset of " + ", ".join(OPS))
    ap.add_argument("--leg", nargs=3, default=None, metavar=("OP", "DTYPE", "STEP"), help="(internal) run one leg in this process")
    a = ap.parse_args()
    if a.leg:
        return child(*a.leg, a.iters, a.rounds, a.small)
    for op in a.only.split(","):
        assert op in OPS, op
        for dtype in DTYPES:
            for step in STEPS:
                cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--leg", op, dtype, step, "--iters",
                       str(a.iters), "--rounds", str(a.rounds)] + (["--small"] if a.small else [])
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    sys.exit(f"filter2d_bench: leg '{op} {dtype} {step}' ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
