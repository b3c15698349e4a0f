#!/usr/bin/env python3
"""`ssim` and `photometric_loss` under a foreground mask, float32, at 8 x 3 x 2048 x 2048, 2 x 3 x 4096 x 4096 and
8 x 3 x 512 x 512: forward without gradient and forward+backward -- each leg next to the formulation a user of PyTorch-ROCm
would otherwise write on the same card in the same run: five grouped Gaussian convolutions as two `conv2d` calls each and
the element-wise glue around them (tests/image_loss_oracle.py), under autograd for the backward.

    python profiles/image_loss_bench.py [--iters 20] [--rounds 3] [--small] [--only ssim,photometric_loss]

The script is a driver: every (operator, shape) runs in a child process of its own under `timeout`, one after the other, and
the driver stops at the first child that fails.  A child checks that the two formulations agree on its shape, warms both up,
then times `rounds` windows of `iters` back-to-back calls with device events; the median window is printed with min - max,
the spread a difference has to be read against.  Also printed, from shapes: the algorithmic bytes -- the two images and the
(bool) weight read once; with the backward pass also the three gradient maps written once and read once and the gradient
written once -- over the time, and that as a share of the 8 TB/s HBM figure of BASELINE.md.  No ratio is fixed in advance.
A separate tool: bench.py does not call it."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E, nominal
OPS = ("ssim", "photometric_loss")
SHAPES = {"8x3x2048x2048": (8, 3, 2048, 2048), "2x3x4096x4096": (2, 3, 4096, 4096), "8x3x512x512": (8, 3, 512, 512)}
SMALL = {"2x3x96x128": (2, 3, 96, 128)}
STEPS = ("forward", "forward+backward")
LIMIT = 300  # seconds per child


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


def inputs(shape, dev):
    """(img, target, mask) made on the device from a seed: a smooth target whose top third is constant, img = target plus
    noise of 0.1 clamped to [0, 1], the mask a disc per view with holes."""
    import torch as th

    N, C, H, W = shape
    th.manual_seed(1)
    yy = th.linspace(0, 1, H, device=dev).view(1, 1, H, 1)
    xx = th.linspace(0, 1, W, device=dev).view(1, 1, 1, W)
    c = th.arange(C, device=dev, dtype=th.float32).view(1, C, 1, 1)
    n = th.arange(N, device=dev, dtype=th.float32).view(N, 1, 1, 1)
    target = (0.5 + 0.25 * th.sin(6.0 * xx + 0.7 * c + 0.3 * n) * th.cos(5.0 * yy - 0.4 * c)).clamp(0, 1).contiguous()
    target[:, :, :H // 3] = 0.4
    img = (target + 0.1 * th.randn(shape, device=dev)).clamp(0, 1)
    mask = ((yy - 0.5) ** 2 + (xx - 0.5) ** 2 < 0.2).expand(N, 1, H, W)[:, 0] & (th.rand(N, H, W, device=dev) > 0.1)
    return img, target, mask.contiguous()


def child(op, shape_name, iters, rounds, small):
    import torch as th

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import drtk_amd
    import image_loss_oracle as O

    assert th.cuda.is_available(), "image_loss_bench needs a GPU: there is no CPU path to time"
    dev = "cuda:0"
    shape = (SMALL if small else SHAPES)[shape_name]
    N, C, H, W = shape
    img, target, mask = inputs(shape, dev)
    ours_fn = getattr(drtk_amd, op)
    torch_fn = getattr(O, op)

    for step in STEPS:
        backward = step == "forward+backward"
        x = img.clone().requires_grad_(backward)

        def run(fn):
            def go():
                if backward:
                    x.grad = None
                    fn(x, target, mask).backward()
                else:
                    with th.no_grad():
                        fn(x, target, mask)
            return go

        # the two formulations agree on this shape (a sanity check of the comparison, not a test: tests/test_gpu_image_loss.py)
        got = {}
        for who, fn in (("drtk_amd", ours_fn), ("pytorch", torch_fn)):
            run(fn)()
            with th.no_grad():
                got[who] = (float(fn(x, target, mask)), x.grad.clone() if backward else None)
        va, vb = got["drtk_amd"][0], got["pytorch"][0]
        assert abs(va - vb) <= 1e-4 * max(1.0, abs(vb)), f"the two formulations disagree: {va} vs {vb}"
        if backward:
            ga, gb = got["drtk_amd"][1], got["pytorch"][1]
            assert float((ga - gb).abs().max()) <= 2e-2 * float(gb.abs().max()), "the two gradients disagree"
        del got
        x.grad = None

        elem = img.element_size()
        moved = 2 * img.numel() * elem + mask.numel() * mask.element_size()
        if backward:
            moved += (6 + 1) * img.numel() * elem
        res = {}
        for who, fn in (("drtk_amd", run(ours_fn)), ("pytorch", run(torch_fn))):
            for _ in range(2):
                fn()
            t = sorted(window(fn, iters) for _ in range(rounds))
            res[who] = ms = t[len(t) // 2]
            print(f"{op} {shape_name} float32 {step} {who}: {ms:.3f} ms ({t[0]:.3f} - {t[-1]:.3f}), median (min - max) of {rounds} windows of "
                  f"{iters} calls; {moved / 1e9:.3f} GB algorithmic -> {moved / (ms * 1e-3) / 1e12:.3f} TB/s "
                  f"({100 * moved / (ms * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s)")
        print(f"{op} {shape_name} float32 {step}: pytorch / drtk_amd = {res['pytorch'] / res['drtk_amd']:.2f}  (value {va:.6f}, "
              f"mask covers {100 * float(mask.float().mean()):.0f} %)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tiny shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--only", default=",".join(OPS), help="comma-separated subset of " + ", ".join(OPS))
    ap.add_argument("--leg", nargs=2, default=None, metavar=("OP", "SHAPE"), help="(internal) run one operator and shape in this process")
    a = ap.parse_args()
    if a.leg:
        return child(*a.leg, a.iters, a.rounds, a.small)
    for op in a.only.split(","):
        assert op in OPS, op
        for shape_name in (SMALL if a.small else SHAPES):
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--leg", op, shape_name, "--iters",
                   str(a.iters), "--rounds", str(a.rounds)] + (["--small"] if a.small else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit(f"image_loss_bench: leg '{op} {shape_name}' ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
