#!/usr/bin/env python3
"""mipmap_pyramid against the loop it replaces, in eager PyTorch: `levels.append(avg_pool2d(levels[-1], 2))`, all levels
(11 at these sizes), forward and forward + backward.

    python profiles/mipmap_pyramid_bench.py [--reps 25] [--small]

Shapes: [1,3,4096,4096] float32 (the scale of BASELINE configs[4]) and float64, [1,3,1024,1024] and [8,16,1024,1024] float32.
Both contenders run in this process on the same card, alternating call by call: `reps` repetitions each of forward and of
forward + backward, after a warm-up of both, each repetition between two device events; the median is printed with
min - max.  The backward pass is torch.autograd.backward of all levels with given upstream gradients, one per level, carved
out of ONE flat buffer as the sampler's backward hands them over: no loss glue on either side.

Algorithmic bytes, from the shapes (s = element size, HW = texels of a plane, S = sum over levels l >= 1 of h_l w_l, P planes):
  forward    s P (HW + S) -- level 0 read once, every level written once -- plus s P h_6 w_6, level 6 read again by the
             second launch (levels > 7)
  backward   s P (HW + S) read -- every gradient texel once -- and s P HW written
and forward + backward is their sum; over the op's time, as a share of the 8 TB/s of BASELINE.md.
The yardstick is the loop in the same run.  Where the op is slower the line says so; nothing else is concluded here.
A separate tool: bench.py does not call it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E, nominal


def loop(x, levels):
    import torch as th

    out = [x]
    for _ in range(levels - 1):
        out.append(th.nn.functional.avg_pool2d(out[-1], 2))
    return out


def timed(fn):
    import torch as th

    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    th.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert a.reps >= 20 or a.small, "the median of at least 20 repetitions"
    import torch as th

    sys.path.insert(0, ROOT)
    import drtk_amd

    assert th.cuda.is_available(), "mipmap_pyramid_bench needs a GPU: there is no CPU path to time"
    dev = "cuda:0"
    cases = [((1, 3, 4096, 4096), th.float32), ((1, 3, 1024, 1024), th.float32), ((8, 16, 1024, 1024), th.float32),
             ((1, 3, 4096, 4096), th.float64)]
    if a.small:
        cases = [((1, 3, 256, 256), th.float32), ((2, 2, 130, 70), th.float64)]
    slower = []
    for shape, dtype in cases:
        N, C, H, W = shape
        L = min(11, min(H, W).bit_length())
        s, P = th.finfo(dtype).bits // 8, N * C
        S = sum((H >> l) * (W >> l) for l in range(1, L))
        fwd_bytes = s * P * (H * W + S) + (s * P * (H >> 6) * (W >> 6) if L > 7 else 0)
        bwd_bytes = s * P * (H * W + S) + s * P * H * W
        g = th.Generator(device=dev).manual_seed(1)
        x0 = th.rand(shape, generator=g, device=dev, dtype=dtype)
        flat = th.rand(P * (H * W + S), generator=g, device=dev, dtype=dtype)
        grads, at = [], 0
        for l in range(L):
            n = P * (H >> l) * (W >> l)
            grads.append(flat[at:at + n].view(N, C, H >> l, W >> l))
            at += n

        def op(x):
            return drtk_amd.mipmap_pyramid(x, L)

        def lp(x):
            return loop(x, L)

        x = x0.clone().requires_grad_(True)
        with th.no_grad():
            same = all(th.equal(p, q) for p, q in zip(op(x0), lp(x0)))
        th.autograd.backward(op(x), grads)
        g_op, x.grad = x.grad, None
        th.autograd.backward(lp(x), grads)
        err = float(((g_op - x.grad).abs() / x.grad.abs()).max()) / th.finfo(dtype).eps
        same_grad = th.equal(g_op, x.grad)
        del g_op

        def forward(f):
            with th.no_grad():
                f(x0)

        def both(f):
            x.grad = None
            th.autograd.backward(f(x), grads)

        print(f"{N} x {C} x {H} x {W}, {str(dtype).split('.')[-1]}, {L} levels; levels bitwise equal to the loop's: {same}; "
              f"grad_input bitwise equal: {same_grad} (max rel err {err:.2f} eps)")
        for step, run, nbytes in (("forward", forward, fwd_bytes), ("forward+backward", both, fwd_bytes + bwd_bytes)):
            for _ in range(3):
                run(op), run(lp)
            t = {"op": [], "loop": []}
            for _ in range(a.reps):
                t["op"].append(timed(lambda: run(op)))
                t["loop"].append(timed(lambda: run(lp)))
            med = {}
            for who, v in t.items():
                v.sort()
                med[who] = v[len(v) // 2]
            rate = nbytes / (med["op"] * 1e-3)
            note = ""
            if med["op"] > med["loop"]:
                note = "   THE OP IS SLOWER THAN THE LOOP"
                slower.append(f"{shape} {str(dtype).split('.')[-1]} {step}")
            print(f"  {step:17s} op {med['op']:8.3f} ms ({t['op'][0]:.3f} - {t['op'][-1]:.3f})   loop {med['loop']:8.3f} ms "
                  f"({t['loop'][0]:.3f} - {t['loop'][-1]:.3f})   x{med['loop'] / med['op']:.2f};  median (min - max) of {a.reps};  "
                  f"op: {nbytes / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s = {rate / HBM_BYTES_PER_S:.2f} of 8 TB/s{note}")
        del x, x0, flat, grads
        th.cuda.empty_cache()
    print("slower than the loop: " + (", ".join(slower) if slower else "nowhere"))


if __name__ == "__main__":
    main()
