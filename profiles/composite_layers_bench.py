#!/usr/bin/env python3
"""composite_layers against the loop it replaces, in eager PyTorch: 8 views of 2048 x 2048, K = 4 layers, C = 3, float32,
rgba form ([N,K,C+1,H,W], what interpolate(...).unflatten(0, (N, K)) gives), with index_img and a background.

    python profiles/composite_layers_bench.py [--reps 25] [--small]

Two occupancies:
  full     every layer present at every pixel;
  layered  layers 0 ... 3 present on 100 / 50 / 25 / 12 % of the pixels, -1 entries trailing: layer k covers a centred
           rectangle of that share of the image (a mesh's deeper layers are regions, not salt and pepper).
Both contenders run in this process on the same card, alternating call by call: `reps` repetitions each of forward and of
forward + backward (torch.autograd.backward of (img, T) with given upstream gradients: no loss glue on either side), after
a warm-up of both, each repetition between two device events; the median is printed with min - max.

Algorithmic bytes per pixel (float32; f_k = share of pixels where layer k is present, F = sum f_k; absent layers cost their
4 bytes of index and nothing else, and gradients are written in full, zeros included):
  forward    4 K (index) + 4 (C + 1) F (rgba) + 4 C (background) + 4 (C + 1) (img, T)
  backward   4 K (index) + 4 (C + 1) F (rgba) + 4 C (background) + 4 (C + 1) (grad_img, grad_T)
             + 4 K (C + 1) (grad_rgba) + 4 C (grad_background)
and forward + backward is their sum; over the op's time, as a share of the 8 TB/s of BASELINE.md.  (The backward kernel
reads grad_img twice; the second pass is not counted: it is the kernel's choice, not the algorithm's.)
The one condition: the op must not be slower than the loop, at either occupancy, forward or forward + backward -- the
script exits with status 1 if it is.  A separate tool: bench.py does not call it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E, nominal
SHARES = (1.0, 0.5, 0.25, 0.12)


def loop(rgba, index, background):
    """INTEGRATION.md, "Layers": the definition."""
    import torch as th

    N, K, C1, H, W = rgba.shape
    C = C1 - 1
    img, T = rgba.new_zeros(N, C, H, W), rgba.new_ones(N, 1, H, W)
    for k in range(K):
        a = rgba[:, k, C:] * (index[:, k:k + 1] != -1)
        img = img + (T * a) * rgba[:, k, :C]
        T = T * (1 - a)
    return img + T * background, T


def make(small, layered):
    import torch as th

    dev = "cuda:0"
    N, K, C, S = (2, 4, 3, 256) if small else (8, 4, 3, 2048)
    g = th.Generator(device=dev).manual_seed(1)
    rgba = th.rand(N, K, C + 1, S, S, generator=g, device=dev)
    index = th.randint(0, 100000, (N, K, S, S), generator=g, device=dev, dtype=th.int32)
    if layered:
        ys, xs = th.meshgrid(th.arange(S, device=dev), th.arange(S, device=dev), indexing="ij")
        for k, share in enumerate(SHARES[:K]):
            half = S * share ** 0.5 / 2
            inside = ((ys + 0.5 - S / 2).abs() < half) & ((xs + 0.5 - S / 2).abs() < half)
            index[:, k] = th.where(inside, index[:, k], -1)
    bg = th.rand(N, C, S, S, generator=g, device=dev)
    g_img = th.rand(N, C, S, S, generator=g, device=dev) * 2 - 1
    g_T = th.rand(N, 1, S, S, generator=g, device=dev) * 2 - 1
    return rgba, index, bg, g_img, g_T


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

    assert th.cuda.is_available(), "composite_layers_bench needs a GPU: there is no CPU path to time"
    slower = []
    for layered in (False, True):
        rgba0, index, bg0, g_img, g_T = make(a.small, layered)
        N, K, C1, H, W = rgba0.shape
        C = C1 - 1
        shares = [float((index[:, k] != -1).float().mean()) for k in range(K)]
        F = sum(shares)
        fwd_bytes = 4 * K + 4 * (C + 1) * F + 4 * C + 4 * (C + 1)
        bwd_bytes = 4 * K + 4 * (C + 1) * F + 4 * C + 4 * (C + 1) + 4 * K * (C + 1) + 4 * C
        pixels = N * H * W

        def op(x, b):
            return drtk_amd.composite_layers(x, index_img=index, background=b)

        def lp(x, b):
            return loop(x, index, b)

        with th.no_grad():
            got, want = op(rgba0, bg0), lp(rgba0, bg0)
            assert th.equal(got[0], want[0]) and th.equal(got[1], want[1]), "the op and the loop disagree"
        del got, want
        rgba, bg = rgba0.clone().requires_grad_(True), bg0.clone().requires_grad_(True)

        def forward(f):
            with th.no_grad():
                f(rgba0, bg0)

        def both(f):
            rgba.grad = bg.grad = None
            th.autograd.backward(f(rgba, bg), (g_img, g_T))

        name = "layered" if layered else "full"
        print(f"{name}: {N} x {H} x {W}, K = {K}, C = {C}, float32, rgba + index + background; layers present on "
              + " / ".join(f"{100 * s:.0f}" for s in shares) + " % of the pixels")
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
            rate = nbytes * pixels / (med["op"] * 1e-3)
            print(f"  {step:17s} op {med['op']:8.3f} ms ({t['op'][0]:.3f} - {t['op'][-1]:.3f})   loop {med['loop']:8.3f} ms "
                  f"({t['loop'][0]:.3f} - {t['loop'][-1]:.3f})   x{med['loop'] / med['op']:.2f};  median (min - max) of {a.reps};  "
                  f"op: {nbytes:.1f} B/px -> {rate / 1e12:.2f} TB/s = {rate / HBM_BYTES_PER_S:.2f} of 8 TB/s")
            if med["op"] > med["loop"]:
                slower.append(f"{name} {step}")
        th.cuda.empty_cache()
    if slower:
        sys.exit("composite_layers_bench: the op is slower than the loop: " + ", ".join(slower))


if __name__ == "__main__":
    main()
