#!/usr/bin/env python3
"""grid_scatter against the only other way to get its result on PyTorch-ROCm: the adjoint of torch's own device
grid_sample (zero texture -> F.grid_sample -> backward with `input` as cotangent), on the same card.

    python profiles/grid_scatter_bench.py [--iters 30] [--rounds 5] [--json out.json]

Per case, forward and backward separately:
  ours       drtk_amd.capi.grid_scatter_2d / grid_scatter_2d_backward (the C ABI the operator calls; output zero fill included)
  yardstick  forward:  tex = zeros(requires_grad); autograd.grad(F.grid_sample(tex, grid), tex, input)
             backward: s = F.grid_sample(grad_out, grid_leaf); autograd.grad(s, grid_leaf, input)   (s is grad_input)
Timing: device events around `iters` back-to-back calls after a warm-up of every shape, `rounds` such windows per side,
the two sides alternating (other work shares the machine: a difference is read against the spread of the rounds); the
median window is reported, with min - max.  Before timing, the two sides' results are compared.
Also reported: the kernel route taken (workgroups windowed / direct, from the C ABI's route counters) and the float
atomic traffic of the forward -- the bytes added to global memory, counted from the grid (one add per touched texel,
channel and 16 x 16 tile on the windowed route, one per in-range tap and channel on the direct route) -- over the
forward time, against the ~1.3 TB/s of added bytes the card sustains for contiguous row segments.
A separate tool: bench.py (the flagship workload) does not call it."""
import argparse
import json
import math
import os
import sys

import torch as th
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drtk_amd import capi  # noqa: E402

DEV = "cuda:0"
MODE = {"bilinear": 0, "bicubic": 2}
PAD = {"zeros": 0, "border": 1, "reflection": 2}


def warp_grid(N, H, W, dtype, gen):
    ys, xs = th.meshgrid(th.linspace(-1, 1, H, dtype=th.float64), th.linspace(-1, 1, W, dtype=th.float64), indexing="ij")
    ph = th.rand(N, 4, generator=gen, dtype=th.float64) * 6.28
    gx = xs[None] + 0.08 * th.sin(3 * ys[None] + ph[:, 0, None, None]) + 0.05 * th.cos(2 * xs[None] + ph[:, 1, None, None])
    gy = ys[None] + 0.08 * th.cos(2 * xs[None] + ph[:, 2, None, None]) + 0.05 * th.sin(3 * ys[None] + ph[:, 3, None, None])
    return (th.stack([gx, gy], -1) * 0.86).to(dtype)


def make(case):
    gen = th.Generator().manual_seed(case["seed"])
    N, C, H, W, oh, ow, dtype = case["N"], case["C"], case["H"], case["W"], case["oh"], case["ow"], case["dtype"]
    inp = (th.rand(N, C, H, W, generator=gen) * 2 - 1).to(dtype)
    gout = (th.rand(N, C, oh, ow, generator=gen) * 2 - 1).to(dtype)
    if case["grid"] == "warp":
        grid = warp_grid(N, H, W, dtype, gen)
    elif case["grid"] == "random":
        grid = (th.rand(N, H, W, 2, generator=gen) * 2 - 1).to(dtype)
    else:  # every pixel on one texel neighbourhood
        grid = th.tensor([0.137, -0.291], dtype=dtype).expand(N, H, W, 2).contiguous()
    return inp.to(DEV), grid.to(DEV), gout.to(DEV)


def atomic_bytes(grid, oh, ow, C, mode, windowed, elem):
    """Bytes the forward adds to global memory, counted from the grid (align_corners=False, taps clipped to the image;
    the cell of a tap is taken from a float64 evaluation -- a count, not a result)."""
    N, H, W, _ = grid.shape
    g = grid.double()
    x, y = ((g[..., 0] + 1) * ow - 1) / 2, ((g[..., 1] + 1) * oh - 1) / 2
    x, y = x.clamp(0, ow - 1), y.clamp(0, oh - 1)  # border padding
    taps = range(0, 2) if mode == "bilinear" else range(-1, 3)
    fx, fy = th.floor(x).long(), th.floor(y).long()
    if not windowed:
        n = 0
        for i in taps:
            for j in taps:
                n += int((((fx + i) >= 0) & ((fx + i) < ow) & ((fy + j) >= 0) & ((fy + j) < oh)).sum()) if mode == "bilinear" else N * H * W
        return n * C * elem
    ty, tx = th.arange(H, device=grid.device) // 16, th.arange(W, device=grid.device) // 16
    tile = (ty[:, None] * ((W + 15) // 16) + tx[None, :])[None] + th.arange(N, device=grid.device)[:, None, None] * (((H + 15) // 16) * ((W + 15) // 16))
    total = 0
    keys = []
    for i in taps:
        for j in taps:
            cx, cy = (fx + i).clamp(0, ow - 1), (fy + j).clamp(0, oh - 1)
            if mode == "bilinear":
                ok = ((fx + i) < ow) & ((fy + j) < oh)
                keys.append((tile * (oh * ow) + cy * ow + cx)[ok])
            else:
                keys.append((tile * (oh * ow) + cy * ow + cx).reshape(-1))
    total = int(th.unique(th.cat(keys)).numel())
    return total * C * elem


def window(fn, iters):
    th.cuda.synchronize()
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    th.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare_sides(a, b, what, check=True):
    a, b = a.double(), b.double()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert not check or err <= 1e-4 * scale + 1e-30, f"{what}: the two sides differ by {err:.3e} on a scale of {scale:.3e}"
    return err / max(scale, 1e-300)


def run_case(case, iters, rounds):
    inp, grid, gout = make(case)
    mode, pad, oh, ow = case["mode"], "border", case["oh"], case["ow"]
    m, p = MODE[mode], PAD[pad]

    def ours_fwd():
        return capi.grid_scatter_2d(inp, grid, oh, ow, p, m, False)

    def yard_fwd():
        tex = th.zeros(inp.shape[0], inp.shape[1], oh, ow, dtype=inp.dtype, device=DEV, requires_grad=True)
        s = F.grid_sample(tex, grid, mode=mode, padding_mode=pad, align_corners=False)
        return th.autograd.grad(s, tex, inp)[0]

    def ours_bwd():
        return capi.grid_scatter_2d_backward(gout, inp, grid, p, m, False)

    def yard_bwd():
        g = grid.detach().requires_grad_(True)
        s = F.grid_sample(gout, g, mode=mode, padding_mode=pad, align_corners=False)
        return s.detach(), th.autograd.grad(s, g, inp)[0]

    counts = th.zeros(2, dtype=th.int32, device=DEV)
    out = capi.grid_scatter_2d(inp, grid, oh, ow, p, m, False, route_counts=counts)
    routes = counts.tolist()
    # (millions of float32 terms on one texel: either side's sum is a matter of order; reported, not asserted)
    rel = {"fwd": compare_sides(out, yard_fwd(), case["name"] + " forward", check=case["grid"] != "one")}
    if case["grid"] != "one":  # (the grid gradient at one shared location is compared by the tests, per element)
        (gi, gg), (yi, yg) = ours_bwd(), yard_bwd()
        rel["grad_input"] = compare_sides(gi, yi, case["name"] + " grad_input")
    res = {"name": case["name"], "routes": routes, "rel_diff": rel}
    for tag, ours, yard in (("fwd", ours_fwd, yard_fwd), ("bwd", ours_bwd, yard_bwd)):
        for fn in (ours, yard):
            for _ in range(3):
                fn()
        t = {"ours": [], "yardstick": []}
        for _ in range(rounds):  # alternating windows
            t["ours"].append(window(ours, iters))
            t["yardstick"].append(window(yard, iters))
        for k, v in t.items():
            v.sort()
            res[f"{tag}_{k}_ms"] = v[len(v) // 2]
            res[f"{tag}_{k}_range_ms"] = (v[0], v[-1])
        res[f"{tag}_speedup"] = res[f"{tag}_yardstick_ms"] / res[f"{tag}_ours_ms"]
    elem = inp.element_size()
    nb = atomic_bytes(grid, oh, ow, inp.shape[1], mode, routes[0] >= routes[1], elem)
    res["atomic_bytes"] = nb
    res["atomic_TBps"] = nb / (res["fwd_ours_ms"] * 1e-3) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert th.cuda.is_available(), "grid_scatter_bench needs a GPU: there is no CPU path to time"
    S = 128 if a.small else 1024
    base = dict(N=2 if a.small else 8, C=4, H=S, W=S, oh=S, ow=S, dtype=th.float32, seed=1)
    cases = [
        dict(base, name="smooth warp, bilinear", grid="warp", mode="bilinear"),
        dict(base, name="smooth warp, bicubic", grid="warp", mode="bicubic"),
        dict(base, name="random grid, bilinear", grid="random", mode="bilinear"),
        dict(base, name="all to one texel, bilinear", grid="one", mode="bilinear"),
        dict(base, name="smooth warp, bilinear, float64", grid="warp", mode="bilinear", dtype=th.float64),
        dict(base, name="smooth warp, bicubic, float64", grid="warp", mode="bicubic", dtype=th.float64),
    ]
    results = [run_case(c, a.iters, a.rounds) for c in cases]
    print(f"{base['N']} x {S}^2 -> {S}^2, C = 4, border padding; median of {a.rounds} windows of {a.iters} calls, ms (min - max)")
    print("| case | route (windowed / direct tiles) | fwd ours | fwd yardstick | x | bwd ours | bwd yardstick | x | fwd atomic bytes | TB/s added |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        f = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_range_ms'][0]:.3f} - {r[k + '_range_ms'][1]:.3f})"  # noqa: E731
        print(f"| {r['name']} | {r['routes'][0]} / {r['routes'][1]} | {f('fwd_ours')} | {f('fwd_yardstick')} | {r['fwd_speedup']:.2f} | "
              f"{f('bwd_ours')} | {f('bwd_yardstick')} | {r['bwd_speedup']:.2f} | {r['atomic_bytes'] / 1e6:.1f} MB | {r['atomic_TBps']:.3f} |")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)
    assert all(math.isfinite(r["fwd_ours_ms"]) for r in results)


if __name__ == "__main__":
    main()
