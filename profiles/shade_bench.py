#!/usr/bin/env python3
"""shade at the headline shape -- 8 views of 2048 x 2048, C = 3, float32 -- forward, and forward + backward to every
floating-point argument, with and without the highlight, albedo as a vector and as an image: the HIP route
(csrc/shade.hip) against the eager PyTorch formulation of the same definition on the same card in the same run.

The scene is a shaded sphere in front of a background image (about half of the pixels are foreground), index image,
background and gamma = 2.2 always on.  Both routes are timed with device events after warm-up, alternating, `--rounds`
times each, over windows of about `--window-ms`; reported are the median and the spread (min ... max) of the rounds, and
HIP counts as faster only when its slowest round beats the eager route's fastest.  Then each kernel's time from the
library's own timing collection, with the bytes the algorithm must move at least once (from the shapes and the foreground
share) and their rate as a fraction of the 8 TB/s HBM figure.

    timeout -k 10 500 python profiles/shade_bench.py
"""
import argparse
import os
import statistics
import sys

import torch as th
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drtk_amd  # noqa: E402
from drtk_amd import capi  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12


def eager_shade(normal_img, light_dir, albedo, ambient, index_img, pos_img, specular, shininess, background, gamma):
    """The definition in eager PyTorch, parameters [C] / [1]: what a render-and-compare step writes without the kernel"""
    col = lambda p: p.view(1, -1, 1, 1)  # noqa: E731
    L = F.normalize(light_dir, dim=0).view(1, 3, 1, 1)
    n = F.normalize(normal_img, dim=1)
    d = (-(n * L).sum(1, keepdim=True)).clamp(min=0)
    img = (albedo if albedo.ndim == 4 else col(albedo)) * (d + col(ambient))
    if specular is not None:
        h = F.normalize(L - F.normalize(pos_img, dim=1), dim=1)
        img = img + (-(h * n).sum(1, keepdim=True)).clamp(min=1e-8) ** col(shininess) * col(specular)
    img = th.where((index_img != -1)[:, None], img, background)
    return th.pow(img.clamp(min=0), 1.0 / gamma)


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
    iters = max(5, min(2000, int(window_ms / max(_window_ms(fn, 3) / 3, 1e-3))))
    return _window_ms(fn, iters) / iters


def scene(N, H, W):
    """A unit sphere at z = 3 seen from the origin: normals, camera-space positions, an index image (-1 off the sphere)"""
    y, x = th.meshgrid(th.linspace(-1.4, 1.4, H, device=DEV), th.linspace(-1.4, 1.4, W, device=DEV), indexing="ij")
    r2 = x * x + y * y
    z = -(1 - r2).clamp(min=0).sqrt()
    normal = th.stack([x, y, z], 0)[None].repeat(N, 1, 1, 1)
    k = th.arange(N, device=DEV).view(N, 1, 1, 1)
    normal = normal * (1 + 0.05 * k)  # (unnormalised, and not the same in every view)
    pos = normal + th.tensor([0.0, 0.0, 3.0], device=DEV).view(1, 3, 1, 1)
    index = th.where(r2 < 1, 1, -1).int()[None].repeat(N, 1, 1).contiguous()
    return normal.contiguous(), pos.contiguous(), index


def algorithmic_bytes(N, C, H, W, fg, specular, albedo_img, es=4):
    """(forward, backward) bytes that must move at least once: a foreground pixel reads its normals (positions, albedo), a
    background pixel its background, every pixel its index and writes its output; the backward reads grad_out and the same
    inputs again and writes every requested image gradient at every pixel."""
    px = N * H * W
    fg_in = (3 + (3 if specular else 0) + (C if albedo_img else 0)) * es
    inputs = px * (fg * fg_in + (1 - fg) * C * es + 4)
    grads = px * (3 + (3 if specular else 0) + (C if albedo_img else 0) + C) * es
    return inputs + px * C * es, inputs + px * C * es + grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--window-ms", type=float, default=200.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert th.cuda.is_available(), "shade_bench.py measures on the GPU; there is no CPU fall-back"
    N, C, H, W = a.views, 3, a.size, a.size
    normal, pos, index = scene(N, H, W)
    fg = float((index != -1).float().mean())
    gen = th.Generator(DEV).manual_seed(1)
    bg = th.rand(N, C, H, W, device=DEV, generator=gen) * 0.9 + 0.05
    albedo_img = th.rand(N, C, H, W, device=DEV, generator=gen) * 0.9 + 0.05
    g = th.randn(N, C, H, W, device=DEV, generator=gen)
    t = lambda *x: th.tensor(x, device=DEV)  # noqa: E731
    light, albedo, ambient, spec, shin = t(0.3, 0.4, 0.85), t(0.8, 0.6, 0.5), t(0.2, 0.25, 0.3), t(0.5, 0.5, 0.6), t(16.0)
    print(f"{N} views of {H} x {W}, C = {C}, float32, {fg:.2f} of the pixels foreground, index image, background and gamma = 2.2")

    ok = True
    for specular in (True, False):
        for image in (False, True):
            tensors = [normal, light, albedo_img if image else albedo, ambient] + ([pos, spec, shin] if specular else []) + [bg]

            def call(fn, leaves):
                n, l, al, am = leaves[:4]
                p, sp, sh = leaves[4:7] if specular else (None, None, None)
                return fn(n, l, al, am, index, p, sp, sh, leaves[-1], 2.2)

            def fwd(fn):
                return lambda: call(fn, tensors)

            def fwd_bwd(fn):
                def run():
                    call(fn, [x.detach().requires_grad_(True) for x in tensors]).backward(g)
                return run

            want = call(eager_shade, [x.double() for x in tensors])
            for name, fn in (("hip", drtk_amd.shade), ("eager", eager_shade)):
                err = float((call(fn, tensors).double() - want).abs().max() / want.abs().max())
                print(f"  {name:6s} max |out - f64| / max|f64| = {err:.2e}")
                assert err < 1e-4, name
            del want
            what = f"{'with' if specular else 'without'} specular, albedo {'image' if image else 'vector'}"
            for mode, make in (("forward", fwd), ("forward + backward", fwd_bwd)):
                routes = {"hip": make(drtk_amd.shade), "eager": make(eager_shade)}
                times = {name: [] for name in routes}
                for _ in range(a.rounds):  # alternating: a drift of the machine hits both routes alike
                    for name, fn in routes.items():
                        times[name].append(time_ms(fn, a.window_ms))
                print(f"{what}: {mode}")
                for name, ts in times.items():
                    print(f"  {name:6s} median {statistics.median(ts):8.3f} ms   spread {min(ts):8.3f} ... {max(ts):8.3f} ms")
                faster = max(times["hip"]) < min(times["eager"])
                ok &= faster
                print(f"  hip vs eager: {statistics.median(times['eager']) / statistics.median(times['hip']):.2f}x, "
                      f"{'faster beyond the spread' if faster else 'NOT separated from it by the spread'}")
            # per kernel: the library's own event timing around a few steps
            th.cuda.synchronize()
            capi.kernel_timing_begin()
            for _ in range(10):
                fwd_bwd(drtk_amd.shade)()
            th.cuda.synchronize()
            need = dict(zip(("shade_forward_kernel", "shade_backward_kernel"), algorithmic_bytes(N, C, H, W, fg, specular, image)))
            print("  kernels (per launch; bytes: what the algorithm must move at least once)")
            for name, (count, ms) in capi.kernel_timing_report().items():
                per = ms / count
                nbytes = need.get(name.split("<")[0])
                frac = f"{nbytes / (per * 1e-3) / HBM:5.2f} of 8 TB/s on {nbytes / 1e6:8.1f} MB ({nbytes / (N * H * W):.0f} B/px)" if nbytes else ""
                print(f"    {name:34s} {count:4d} launches  {per * 1e3:9.1f} us  {frac}")
    print("verdict:", "HIP faster than the eager formulation beyond the spread in every row" if ok else "see the rows marked NOT")


if __name__ == "__main__":
    main()
