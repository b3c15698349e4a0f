#!/usr/bin/env python3
"""drtk_amd.forward_kinematics (forward, forward + backward to the pose, the rest joints and the translation), float32, a
hand (J = 16), a body (J = 24) and a 128-joint random tree of 12 levels, N = 8 and N = 1024 views: the HIP route
(csrc/kinematics.hip) against

  loop       what users write: batch_rodrigues (angle = |r + 1e-8|, I + sin K + (1 - cos) K K), a Python loop over the
             joints with one 4x4 matmul each, a stack, and the inverse-bind correction -- eager PyTorch on the same card
             in the same run;

and, at 8 views and 50 400 vertices, forward_kinematics + skin against that loop + the gather formulation of skin
(drtk_amd/skin.py).  Whole calls are timed with device events after warm-up, alternating, `--rounds` windows each;
reported are the median and the spread (min ... max) of the windows, and HIP counts as faster only when its slowest
window beats the baseline's fastest.  Then the kernels' own times from the library's timing collection.  The data is a
few kilobytes: what is measured is launches and dependent latency, so no bandwidth fraction is stated.

    timeout -k 10 500 python profiles/kinematics_bench.py
"""
import argparse
import os
import statistics
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drtk_amd  # noqa: E402
from drtk_amd import capi  # noqa: E402
from drtk_amd.skin import _skin_torch  # noqa: E402

DEV = "cuda:0"
HAND = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
BODY = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]


def tree128(gen):
    """128 joints on 12 levels: joint j >= 1 sits on level 1 + (j - 1) % 11 under a random earlier joint of the level above"""
    level, parents = [0], [-1]
    for j in range(1, 128):
        lv = 1 + (j - 1) % 11
        above = [i for i in range(j) if level[i] == lv - 1]
        parents.append(above[int(th.randint(0, len(above), (1,), generator=gen))])
        level.append(lv)
    return parents


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


def batch_rodrigues(r):
    """[B,3] -> [B,3,3], the way rig code writes it"""
    angle = th.norm(r + 1e-8, dim=1, keepdim=True)
    axis = r / angle
    cos, sin = th.cos(angle)[:, None], th.sin(angle)[:, None]
    rx, ry, rz = th.split(axis, 1, dim=1)
    zeros = th.zeros_like(rx)
    k = th.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    return th.eye(3, dtype=r.dtype, device=r.device)[None] + sin * k + (1 - cos) * th.bmm(k, k)


def loop_fk(rotations, joints, parents, translation):
    """batch_rodrigues + a matmul per joint + the inverse bind: (transforms [N,J,3,4], posed [N,J,3])"""
    n, num_j = rotations.shape[:2]
    rot = batch_rodrigues(rotations.reshape(-1, 3)).view(n, num_j, 3, 3)
    c = joints[None].expand(n, -1, -1)
    rel = c.clone()
    rel[:, 1:] = c[:, 1:] - c[:, parents[1:]]
    rel[:, 0] = rel[:, 0] + translation
    bottom = th.tensor([0.0, 0.0, 0.0, 1.0], dtype=rot.dtype, device=rot.device).expand(n, num_j, 1, 4)
    local = th.cat([th.cat([rot, rel[..., None]], -1), bottom], -2)
    chain = [local[:, 0]]
    for j in range(1, num_j):
        chain.append(th.matmul(chain[parents[j]], local[:, j]))
    world = th.stack(chain, 1)
    posed = world[:, :, :3, 3]
    shift = th.matmul(world[:, :, :3, :3], c[..., None])
    transforms = th.cat([world[:, :, :3, :3], world[:, :, :3, 3:] - shift], -1)
    return transforms, posed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=100.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--vertices", type=int, default=50400)
    a = ap.parse_args()
    assert th.cuda.is_available(), "kinematics_bench.py measures on the GPU; there is no CPU fall-back"
    cpu_gen = th.Generator().manual_seed(3)
    gen = th.Generator(DEV).manual_seed(1)
    rigs = (("hand", HAND), ("body", BODY), ("tree128", tree128(cpu_gen)))
    ok = True

    def report(what, times):
        nonlocal ok
        print(what)
        for name, tm in times.items():
            print(f"  {name:8s} median {statistics.median(tm):8.3f} ms   spread {min(tm):8.3f} ... {max(tm):8.3f} ms")
        faster = max(times["hip"]) < min(times["loop"])
        ok &= faster
        print(f"  hip vs loop: {statistics.median(times['loop']) / statistics.median(times['hip']):.1f}x, "
              f"{'slowest hip window beats its fastest' if faster else 'NOT separated from it by the spread'}")

    for rig_name, parents in rigs:
        J = len(parents)
        depth = [0] * J
        for j, p in enumerate(parents):
            depth[j] = 0 if p < 0 else depth[p] + 1
        ptensor = th.tensor(parents, dtype=th.int32, device=DEV)
        for N in (8, 1024):
            theta = 0.5 * th.randn(N, 3 + 3 * J, device=DEV, generator=gen)
            joints = 0.3 * th.randn(J, 3, device=DEV, generator=gen)
            tr = th.randn(N, 3, device=DEV, generator=gen)
            gA, gP = th.randn(N, J, 3, 4, device=DEV, generator=gen), th.randn(N, J, 3, device=DEV, generator=gen)
            print(f"rig {rig_name}: J = {J}, {max(depth) + 1} levels, {N} views, float32")
            routes = {"hip": lambda r, c, t: drtk_amd.forward_kinematics(r, c, ptensor, t), "loop": lambda r, c, t: loop_fk(r, c, parents, t)}
            pose = theta[:, 3:].view(N, J, 3)
            ref = drtk_amd.forward_kinematics(pose.double().cpu(), joints.double().cpu(), parents, tr.double().cpu())
            for name, fn in routes.items():
                out = fn(pose, joints, tr)
                err = max(float((o.double().cpu() - r).abs().max() / r.abs().max()) for o, r in zip(out, ref))
                print(f"  {name:8s} max |out - f64| / max|f64| = {err:.2e}")
                assert err < 1e-4, name

            def fwd(fn):
                return lambda: fn(theta[:, 3:].view(N, J, 3), joints, tr)

            def fwd_bwd(fn):
                def run():
                    th_, c, t = theta.detach().requires_grad_(True), joints.detach().requires_grad_(True), tr.detach().requires_grad_(True)
                    transforms, posed = fn(th_[:, 3:].view(N, J, 3), c, t)
                    th.autograd.backward((transforms, posed), (gA, gP))
                return run

            for what, make in (("forward", fwd), ("forward + backward (pose, joints, translation)", fwd_bwd)):
                times = {name: [] for name in routes}
                for _ in range(a.rounds):  # alternating: a drift of the machine hits every route alike
                    for name, fn in routes.items():
                        times[name].append(time_ms(make(fn), a.window_ms))
                report(what, times)

            th.cuda.synchronize()
            capi.kernel_timing_begin()
            for _ in range(10):
                fwd_bwd(routes["hip"])()
            th.cuda.synchronize()
            print("  kernels (per launch)")
            for name, (count, ms) in capi.kernel_timing_report().items():
                print(f"    {name:56s} {count:4d} launches  {ms / count * 1e3:9.1f} us")

    # pose -> skinned vertices: forward_kinematics + skin against the loop + the gather formulation of skin
    N, V, K = 8, a.vertices, 4
    for rig_name, parents in rigs[:2]:
        J = len(parents)
        ptensor = th.tensor(parents, dtype=th.int32, device=DEV)
        theta = 0.5 * th.randn(N, 3 + 3 * J, device=DEV, generator=gen)
        joints = 0.3 * th.randn(J, 3, device=DEV, generator=gen)
        tr = th.randn(N, 3, device=DEV, generator=gen)
        v = th.randn(V, 3, device=DEV, generator=gen)
        idx = th.randint(0, J, (V, K), device=DEV, generator=gen)
        w = th.softmax(th.randn(V, K, device=DEV, generator=gen), 1)
        g = th.randn(N, V, 3, device=DEV, generator=gen)
        drtk_amd.skin(v, idx, w, drtk_amd.forward_kinematics(theta[:, 3:].view(N, J, 3), joints, ptensor, tr)[0])  # (the caches)
        print(f"rig {rig_name}: J = {J}, {N} views, {V} vertices, K = {K}, float32: pose -> skinned vertices")
        routes = {"hip": (lambda r, c, t: drtk_amd.forward_kinematics(r, c, ptensor, t), drtk_amd.skin),
                  "loop": (lambda r, c, t: loop_fk(r, c, parents, t), _skin_torch)}

        def fwd(fk, skin):
            return lambda: skin(v, idx, w, fk(theta[:, 3:].view(N, J, 3), joints, tr)[0])

        def fwd_bwd(fk, skin):
            def run():
                th_, c, t = theta.detach().requires_grad_(True), joints.detach().requires_grad_(True), tr.detach().requires_grad_(True)
                skin(v, idx, w, fk(th_[:, 3:].view(N, J, 3), c, t)[0]).backward(g)
            return run

        for what, make in (("forward_kinematics + skin, forward", fwd), ("forward_kinematics + skin, forward + backward to the pose", fwd_bwd)):
            times = {name: [] for name in routes}
            for _ in range(a.rounds):
                for name, (fk, skin) in routes.items():
                    times[name].append(time_ms(make(fk, skin), a.window_ms))
            report(what, times)
    print("verdict:", "HIP beats the loop beyond the spread in every row" if ok else "see the rows marked NOT")


if __name__ == "__main__":
    main()
