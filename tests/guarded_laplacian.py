"""The C-ABI entry points of the mesh regulariser -- drtk_amd_geometry_cot_weights, _cot_weights_backward, _laplacian (with
its workspace) and _laplacian_grad_weights -- through the ctypes binding with every output and workspace between sentinel
elements (DRTK_CAPI_GUARD, drtk_amd/capi.py `_out`), on the structural cases of tests/laplacian_oracle.py: ragged channel
groups, one lane past a block, chunked rows with shared and per-view topology, degenerate faces.  Each case is compared
with the oracle under the bounds of tests/test_gpu_laplacian.py (the guard also leaves every output merely element-aligned),
shared and absent weights included, and after each `capi.check_guards()`.  Not collected by pytest;
tests/test_gpu_laplacian.py starts it in a child process:

    DRTK_CAPI_GUARD=1 DRTK_CAPI_POISON=1 python tests/guarded_laplacian.py [--only NAME]
    python tests/guarded_laplacian.py --list                (no GPU needed)"""
import argparse
import os
import sys

import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
TAG = {th.float32: "f32", th.float64: "f64"}


def pipeline_case(name, dtype):
    import test_gpu_laplacian as T

    T.check_case(name, dtype, "capi")


def shared_and_uniform_case(name, dtype):
    """One weight set for all views ([1,F,3]: the gradient summed over the views) and no weights at all"""
    import laplacian_oracle as O
    from drtk_amd import capi
    from f64_distance import assert_within_f64_distance

    v, x, grad, vi = O.case(name)
    x, grad = x.to(dtype), grad.to(dtype)
    w = O.cot_weights(v, vi)[:1].to(dtype)
    V = x.shape[1]
    inc = capi.vertex_incidence_numpy(vi.numpy(), V)
    xd, gd, vi32 = x.to(DEV), grad.to(DEV), vi.to(DEV).int()
    got = [capi.geometry_laplacian(xd, vi32, inc, w.to(DEV)), capi.geometry_laplacian_grad_weights(gd, xd, vi32, shared_weights=True),
           capi.geometry_laplacian(xd, vi32, inc, None)]

    def oracle(dt):
        ww = w.to(dt).clone().requires_grad_(True)
        out = O.mesh_laplacian(x.to(dt), vi, ww)
        out.backward(grad.to(dt))
        return [out.detach(), ww.grad, O.mesh_laplacian(x.to(dt), vi)]

    r64, r32 = oracle(th.float64), oracle(th.float32)
    for what, a, b32, b64 in zip(("out", "grad_w", "uniform"), got, r32, r64):
        a = a.cpu()
        assert a.shape == b64.shape, (what, a.shape, b64.shape)
        if dtype == th.float64:
            assert float((a - b64).abs().max()) <= 1e-12 * float(b64.abs().max()), what
        else:
            assert_within_f64_distance(a, b32, b64, f"{name} {what}")


def cases():
    """[(name, function, arguments)], in the order they run"""
    import laplacian_oracle as O

    out = []
    for name in O.CASES:
        for dtype in (th.float32, th.float64):
            out.append((f"pipeline/{name}/{TAG[dtype]}", pipeline_case, (name, dtype)))
    for name in ("soup257_c5_n3", "fan600_shared", "fan300_per_view", "degenerate_shared"):
        for dtype in (th.float32, th.float64):
            out.append((f"shared_and_uniform/{name}/{TAG[dtype]}", shared_and_uniform_case, (name, dtype)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the names of the cases and leave (no GPU needed)")
    ap.add_argument("--only", metavar="NAME", help="run the cases called NAME or NAME/...")
    a = ap.parse_args()
    todo = cases()
    if a.only:
        todo = [c for c in todo if c[0] == a.only or c[0].startswith(a.only + "/")]
        assert todo, f"no case is called {a.only}"
    if a.list:
        print("\n".join(c[0] for c in todo))
        sys.exit(0)
    from drtk_amd import capi

    assert capi._GUARD > 0 and capi._POISON, "run with DRTK_CAPI_GUARD=g (g = 1, 2, 3) and DRTK_CAPI_POISON=1 in the environment"
    bad = 0
    for name, fn, args in todo:
        try:
            fn(*args)
            checked = capi.check_guards()
            assert checked >= 1, "the case went through no allocation of the binding"
        except AssertionError as e:
            bad += 1
            print(f"FAIL {name}: {str(e)[:600]}", flush=True)
        except Exception as e:  # an error of the runtime or the library: nothing more is started on the device
            print(f"ERROR {name}: {type(e).__name__}: {str(e)[:600]}\nstopped after {name}", flush=True)
            sys.exit(2)
    print(f"{len(todo) - bad}/{len(todo)} cases passed (DRTK_CAPI_GUARD={capi._GUARD})")
    sys.exit(1 if bad else 0)
