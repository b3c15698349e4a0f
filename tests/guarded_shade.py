"""The C-ABI entry points of shade -- drtk_amd_shade_forward, drtk_amd_shade_backward and its workspace -- through the ctypes
binding with every output and workspace between sentinel elements (DRTK_CAPI_GUARD, drtk_amd/capi.py `_out`), on the
structural cases of tests/shade_oracle.py: plane sizes around a lane's and a workgroup's pixel count, row counts around the
finalize kernel's pass, every view and channel count, shared and per-view parameters, every combination of options.  Each
case is compared with the oracle under the bounds of tests/test_gpu_shade.py (the guard also leaves every output merely
element-aligned), once with every gradient and once with the image gradients alone, and after each `capi.check_guards()`.
Not collected by pytest; tests/test_gpu_shade.py starts it in a child process:

    DRTK_CAPI_GUARD=1 DRTK_CAPI_POISON=1 python tests/guarded_shade.py [--only NAME]
    python tests/guarded_shade.py --list                (no GPU needed)"""
import argparse
import os
import sys

import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

TAG = {th.float32: "f32", th.float64: "f64"}


def oracle_case(name, dtype):
    import test_gpu_shade as T

    T.check_case(name, dtype, "capi")


def images_only_case(name, dtype):
    """No parameter gradient: no workspace, no finalize launch, the same image gradients"""
    import test_gpu_shade as T

    inp, grad_out = T.inputs(name)
    images = tuple(k for k in ("normal_img", "pos_img", "albedo", "background") if inp[k] is not None and inp[k].ndim == 4)
    got = T.run_hip(inp, grad_out, dtype, "capi", need=images)
    assert set(got) == {"out"} | {"grad_" + k for k in images}, sorted(got)
    keep = lambda r: None if r is None else {k: v for k, v in r.items() if k in got}  # noqa: E731
    T.check(got, keep(T.oracle(name, th.float64)), keep(T.oracle(name, th.float32)) if dtype == th.float32 else None, dtype, name)


def cases():
    """[(name, function, arguments)], in the order they run"""
    import shade_oracle as O

    out = []
    for name in O.CASES:
        for dtype in (th.float32, th.float64):
            out.append((f"oracle/{name}/{TAG[dtype]}", oracle_case, (name, dtype)))
    for name in ("plane1", "rows_S+1_f32", "n3_c4", "opt_i1s1b0g1"):
        for dtype in (th.float32, th.float64):
            out.append((f"images_only/{name}/{TAG[dtype]}", images_only_case, (name, dtype)))
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
