"""The C-ABI entry points of the closest-point queries -- drtk_amd_nearest_forward and drtk_amd_nearest_backward (with their
workspaces) -- through the ctypes binding with every output and workspace between sentinel elements (DRTK_CAPI_GUARD,
drtk_amd/capi.py `_out`), on the structural cases of tests/nearest_oracle.py: queries and targets one past a workgroup and
a tile, split targets with a short last range, shared point sets, runs across chunks, rejected candidates.  Each case is
compared with the oracle under the bounds of tests/test_gpu_nearest.py (the guard also leaves every output merely
element-aligned), both gradients at once and each on its own, and after each `capi.check_guards()`.  Not collected by
pytest; tests/test_gpu_nearest.py starts it in a child process:

    DRTK_CAPI_GUARD=1 DRTK_CAPI_POISON=1 python tests/guarded_nearest.py [--only NAME]
    python tests/guarded_nearest.py --list                (no GPU needed)"""
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


def both_gradients_case(name, dtype):
    import test_gpu_nearest as T

    T.check_key(name, dtype, "capi")


def single_gradient_case(name, dtype):
    """Each gradient requested on its own gives the bits it has when both are requested"""
    import nearest_oracle as O
    import test_gpu_nearest as T

    inputs = O.case(name)
    full = T.hip_results(inputs, dtype, "capi")
    for grads, key in ((("p",), "grad_p"), (("q",), "grad_q")):
        one = T.hip_results(inputs, dtype, "capi", grads=grads)
        assert th.equal(one[key], full[key]), (name, key)
        assert th.equal(one["dist2"], full["dist2"]) and th.equal(one["idx"], full["idx"]), name


def cases():
    """[(name, function, arguments)], in the order they run"""
    import nearest_oracle as O

    out = []
    for name in O.CASES:
        for dtype in (th.float32, th.float64):
            out.append((f"both_gradients/{name}/{TAG[dtype]}", both_gradients_case, (name, dtype)))
    for name in ("split_six", "shared_p", "shared_q_2d", "minus_one_front"):
        for dtype in (th.float32, th.float64):
            out.append((f"single_gradient/{name}/{TAG[dtype]}", single_gradient_case, (name, dtype)))
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
