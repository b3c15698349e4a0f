"""The C-ABI entry points of forward kinematics -- drtk_amd_kinematics_forward and drtk_amd_kinematics_backward (with its
workspace) -- through the ctypes binding with every output and workspace between sentinel elements (DRTK_CAPI_GUARD,
drtk_amd/capi.py `_out`), on the structural cases of tests/kinematics_oracle.py: no levels, chains, a level wider than a
wave, a forest, real rigs, both sides of the Taylor switch, matrices, every rest-pose layout, strided poses, a tree at
the cap.  Each case is compared with the oracle under the bounds of tests/test_gpu_kinematics.py (the guard also leaves
every output merely element-aligned), all gradients at once and each on its own, and after each `capi.check_guards()`.
Not collected by pytest; tests/test_gpu_kinematics.py starts it in a child process:

    DRTK_CAPI_GUARD=1 DRTK_CAPI_POISON=1 python tests/guarded_kinematics.py [--only NAME]
    python tests/guarded_kinematics.py --list                (no GPU needed)"""
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


def all_gradients_case(name, dtype):
    import test_gpu_kinematics as T

    T.check_key(name, dtype, "capi")


def single_gradient_case(name, dtype):
    """Each gradient requested on its own gives the bits it has when all are requested"""
    import kinematics_oracle as O
    import test_gpu_kinematics as T

    case = O.case(name)
    full = T.capi_results(case, dtype)
    for grads, key in ((("rotations",), "grad_rot"), (("joints",), "grad_joints"), (("translation",), "grad_tr")):
        one = T.capi_results(case, dtype, grads)
        assert th.equal(one[key], full[key]), (name, key)
        assert th.equal(one["transforms"], full["transforms"]) and th.equal(one["posed"], full["posed"]), name


def cases():
    """[(name, function, arguments)], in the order they run"""
    import kinematics_oracle as O

    out = []
    for name in O.CASES:
        if name == "past_cap":  # refused by the entry points: tests/test_gpu_kinematics.py
            continue
        for dtype in (th.float32, th.float64):
            out.append((f"all_gradients/{name}/{TAG[dtype]}", all_gradients_case, (name, dtype)))
    for name in ("wide130", "matrices", "at_cap"):
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
