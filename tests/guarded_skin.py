"""The C-ABI entry points of linear blend skinning -- drtk_amd_skin_forward and drtk_amd_skin_backward (with its workspace) --
through the ctypes binding with every output and workspace between sentinel elements (DRTK_CAPI_GUARD, drtk_amd/capi.py
`_out`), on the structural cases of tests/skin_oracle.py: one lane past a block, shared rest poses, eight slots with empty
ones, chunked joints, more joints than the forward stages in LDS, 4x4 transforms read in place.  Each case is compared with
the oracle under the bounds of tests/test_gpu_skin.py (the guard also leaves every output merely element-aligned), all
three gradients at once and each on its own, and after each `capi.check_guards()`.  Not collected by pytest;
tests/test_gpu_skin.py starts it in a child process:

    DRTK_CAPI_GUARD=1 DRTK_CAPI_POISON=1 python tests/guarded_skin.py [--only NAME]
    python tests/guarded_skin.py --list                (no GPU needed)"""
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
    import test_gpu_skin as T

    T.check_key(name, dtype, "capi")


def single_gradient_case(name, dtype):
    """Each gradient requested on its own gives the bits it has when all three are requested"""
    import skin_oracle as O
    import test_gpu_skin as T

    inputs = O.case(name)
    full = T.hip_results(inputs, dtype, "capi")
    for grads, key in ((("v",), "grad_v"), (("weights",), "grad_w"), (("transforms",), "grad_t")):
        one = T.hip_results(inputs, dtype, "capi", grads=grads)
        assert th.equal(one[key], full[key]), (name, key)
        assert th.equal(one["out"], full["out"]), name


def cases():
    """[(name, function, arguments)], in the order they run"""
    import skin_oracle as O

    out = []
    for name in O.CASES:
        for dtype in (th.float32, th.float64):
            out.append((f"all_gradients/{name}/{TAG[dtype]}", all_gradients_case, (name, dtype)))
    for name in ("k8_slots", "chunked", "mat4_view"):
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
