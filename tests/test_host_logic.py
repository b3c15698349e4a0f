"""CPU: drop-in boundary checks that need no GPU -- the C ABI library loads and exports every
symbol declared in include/drtk_amd.h, the torch operators are registered under the reference's
names with the reference's schemas, the Python API mirrors drtk.*, and the product never imports
the oracle."""
import ctypes
import inspect
import os
import sys
import re

import pytest
import torch as th
from conftest import ROOT


def test_c_abi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "drtk_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(drtk_amd_\w+)\s*\(", hdr)))
    assert len(declared) >= 10
    from drtk_amd import capi

    lib = ctypes.CDLL(os.path.join(ROOT, "drtk_amd", "libdrtk_amd.so"))
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/drtk_amd.h but not exported"
    assert sorted(capi.EXPORTS) == declared
    # ... and nothing else: in particular no ablation switch (those live only in profiles/libdrtk_amd_ablate.so,
    # built with -DDRTK_AMD_ABLATION for profiles/kernel_bench.py --flags)
    import subprocess

    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "drtk_amd", "libdrtk_amd.so")], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (drtk_amd_\w+)", syms)))
    assert exported == declared, set(exported) ^ set(declared)
    # NO other defined dynamic symbol of any kind (C++ internals, toolchain ids): -fvisibility=hidden + csrc/exports.map
    others = [l for l in syms.splitlines() if l.strip() and not re.search(r" T drtk_amd_\w+$", l)]
    assert not others, others
    assert "debug" not in syms
    csrc = os.path.join(ROOT, "drtk_amd", "csrc")
    for path in [os.path.join(d, f) for d, _, files in os.walk(csrc) for f in files]:
        f = os.path.relpath(path, csrc)
        src = open(path).read()
        assert not re.search(r"\bdbg\s*&|debug_flags\(\)\s*(&|>>)", src.replace("debug_flags() >> 10", "")) , f"{f}: phase switch outside DRTK_DBG()"
    assert b"gfx950" in capi.lib().drtk_amd_version()
    assert capi.lib().drtk_amd_status_string(0) == b"ok"


def test_c_abi_argument_validation_without_gpu():
    from drtk_amd import capi

    L = capi.lib()
    out = ctypes.c_size_t(0)
    assert L.drtk_amd_rasterize_workspace_bytes(ctypes.c_int64(8), ctypes.c_int64(100352), ctypes.c_int64(2048),
                                                ctypes.c_int64(2048), ctypes.byref(out)) == 0
    assert 0 < out.value < 64 * 2**20
    assert L.drtk_amd_rasterize_workspace_bytes(ctypes.c_int64(1), ctypes.c_int64(1), ctypes.c_int64(0),
                                                ctypes.c_int64(4), ctypes.byref(out)) == -1
    z = ctypes.c_void_p(0)
    # wireframe mode needs its own (packed image) workspace
    rc = L.drtk_amd_rasterize(ctypes.c_int(0), z, z, ctypes.c_int64(1), ctypes.c_int64(0), ctypes.c_int64(0),
                              ctypes.c_int64(0), ctypes.c_int64(4), ctypes.c_int64(4), ctypes.c_int(1), ctypes.c_void_p(16),
                              ctypes.c_void_p(16), z, ctypes.c_size_t(0), z)
    assert rc == -2  # DRTK_ERR_WORKSPACE_TOO_SMALL
    assert L.drtk_amd_rasterize_lines_workspace_bytes(ctypes.c_int64(2), ctypes.c_int64(8), ctypes.c_int64(8), ctypes.byref(out)) == 0
    assert out.value == 2 * 8 * 8 * 8
    # interpolate backward's OPTIONAL scratch buffer: rows padded to 64 bytes for float attributes of 11 ... 15 channels, nothing else
    i64 = ctypes.c_int64
    for dtype, C, want in ((0, 13, 8 * 1000 * 16 * 4), (0, 11, 8 * 1000 * 16 * 4), (0, 12, 8 * 1000 * 16 * 4), (0, 15, 8 * 1000 * 16 * 4), (0, 16, 0), (0, 10, 0),
                           (0, 3, 0), (0, 17, 0), (0, 20, 0), (0, 0, 0), (1, 13, 0), (1, 12, 0)):
        assert L.drtk_amd_interpolate_backward_workspace_bytes(ctypes.c_int(dtype), i64(8), i64(1000), i64(C), ctypes.byref(out)) == 0
        assert out.value == want, (dtype, C, out.value, want)
    assert L.drtk_amd_interpolate_backward_workspace_bytes(ctypes.c_int(0), i64(0), i64(1000), i64(13), ctypes.byref(out)) == 0 and out.value == 0
    assert L.drtk_amd_interpolate_backward_workspace_bytes(ctypes.c_int(0), i64(-1), i64(1000), i64(13), ctypes.byref(out)) == -1
    assert L.drtk_amd_interpolate_backward_workspace_bytes(ctypes.c_int(7), i64(1), i64(1), i64(13), ctypes.byref(out)) == -1
    # ... which must be 64-byte aligned when given (whole segments), and may always be absent
    a16 = ctypes.c_void_p(16)
    def ibw(ws, nbytes):
        return L.drtk_amd_interpolate_backward_ws(ctypes.c_int(0), a16, a16, a16, a16, a16, i64(1), i64(0), i64(13), i64(1), i64(0), i64(0), i64(4),
                                                  ctypes.c_void_p(64), ctypes.c_void_p(64), ctypes.c_void_p(ws), ctypes.c_size_t(nbytes), z)
    assert ibw(4096 + 16, 1 << 20) == -1          # misaligned workspace
    assert ibw(0, 0) == 0 and ibw(4096, 1 << 20) == 0  # V = 0, H = 0: nothing to fill or launch, both spellings accepted
    rc = L.drtk_amd_rasterize(ctypes.c_int(0), z, z, ctypes.c_int64(1), ctypes.c_int64(1 << 28), ctypes.c_int64(0),
                              ctypes.c_int64(0), ctypes.c_int64(4), ctypes.c_int64(4), ctypes.c_int(0), z, z, z,
                              ctypes.c_size_t(0), z)
    assert rc == -5  # V >= 2^28 (rasterize_kernel.cu:459-462)
    # workspaces hold 64-bit counters updated atomically: they must be 16-byte aligned (include/drtk_amd.h), which is
    # checked BEFORE the size -- an aligned workspace that is too small is -2, a misaligned one of any size is -1
    big = ctypes.c_size_t(1 << 30)
    for wire in (0, 1):
        args = lambda ws, nbytes: (ctypes.c_int(0), z, z, ctypes.c_int64(1), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0),  # noqa: E731
                                   ctypes.c_int64(4), ctypes.c_int64(4), ctypes.c_int(wire), ctypes.c_void_p(16), ctypes.c_void_p(16),
                                   ctypes.c_void_p(ws), nbytes, z)
        assert L.drtk_amd_rasterize(*args(4096, ctypes.c_size_t(0))) == -2
        for off in (4, 8, 12):
            assert L.drtk_amd_rasterize(*args(4096 + off, big)) == -1
    for fn, extra in ((L.drtk_amd_edge_grad_backward, ()), (L.drtk_amd_edge_grad_backward_fused, ("bary",))):
        def call(ws, nbytes):
            a = [ctypes.c_int(0), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16)]
            a += [ctypes.c_void_p(16)] * len(extra) + [ctypes.c_void_p(16)]                                  # (bary_img,) grad_output
            a += [ctypes.c_int64(1), ctypes.c_int64(3), ctypes.c_int64(1), ctypes.c_int64(1), ctypes.c_int64(0), ctypes.c_int64(4),
                  ctypes.c_int64(4), ctypes.c_double(1e4), ctypes.c_void_p(16), ctypes.c_void_p(ws), nbytes, z]
            return fn(*a)
        assert call(4096, ctypes.c_size_t(0)) == -2
        assert call(4096 + 4, big) == -1


def test_depth_order_setting_is_one_library_level_switch_shared_by_every_route():
    """include/drtk_amd.h drtk_amd_set_depth_order / drtk_amd_get_depth_order: no GPU needed for the setting itself.  The C
    ABI handle, drtk_amd.set_depth_order and the library the torch-operator shim links are ONE library object per process;
    the initial value follows DRTK_AMD_DEPTH_ORDER; invalid values are rejected.  (Child processes: the setting is global.)"""
    import subprocess

    code = f"""
import ctypes, os, sys
sys.path.insert(0, {ROOT!r})
import drtk_amd
from drtk_amd import capi
L = ctypes.CDLL(os.path.join({ROOT!r}, "drtk_amd", "libdrtk_amd.so"))
first = drtk_amd.get_depth_order()
assert capi.depth_order() == first and L.drtk_amd_get_depth_order() == {{"strict": 0, "fastmath": 1}}[first]
assert L.drtk_amd_set_depth_order(2) == -1 and L.drtk_amd_set_depth_order(-1) == -1 and drtk_amd.get_depth_order() == first
other = "strict" if first == "fastmath" else "fastmath"
drtk_amd.set_depth_order(other)
assert capi.depth_order() == other and L.drtk_amd_get_depth_order() == {{"strict": 0, "fastmath": 1}}[other]
capi.use_depth_order(first)
assert drtk_amd.get_depth_order() == first
try:
    drtk_amd.set_depth_order("fast")
    raise SystemExit("accepted an unknown order")
except ValueError:
    pass
# the operator shim resolves its C-ABI calls in the same library object (one mapping of libdrtk_amd.so in the process)
maps = [l.split()[-1] for l in open("/proc/self/maps") if "libdrtk_amd" in l]
assert len(set(maps)) == 1, set(maps)
print("FIRST", first)
"""
    for env_value, want in ((None, "strict"), ("fastmath", "fastmath"), ("strict", "strict"), ("nonsense", "strict")):
        env = dict(os.environ)
        env.pop("DRTK_AMD_DEPTH_ORDER", None)
        if env_value is not None:
            env["DRTK_AMD_DEPTH_ORDER"] = env_value
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split()[-2:] == ["FIRST", want], (env_value, r.stdout)
    assert not os.path.exists(os.path.join(ROOT, "drtk_amd", "libdrtk_amd_depth_fastmath.so")), "the second library of rounds 4-5 is gone: one library, one setting"


def test_torch_operator_schemas_match_reference():
    import drtk_amd  # noqa: F401  (loads the library)

    want = {
        "rasterize_ext::rasterize": "rasterize_ext::rasterize(Tensor v, Tensor vi, int height, int width, bool wireframe) -> Tensor[]",
        "render_ext::render": "render_ext::render(Tensor v, Tensor vi, Tensor index_img) -> Tensor[]",
        "interpolate_ext::interpolate": "interpolate_ext::interpolate(Tensor vert_attributes, Tensor vi, Tensor index_img, Tensor bary_img) -> Tensor",
        "interpolate_ext::interpolation_matrix": "interpolate_ext::interpolation_matrix(Tensor vi, Tensor index_img, Tensor bary_img) -> (Tensor, Tensor, Tensor, Tensor)",
        "interpolate_ext::interpolation_normal_matrix": "interpolate_ext::interpolation_normal_matrix(Tensor vi, Tensor index_img, Tensor bary_img, int num_vertices) -> (Tensor, Tensor, Tensor)",
        "interpolate_ext::interpolation_normal_matrix_values": "interpolate_ext::interpolation_normal_matrix_values(Tensor pair_indices, Tensor index_img, Tensor bary_img, int nnz) -> Tensor",
        "mipmap_grid_sampler_ext::mipmap_grid_sampler_2d": "mipmap_grid_sampler_ext::mipmap_grid_sampler_2d(Tensor[] x, Tensor grid, Tensor vt_dxdy_img, int max_aniso, int padding_mode, int interpolation_mode, bool align_corners, bool force_max_ansio, bool clip_grad) -> Tensor",
        "edge_grad_ext::edge_grad_estimator": "edge_grad_ext::edge_grad_estimator(Tensor v_pix, Tensor v_pix_img, Tensor vi, Tensor img, Tensor index_img, float max_dp_dr=10000.) -> Tensor",
    }
    for name, schema in want.items():
        ns, op = name.split("::")
        got = str(getattr(getattr(th.ops, ns), op).default._schema)
        assert got.replace(" ", "") == schema.replace(" ", ""), got
        for key in ("CUDA", "CPU", "Autograd", "AutocastCUDA"):
            assert th._C._dispatch_has_kernel_for_dispatch_key(name, key), (name, key)


def test_python_api_mirrors_drtk_signatures():
    import drtk_amd

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert params(drtk_amd.rasterize) == [("v", E), ("vi", E), ("height", E), ("width", E), ("wireframe", False)]
    assert params(drtk_amd.rasterize_with_depth) == params(drtk_amd.rasterize)
    assert params(drtk_amd.render) == [("v", E), ("vi", E), ("index_img", E)]
    assert params(drtk_amd.interpolate) == [("vert_attributes", E), ("vi", E), ("index_img", E), ("bary_img", E)]
    assert params(drtk_amd.edge_grad_estimator) == [
        ("v_pix", E), ("vi", E), ("bary_img", E), ("img", E), ("index_img", E), ("v_pix_img_hook", None),
        ("max_dp_dr", 1e4)]
    assert params(drtk_amd.mipmap_grid_sample) == [
        ("input", E), ("grid", E), ("vt_dxdy_img", E), ("max_aniso", E), ("mode", "bilinear"), ("padding_mode", "zeros"),
        ("align_corners", None), ("force_max_aniso", False), ("clip_grad", False)]  # drtk/mipmap_grid_sample.py:17-27
    sparse = [("vi", E), ("index_img", E), ("bary_img", E), ("num_vertices", E)]  # drtk/interpolate.py:53-58,127-132
    assert params(drtk_amd.interpolation_matrix) == sparse and params(drtk_amd.interpolation_normal_matrix) == sparse
    assert drtk_amd.__version__ == "0.1.0"


def test_cpu_tensors_fail_loudly_no_fallback():
    import drtk_amd

    v = th.zeros(1, 3, 3)
    vi = th.zeros(1, 3, dtype=th.int32)
    with pytest.raises(RuntimeError, match="HIP"):
        drtk_amd.rasterize(v, vi, 4, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        drtk_amd.render(v, vi, th.zeros(1, 4, 4, dtype=th.int32))
    with pytest.raises(RuntimeError, match="HIP"):
        drtk_amd.interpolate(v, vi, th.zeros(1, 4, 4, dtype=th.int32), th.zeros(1, 3, 4, 4))


def test_missing_native_libraries_fail_loudly(tmp_path):
    """No binaries -> ImportError that says what to do, at `import drtk_amd` and from the ctypes binding.  Never a
    silent eager / CPU substitute.  Run in a subprocess on a copy of the package's Python files WITHOUT its .so files,
    so neither the real binaries nor this process's already-loaded operators are involved.

    The advice in that error has to be runnable in exactly that state: the command it names is executed here (with
    --dry-run, nothing is compiled).  It is the build FILE; `python -m drtk_amd.build` cannot bootstrap, because -m
    imports the package first -- build.py therefore imports nothing from the package."""
    import ast
    import shutil
    import subprocess
    import sys

    src = os.path.join(ROOT, "drtk_amd")
    dst = tmp_path / "drtk_amd"
    for dirpath, dirnames, files in os.walk(src):
        dirnames[:] = [d for d in dirnames if d not in ("__pycache__", "csrc")]
        rel = os.path.relpath(dirpath, src)
        (dst / rel).mkdir(parents=True, exist_ok=True)
        for f in files:
            if f.endswith(".py"):
                shutil.copy(os.path.join(dirpath, f), dst / rel / f)
    assert not list(dst.rglob("*.so"))

    def run(code):
        return subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {str(tmp_path)!r}); " + code],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=str(tmp_path))

    r = run("import drtk_amd")
    assert r.returncode != 0 and "ImportError" in r.stderr, r.stderr[-2000:]
    assert "native libraries are not built" in r.stderr
    assert "libdrtk_amd.so" in r.stderr and "drtk_amd_torch_ops.so" in r.stderr  # names what is missing
    # ... and no submodule can be reached around that check (a submodule import runs the package's __init__ first)
    for mod in ("drtk_amd.capi", "drtk_amd.rasterize", "drtk_amd.render", "drtk_amd.mipmap_grid_sample", "drtk_amd.build"):
        r2 = run(f"import {mod}")
        assert r2.returncode != 0 and "native libraries are not built" in r2.stderr, (mod, r2.stderr[-1500:])

    # the command the error names: extract it, check it is the build file of THIS copy, and run it
    m = re.search(r"Run `python ([^`]+)`", r.stderr)
    assert m, r.stderr[-1500:]
    build_py = m.group(1)
    assert os.path.samefile(build_py, dst / "build.py"), build_py
    d = subprocess.run([sys.executable, build_py, "--dry-run"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300, cwd="/")  # from an unrelated directory
    assert d.returncode == 0, d.stderr[-2000:]
    lines = [ln for ln in d.stdout.splitlines() if ln.startswith("[drtk_amd]")]
    assert len(lines) == 2 and all(ln.endswith(": missing") for ln in lines), d.stdout
    assert "libdrtk_amd.so" in lines[0] and "drtk_amd_torch_ops.so" in lines[1]
    # `-m` is NOT that command: it ends in the same ImportError (known, and the reason the docs name the file)
    mrun = subprocess.run([sys.executable, "-m", "drtk_amd.build", "--dry-run"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300, cwd=str(tmp_path))
    assert mrun.returncode != 0 and "native libraries are not built" in mrun.stderr
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "python drtk_amd/build.py" in text and "python -m drtk_amd.build" not in text, doc

    # build.py stands alone: standard library at module level, torch only inside the function that needs its paths
    tree = ast.parse(open(os.path.join(src, "build.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else (
            [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
        assert not any(n.split(".")[0] == "drtk_amd" for n in names), "drtk_amd/build.py must not import the package"
        assert not (isinstance(node, ast.ImportFrom) and node.level > 0), "no relative imports in drtk_amd/build.py"

    # and the ctypes binding's own check gives the same advice
    capi_src = open(os.path.join(src, "capi.py")).read()
    assert "build.py" in capi_src and "-m drtk_amd.build" not in capi_src


def test_product_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "drtk_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                for pat in (r"import\s+oracle", r"from\s+oracle", r"drtk_oracle", r"[\"'/]oracle[\"'/]", r"ref_build", r"_ref/"):
                    assert not re.search(pat, src), f"{f} reaches into the oracle ({pat})"


def test_library_fills_with_a_kernel_not_with_hipMemset():
    """Zero-initialised counters and gradients are filled by fill_bytes_async (a kernel launch), never by
    hipMemset*: a captured memset node stops zeroing on graph replays that follow other device work (MI355X,
    ROCm 7.2), which turns rasterize into an out-of-bounds scatter and every backward op into silent
    accumulation.  The behaviour itself is pinned on the GPU by
    tests/test_gpu_parity.py::test_graph_capture_and_replay_with_other_work_between_replays."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "drtk_amd", "csrc")):
        for f in files:
            if not f.endswith((".hip", ".hpp", ".cpp", ".h")):
                continue
            for no, line in enumerate(open(os.path.join(dirpath, f), errors="ignore"), 1):
                if "hipMemset" in line.split("//")[0]:
                    bad.append(f"{f}:{no}: {line.strip()}")
    assert not bad, "\n".join(bad)


def test_kernels_use_correctly_rounded_roots_and_quotients():
    """Discrete decisions of the reference hang on the last bit of normalised vectors (edge_grad's get_dp_dr sign,
    the mip level's floor), so square roots and divisions that feed them are the IEEE ones.  `__fsqrt_rn` LOOKS like
    one, but without OCML_BASIC_ROUNDED_OPERATIONS __clang_hip_math.h defines it as __ocml_native_sqrt_f32 (bare
    v_sqrt_f32, 1 ulp); the native / approximate families are equally out.  `__builtin_amdgcn_rcpf` is allowed in
    render.hip only, where the backward's quotients are documented as 1-2 ulp on purpose (no decision depends on
    them), and in rasterize.hip as the SEED of exact_rcp: one Markstein correction makes it the correctly rounded
    reciprocal, which drtk_amd_selftest_exact_div checks exhaustively over all 2^23 significands on the device (GPU
    suite).  Behaviour pinned on the GPU by test_edge_grad_sign_decisions_at_near_parallel_normals_follow_the_reference."""
    banned = re.compile(r"__fsqrt_r[nduz]|__frsqrt_rn|__ocml_native_|__builtin_amdgcn_(sqrt|rsq|rcp)|\b(rsqrtf?|__f(div|sqrt)def|"
                        r"__fdividef|__expf|__logf|__log2f|__powf|__sinf|__cosf)\b")
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "drtk_amd", "csrc")):
        for f in files:
            if not f.endswith((".hip", ".hpp", ".cpp", ".h")):
                continue
            for no, line in enumerate(open(os.path.join(dirpath, f), errors="ignore"), 1):
                code = line.split("//")[0]
                m = banned.search(code)
                if m and not (f in ("render.hip", "rasterize.hip") and m.group(0).startswith("__builtin_amdgcn_rcp")):
                    bad.append(f"{f}:{no}: {line.strip()}")
    assert not bad, "\n".join(bad)
    build_py = open(os.path.join(ROOT, "drtk_amd", "build.py")).read()
    assert "-fno-fast-math" in build_py and "-ffp-contract=off" in build_py
    assert "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in build_py and "-ffast-math" not in build_py


def test_no_cross_lane_operation_sits_behind_a_short_circuit():
    """`(lane & 15) == 0 || tr != __shfl_up(x, 1)` evaluates the shuffle only on the lanes whose first operand is false:
    the others are switched off for the ds_bpermute, and a lane that reads from one of them gets 0 instead of that lane's
    value (found while bringing up the four-pixel-lane render backward, profiles/NOTES.md R6.7: one pixel pattern in one
    fixture).  The same holds for `&&` and `?:`.  Cross-lane values are computed into a variable first, by every lane."""
    # operations that MOVE a value between lanes (a ballot behind a wave-uniform condition is harmless: switched-off lanes
    # contribute the 0 they should)
    cross = re.compile(r"(__shfl\w*|__builtin_amdgcn_(update_dpp|mov_dpp|ds_bpermute|ds_permute|readlane)|dpp_row_sh[lr]\w*|dpp_i32|"
                       r"wave_(min|max)_i32)\s*[<(]")

    def guarded(code, pos):
        """Is there a `||`, `&&` or `?` to the left of code[pos] in the same statement that decides whether it is evaluated?
        (operators inside parenthesised groups that are already closed -- other calls' arguments -- do not)"""
        depth = 0
        i = pos - 1
        while i >= 0:
            ch = code[i]
            if ch == ")":
                depth += 1
            elif ch == "(":
                depth = max(depth - 1, 0) if depth else 0
            elif depth == 0:
                if ch in ";{}" or ch == ",":
                    return False
                if ch == "?" or code[i - 1:i + 1] in ("||", "&&"):
                    return True
            i -= 1
        return False

    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "drtk_amd", "csrc")):
        for f in files:
            if not f.endswith((".hip", ".hpp")):
                continue
            for no, line in enumerate(open(os.path.join(dirpath, f), errors="ignore"), 1):
                code = line.split("//")[0]
                if any(guarded(code, m.start()) for m in cross.finditer(code)):
                    bad.append(f"{f}:{no}: {line.strip()}")
    assert not bad, "\n".join(bad)
    # the check checks: the line that had the bug, a select, and two harmless neighbours
    for text, call, want in (("const bool b0 = (lane & 15) == 0 || tr[0] != __shfl_up(tr[3], 1);", "__shfl_up", True),
                             ("x = on ? dpp_row_shr<1>(v) : 0;", "dpp_row_shr", True),
                             ("x0 = wave_min_i32(on ? x : M), y0 = wave_min_i32(on ? y : M);", "y0 = wave_min_i32", False),
                             ("const int32_t left = __shfl_up(tr[3], 1); const bool b0 = first || tr[0] != left;", "__shfl_up", False)):
        assert guarded(text, text.index(call) + (len("y0 = ") if call.startswith("y0") else 0)) == want, text


def test_only_the_cpu_baseline_leg_and_the_smoke_check_use_the_oracle():
    """Outside tests/ and oracle/ itself: bench.py may reach into oracle/ only inside cpu_baseline() (the reported
    baseline, never the thing measured), __graft_entry__.py only to build the checker and in smoke(); the profiling
    scripts not at all."""
    import ast

    pat = re.compile(r"import\s+oracle|from\s+oracle|[\"']oracle[\"']|drtk_oracle|ref_build|_ref/")

    def offending(path, allowed_functions):
        src = open(path).read()
        tree = ast.parse(src)
        spans = [(n.lineno, n.end_lineno) for n in ast.walk(tree)
                 if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name in allowed_functions]
        doc_lines = set()
        for n in ast.walk(tree):  # prose in docstrings / help strings is not a use
            if isinstance(n, ast.Constant) and isinstance(n.value, str) and ("\n" in n.value or " " in n.value):
                doc_lines.update(range(n.lineno, n.end_lineno + 1))
        bad = []
        for no, line in enumerate(src.splitlines(), 1):
            if pat.search(line.split("#")[0]) and no not in doc_lines and not any(a <= no <= b for a, b in spans):
                bad.append(f"{os.path.basename(path)}:{no}: {line.strip()}")
        return bad

    # the leg (one function per workload) and its loader
    assert offending(os.path.join(ROOT, "bench.py"), {"cpu_baseline", "cpu_baseline_textured", "_cpu_backend"}) == []
    bench_src = open(os.path.join(ROOT, "bench.py")).read()
    assert len(re.findall(r"_cpu_backend\(", bench_src)) == 2  # its definition + the one call in cpu_baseline()
    assert len(re.findall(r"\bcpu_baseline\(", bench_src)) == 2   # its definition + the one call, rank 0 at N = 1
    assert len(re.findall(r"\bcpu_baseline_textured\(", bench_src)) == 2
    assert offending(os.path.join(ROOT, "__graft_entry__.py"), {"build", "smoke"}) == []
    for dirpath, dirnames, files in os.walk(os.path.join(ROOT, "profiles")):
        dirnames[:] = [d for d in dirnames if d != "__pycache__"]
        for f in files:
            if f.endswith((".py", ".sh")):
                src = open(os.path.join(dirpath, f)).read()
                assert not pat.search(src), f"profiles/{f} reaches into the oracle"


def _kernel_stats(path):
    """profiles/rNN/bench_step_kernel_stats.txt -> [(short kernel name, calls, avg_us)] of this repo's kernels."""
    out = []
    for line in open(path):
        parts = line.split(None, 4)
        if len(parts) == 5 and parts[0].isdigit() and "drtk_amd::" in parts[4]:
            name = parts[4].split("drtk_amd::(anonymous namespace)::")[-1].split("(")[0].split("<")[0]
            out.append((name, int(parts[0]), float(parts[2])))
    return out


def test_committed_profile_artefacts_describe_one_collection():
    """profiles/rNN/: the bench line, the PMC traffic summary and the rocprofv3 kernel summary of a round come from
    ONE run of profiles/scripts/collect_round.sh (counter passes first, then the bench that reads them).
    From round 2 on `roofline` prices ONE HIP kernel: it must be the kernel of this repo with the largest rocprofv3
    average in the same collection's summary, its `traffic` must be that kernel's entry of traffic.json, the
    profiler's average must agree with the HIP-event `ms_per_launch` within 5 %, and `frac` / `frac_traffic` must
    follow from the stated bytes and time.  (Round 1's line priced an op of two kernels: checked by its own rules.)"""
    import glob
    import json

    rounds = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*")))
    checked = 0
    for rdir in rounds:
        if not os.path.exists(os.path.join(rdir, "bench_n1.json")):
            continue  # a round directory opened before its first collection; once the bench line is there, all three are
        checked += 1
        bench = json.loads(open(os.path.join(rdir, "bench_n1.json")).read().strip().splitlines()[-1])
        roof = bench["roofline"]
        traffic = json.load(open(os.path.join(rdir, "traffic.json")))["kernels"]
        stats = _kernel_stats(os.path.join(rdir, "bench_step_kernel_stats.txt"))
        assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
        assert abs(roof["achieved"] - roof["algorithmic_bytes"] / (roof["ms_per_launch"] * 1e-3) / 1e9) < 1.0
        if "hip_kernels" in roof:  # round 1: the slowest OP (edge_dots + edge_scatter_pairs)
            names = roof["hip_kernels"]
            total = sum(rec["hbm_bytes"] for name, rec in traffic.items() if any(pat in name for pat in names))
            assert int(total) == roof["traffic"], f"{rdir}: bench_n1.json and traffic.json are from different collections"
            avg_us = {pat: sum(a for n, c, a in stats if n == pat.split("<")[0]) for pat in names}
            assert all(avg_us.values()), f"{rdir}: rocprofv3 summary lacks some of {names}"
            assert abs(sum(avg_us.values()) / 1e3 - roof["ms_per_launch"]) <= 0.05 * roof["ms_per_launch"]
            continue
        k = roof["kernel"]
        # the priced kernel is the largest single kernel of the step (kernels run many times per step -- those of the
        # bench workload, not the handful of launches of the CPU-baseline / set-up phase)
        step_kernels = [(n, a) for n, c, a in stats if c >= bench["steps"]]
        top = max(step_kernels, key=lambda t: t[1])
        priced = [a for n, a in step_kernels if n == k]
        # (round 4: interpolate backward and edge_dots are within 1 % of each other -- 579.8 and 583.7 us under rocprofv3,
        # 594 and 579 under the bench's own events -- so "the largest" may be either side of a tie)
        assert priced and priced[0] >= 0.97 * top[1], f"{rdir}: roofline prices {k} but the largest kernel of the step is {top}"
        assert abs(priced[0] / 1e3 - roof["ms_per_launch"]) <= 0.05 * roof["ms_per_launch"], (priced, roof["ms_per_launch"])
        mine = [rec["hbm_bytes"] for name, rec in traffic.items() if name.split("<")[0] == k]
        assert mine and int(mine[0]) == roof["traffic"], f"{rdir}: bench_n1.json and traffic.json are from different collections"
        assert abs(roof["frac_traffic"] - roof["traffic"] / (roof["ms_per_launch"] * 1e-3) / 1e9 / roof["peak"]) < 1e-3
        # traffic within sight of the algorithmic bytes: below = lines served by L2 / MALL, above = re-reads or atomics
        assert 0.5 * roof["algorithmic_bytes"] < roof["traffic"] < 1.5 * roof["algorithmic_bytes"]
        path = bench["path_roofline"]
        assert abs(path["t_ops_ms"] - sum(r["ms_per_step"] for r in path["kernels"].values() if r["op"] != "outside the four ops")) < 1e-2
        assert k in path["kernels"] and path["kernels"][k]["ms_per_launch"] == roof["ms_per_launch"]
    assert checked >= 1, "no profiles/rNN directory holds a collection"


def test_synthetic_mesh_sizes():
    from drtk_amd import synthetic as S

    for name, f in (("10k", 10080), ("100k", 100352), ("250k", 250632), ("1M", 1002528)):
        nl, no = S.MESH_SIZES[name]
        assert 2 * nl * no == f
    v, vi = S.uv_sphere(6, 8)
    assert v.shape == (56, 3) and vi.shape == (96, 3) and vi.dtype == th.int32
    vp, _ = S.sphere_views(3, 6, 8, 32, 32)
    assert vp.shape == (3, 56, 3) and (vp[..., 2] > 1.9).all() and (vp[..., 2] < 4.1).all()


def test_normal_matrix_pattern_builder_and_cache():
    """The topology-only half of interpolation_normal_matrix (interpolate_module.cpp:28-262) runs on
    whatever device vi lives on, so its logic is checked here on CPU tensors: pattern == the
    oracle's restatement, stride-0 batches analysed once, identity+version keyed LRU of 128."""
    import drtk_amd  # noqa: F401
    import oracle as O
    from conftest import load_sparse

    ops = th.ops.drtk_amd_ext
    vi, _, _, V, _, go = load_sparse("ragged_f32")
    ops.normal_matrix_cache_clear()
    crow, col, pair = ops.normal_matrix_structure(vi, V)
    assert crow.dtype == th.int64 and col.dtype == th.int64 and pair.dtype == th.int32
    assert th.equal(crow.int(), go["nm_crow"]) and th.equal(col.int(), go["nm_col"]) and th.equal(pair, go["nm_pair"])
    assert ops.normal_matrix_cache_stats() == [0, 1, 1]
    ops.normal_matrix_structure(vi, V)
    assert ops.normal_matrix_cache_stats() == [1, 1, 1]  # hit: same tensor, same version
    ops.normal_matrix_structure(vi.clone(), V)
    assert ops.normal_matrix_cache_stats() == [1, 2, 2]  # another tensor with equal content misses
    vi.add_(0)  # in-place edit bumps the version counter
    ops.normal_matrix_structure(vi, V)
    assert ops.normal_matrix_cache_stats() == [1, 3, 3]
    ops.normal_matrix_structure(vi, V + 5)  # num_vertices is part of the key
    assert ops.normal_matrix_cache_stats() == [1, 4, 4]

    # shared topology: a stride-0 batch is analysed once and handed back as a stride-0 expand
    face = th.tensor([[0, 1, 2], [2, 1, 3]], dtype=th.int32)
    shared = face[None].expand(4, -1, -1)
    crow_s, col_s, pair_s = ops.normal_matrix_structure(shared, 4)
    assert pair_s.shape == (4, 2, 9) and pair_s.stride(0) == 0
    crow_o, col_o, pair_o = O.normal_matrix_structure(shared.contiguous(), 4)
    assert th.equal(crow_s, crow_o) and th.equal(col_s, col_o) and th.equal(pair_s.contiguous(), pair_o)

    # eviction: 128 entries
    ops.normal_matrix_cache_clear()
    keep = [th.tensor([[[0, 1, 2]]], dtype=th.int32) for _ in range(130)]
    for t in keep:
        ops.normal_matrix_structure(t, 3)
    assert ops.normal_matrix_cache_stats() == [0, 130, 128]
    ops.normal_matrix_structure(keep[0], 3)  # the oldest was evicted
    assert ops.normal_matrix_cache_stats()[1] == 131
    ops.normal_matrix_structure(keep[129], 3)
    assert ops.normal_matrix_cache_stats()[0] == 1
    ops.normal_matrix_cache_clear()

    # error behaviour (interpolate_module.cpp:132-137,150-153,181-183)
    with pytest.raises(RuntimeError, match="outside \\[0, num_vertices\\)"):
        ops.normal_matrix_structure(face[None], 3)
    with pytest.raises(RuntimeError, match="non-negative"):
        ops.normal_matrix_structure(face[None], -1)
    with pytest.raises(RuntimeError, match="positive when faces are present"):
        ops.normal_matrix_structure(face[None], 0)
    crow_e, col_e, pair_e = ops.normal_matrix_structure(th.empty(2, 0, 3, dtype=th.int32), 5)
    assert crow_e.tolist() == [0] * 6 and col_e.numel() == 0 and pair_e.shape == (2, 0, 9)


def test_sparse_ops_cpu_tensors_fail_loudly():
    import drtk_amd

    vi = th.tensor([[[0, 1, 2]]], dtype=th.int32)
    index = th.zeros(1, 4, 4, dtype=th.int32)
    bary = th.full((1, 3, 4, 4), 1 / 3)
    for fn in (lambda: drtk_amd.interpolation_matrix(vi, index, bary, 3),
               lambda: drtk_amd.interpolation_normal_matrix(vi, index, bary, 3),
               lambda: th.ops.interpolate_ext.interpolation_normal_matrix_values(th.zeros(1, 1, 9, dtype=th.int32), index, bary, 9)):
        with pytest.raises(RuntimeError, match="HIP\\) path only"):
            fn()


# ---- the `import drtk` drop-in (drtk/ at the repo root) ----------------------------------------------------------
def _run_py(code, cwd=None, extra_path=(), ld_path=None):
    import subprocess

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([*extra_path, ROOT]), PYTHONDONTWRITEBYTECODE="1")
    if ld_path:
        env["LD_LIBRARY_PATH"] = ld_path + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=cwd or ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_import_drtk_resolves_the_reference_export_list_on_the_path():
    """drtk/__init__.py:8-33 of the reference, restricted to SURVEY 8a/8f names: all resolve, are the drtk_amd
    objects, submodule spellings work, and what is out of scope says so."""
    out = _run_py("""
import drtk, drtk_amd, inspect
for n in ["edge_grad_estimator", "interpolate", "interpolation_matrix", "interpolation_normal_matrix", "mipmap_grid_sample",
          "rasterize", "rasterize_with_depth", "render", "transform", "transform_with_v_cam"]:
    assert getattr(drtk, n) is getattr(drtk_amd, n), n
assert drtk.__version__ == "0.1.0" and inspect.ismodule(drtk.utils)
from drtk import edge_grad_estimator, interpolate, rasterize, render          # test/two_triangles.py:11
from drtk.screen_space_uv_derivative import screen_space_uv_derivative
from drtk.mipmap_grid_sample import mipmap_grid_sample
from drtk.utils import load_torch_ops, project_points, DISTORTION_MODES
import drtk.transform, drtk.interpolate, drtk.render, drtk.edge_grad_estimator, drtk.rasterize
for ext in ["drtk.rasterize_ext", "drtk.render_ext", "drtk.interpolate_ext", "drtk.edge_grad_ext", "drtk.mipmap_grid_sampler_ext"]:
    load_torch_ops(ext)
try:
    load_torch_ops("drtk.msi_ext"); raise SystemExit("msi_ext must not load")
except ImportError: pass
for n in ["grid_scatter", "msi", "render_ref", "upsample"]:
    try:
        getattr(drtk, n); raise SystemExit(n)
    except AttributeError as e:
        assert "not provided" in str(e) and "out of scope" in str(e)
try:
    from drtk import msi
    raise SystemExit("msi import")
except ImportError: pass
print("ok")
""")
    assert out.strip().endswith("ok")


def test_extension_modules_load_the_way_the_reference_loader_loads_them():
    """drtk/utils/load_torch_ops.py:14-20 of the reference is `module = importlib.import_module(extension);
    th.ops.load_library(module.__file__)`: those two steps, on drtk/<name>_ext.so, register the operators."""
    out = _run_py("""
import importlib, torch as th
for ext, op in [("rasterize_ext", "rasterize"), ("render_ext", "render"), ("interpolate_ext", "interpolate"),
                ("edge_grad_ext", "edge_grad_estimator"), ("mipmap_grid_sampler_ext", "mipmap_grid_sampler_2d")]:
    module = importlib.import_module("drtk." + ext)
    assert module.__file__.endswith(ext + ".so"), module.__file__
    th.ops.load_library(module.__file__)
    assert th._C._dispatch_has_kernel_for_dispatch_key(ext + "::" + op, "CUDA")
print("ok")
""")
    assert out.strip().endswith("ok")
    import subprocess

    for ext in ("rasterize_ext", "render_ext", "interpolate_ext", "edge_grad_ext", "mipmap_grid_sampler_ext"):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "drtk", ext + ".so")], capture_output=True, text=True).stdout
        assert f" T PyInit_{ext}" in syms  # rasterize_module.cpp:73-75


def test_a_package_of_links_reaches_our_operators_the_way_the_reference_wrappers_call_them(tmp_path):
    """The *_ext surface as a DRTK-style package elsewhere sees it: a package directory holding nothing but LINKS to our
    drtk/<name>_ext.so and a loader that does what the reference's drtk/utils/load_torch_ops.py:14-20 does (import the
    module, th.ops.load_library its file) resolves every operator in our library, and the calls of the reference's
    wrappers (rasterize.py:64, render.py:38, interpolate.py:50, edge_grad_estimator.py:174) with CPU tensors arrive in
    our operator (the 'HIP path only' error of the CPU key)."""
    pkg = tmp_path / "drtk"
    pkg.mkdir()
    exts = ("rasterize_ext", "render_ext", "interpolate_ext", "edge_grad_ext", "mipmap_grid_sampler_ext")
    for ext in exts:
        os.symlink(os.path.join(ROOT, "drtk", ext + ".so"), pkg / (ext + ".so"))
    (pkg / "__init__.py").write_text("import importlib\nimport torch as th\n\nfor _ext in %r:\n"
                                     "    th.ops.load_library(importlib.import_module(__name__ + '.' + _ext).__file__)\n" % (exts,))
    out = _run_py("""
import os, sys, torch as th, drtk
here = os.path.dirname(drtk.__file__)
for ext, op in [("rasterize_ext", "rasterize"), ("render_ext", "render"), ("interpolate_ext", "interpolate"),
                ("edge_grad_ext", "edge_grad_estimator"), ("mipmap_grid_sampler_ext", "mipmap_grid_sampler_2d")]:
    assert os.path.dirname(sys.modules["drtk." + ext].__file__) == here, sys.modules["drtk." + ext].__file__
    assert th._C._dispatch_has_kernel_for_dispatch_key(ext + "::" + op, "CUDA"), op
v = th.zeros(1, 3, 3); vi = th.zeros(1, 3, dtype=th.int32); index = th.zeros(1, 8, 8, dtype=th.int32); img = th.zeros(1, 3, 8, 8)
for call in (lambda: th.ops.rasterize_ext.rasterize(v, vi, 8, 8, False), lambda: th.ops.render_ext.render(v, vi, index),
             lambda: th.ops.interpolate_ext.interpolate(v, vi, index, img),
             lambda: th.ops.edge_grad_ext.edge_grad_estimator(v, img, vi, img, index, 1e4)):
    try:
        call(); raise SystemExit("CPU call did not raise")
    except RuntimeError as e:
        assert "HIP" in str(e), str(e)
print(drtk.__file__); print("ok")
""", cwd=str(tmp_path), extra_path=[str(tmp_path)],
                  # the extension modules find drtk_amd_torch_ops.so through $ORIGIN/../drtk_amd, which a LINK in a
                  # temporary directory does not have next to it
                  ld_path=os.path.join(ROOT, "drtk_amd"))
    lines = out.strip().splitlines()
    assert lines[-1] == "ok" and lines[-2].startswith(str(tmp_path))


def test_sampler_inputs_that_are_read_in_place_and_those_that_are_copied():
    """Host logic of the sampler's strided inputs (capi._grid_layout / _level_table; csrc/torch_ops/mipmap.cpp's prep_grid /
    prep_levels decide the same way): which layouts go to the kernels as they are, with which strides, and which are
    made contiguous first."""
    from drtk_amd import capi

    N, H, W = 3, 5, 7
    P = H * W
    grid = th.rand(N, H, W, 2)
    g, lay = capi._grid_layout(grid)
    assert g is grid and list(lay) == [2 * P, 2, 1]
    uv_img = th.rand(N, 2, H, W)
    cf = uv_img.permute(0, 2, 3, 1)
    g, lay = capi._grid_layout(cf)
    assert g is cf and list(lay) == [2 * P, 1, P]                       # channel-first image read through its strides
    wide = th.rand(N, 6, H, W)[:, 2:4].permute(0, 2, 3, 1)
    g, lay = capi._grid_layout(wide)
    assert g is wide and list(lay) == [6 * P, 1, P]                     # two channels of a wider image
    one = th.rand(1, H, W, 2).expand(1, H, W, 2)
    assert list(capi._grid_layout(one)[1]) == [2 * P, 2, 1]
    for bad in (th.rand(N, H, 2 * W, 2)[:, :, :W],                      # rows with padding
                th.rand(1, H, W, 2).expand(N, H, W, 2),                 # one uv field for all views: overlapping
                th.rand(N, W, H, 2).permute(0, 2, 1, 3),                # transposed image
                th.rand(N, H, W, 4)[..., ::2]):                         # strided channels, pixels not evenly spaced the same way
        g, lay = capi._grid_layout(bad)
        assert g is not bad and g.is_contiguous() and list(lay) == [2 * P, 2, 1] and th.equal(g, bad)

    C, h, w = 3, 4, 6
    lv = th.rand(1, C, h, w)
    shared = lv.expand(N, C, h, w)
    kept, _, lh, lw, lsn = capi._level_table([shared, lv])
    assert kept[0] is shared and list(lsn) == [0, C * h * w] and list(lh) == [h, h] and list(lw) == [w, w]
    spaced = th.rand(2 * N, C, h, w)[::2]
    kept, _, _, _, lsn = capi._level_table([spaced])
    assert kept[0] is spaced and list(lsn) == [2 * C * h * w]
    for bad in (th.rand(N, 2 * C, h, w)[:, ::2],                        # views that are not contiguous blocks
                th.rand(N, C, w, h).transpose(2, 3)):
        kept, _, _, _, lsn = capi._level_table([bad])
        assert kept[0] is not bad and kept[0].is_contiguous() and list(lsn) == [C * h * w]


def test_bench_flags_a_stale_traffic_collection(tmp_path, monkeypatch):
    """roofline.traffic is replayed from the committed PMC collection (profiles/rNN/traffic.json); the collection records the
    SHA-256 of every kernel source (profiles/make_traffic.py) and bench.py reports `traffic_stale` when the file that
    defines the priced kernel, or a shared header, has changed since -- so a driver-run line cannot quote the traffic of a
    kernel that no longer exists.  Pure host logic: exercised here without a GPU."""
    import hashlib
    import importlib.util

    spec = importlib.util.spec_from_file_location("_bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    csrc = os.path.join(ROOT, "drtk_amd", "csrc")
    now = {f: hashlib.sha256(open(os.path.join(csrc, f), "rb").read()).hexdigest() for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))}
    bench.measured_traffic_table.sources = dict(now)
    assert bench.traffic_staleness("interpolate_backward_wide_kernel") == (False, [])
    bench.measured_traffic_table.sources = dict(now, **{"interpolate.hip": "0" * 64})
    assert bench.traffic_staleness("interpolate_backward_wide_kernel") == (True, ["interpolate.hip"])
    assert bench.traffic_staleness("render_kernel") == (False, [])  # another file's kernel is unaffected
    bench.measured_traffic_table.sources = dict(now, **{"common.hpp": "0" * 64})
    assert bench.traffic_staleness("render_kernel") == (True, ["common.hpp"])  # a shared header touches every kernel
    bench.measured_traffic_table.sources = None  # collections of rounds 1-4: provenance unknown
    assert bench.traffic_staleness("render_kernel")[0] is True
    # the committed collection itself parses, and make_traffic.py writes the record the check needs
    table, path = bench.measured_traffic_table()
    assert path is None or len(table) > 0
    assert '"sources": sources' in open(os.path.join(ROOT, "profiles", "make_traffic.py")).read()


def test_bench_dump_outputs_writes_float_arrays_and_samples_large_ones_the_same_way(tmp_path):
    """bench.py --dump-outputs (host logic, CPU tensors): small arrays keep their shape and values, integers become float64,
    half becomes float32, and an array above DUMP_SAMPLE elements becomes DUMP_SAMPLE elements taken at seeded positions
    -- the same positions in every call, so two runs (two builds) can be compared element for element."""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location("_bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    big = th.arange(3 * bench.DUMP_SAMPLE, dtype=th.float32).reshape(3, -1)
    arrays = dict(loss=th.tensor(1.5), index=th.tensor([[-1, 7], [2 ** 30, 3]], dtype=th.int32),
                  half=th.tensor([0.5, 2.0], dtype=th.float16), big=big)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    b = {f.stem: np.load(f) for f in (tmp_path / "b").glob("*.npy")}
    assert set(a) == set(arrays) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["loss"].dtype == np.float32 and a["loss"].shape == () and float(a["loss"]) == 1.5
    assert a["index"].dtype == np.float64 and a["index"].tolist() == [[-1, 7], [2 ** 30, 3]]
    assert a["half"].dtype == np.float32 and a["half"].tolist() == [0.5, 2.0]
    s = a["big"]
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(s) >= 0) and len(np.unique(s)) > bench.DUMP_SAMPLE // 2  # sorted positions, spread over the array
    assert s.min() < bench.DUMP_SAMPLE and s.max() >= 2 * bench.DUMP_SAMPLE
