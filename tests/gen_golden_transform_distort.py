"""Writes tests/golden/transform_distort_<case>.npz and transform_distort_estimators.npz from the REFERENCE's own
`project_points` / `estimate_*_fov` (drtk/utils/projection.py of a DRTK checkout, loaded by file path: it needs only numpy
and torch), on the CPU with one torch thread.  Build machine only -- no test imports this module.

    python tests/gen_golden_transform_distort.py [path/to/drtk/utils/projection.py]

Per case (tests/transform_distort_oracle.py: CASES), in float64 ("..._f64") and in the reference's own float32
("..._f32", inputs rounded to float32): v_pix, v_cam and the VJP with respect to v of the stored g_pix, g_cam; for the
float64 run also the VJPs with respect to campos, camrot, focal, princpt and D.  The inputs every case shares go to
transform_distort_inputs.npz."""
import importlib.util
import os
import sys

import numpy as np
import torch as th

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import transform_distort_oracle as O  # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("_reference_projection", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, name, inputs, dtype):
    mode, D, fov_given, lut_on = O.CASES[name]
    data = dict(inputs, D=D)
    v, cams, kw = O.case_kwargs(name, data, dtype)
    v.requires_grad_(True)
    for c in cams.values():
        c.requires_grad_(True)
    kw["distortion_coeff"].requires_grad_(True)
    shared = O.is_shared(name)
    v_pix, v_cam = ref.project_points(v.expand(O.N, -1, -1) if shared else v, cams["campos"], cams["camrot"], cams["focal"],
                                      cams["princpt"], **kw)
    g_pix, g_cam = (th.from_numpy(inputs[k]).to(dtype) for k in ("g_pix", "g_cam"))
    ((v_pix * g_pix).sum() + (v_cam * g_cam).sum()).backward()
    out = {"v_pix": v_pix, "v_cam": v_cam, "grad_v": v.grad}
    if dtype == th.float64:
        out.update({f"grad_{k}": c.grad for k, c in cams.items()})
        out["grad_D"] = kw["distortion_coeff"].grad
    return {k: t.detach().numpy() for k, t in out.items()}


def main():
    th.set_num_threads(1)
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else "/root/reference/drtk/utils/projection.py")
    inputs = O.make_inputs()
    os.makedirs(O.GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(O.GOLDEN, "transform_distort_inputs.npz"), **inputs)
    for name in O.CASE_NAMES:
        mode, D, fov_given, lut_on = O.CASES[name]
        rec = {"D": D}
        if not fov_given:  # what the margins of make_inputs() assumed is what the reference estimates
            est = (ref.estimate_rt_fov if mode == "radial-tangential" else ref.estimate_fisheye_fov)(th.from_numpy(D))
            assert np.array_equal(est.numpy(), O.case_fov(name)), name
            rec["fov_estimated"] = est.numpy()
        for tag, dtype in (("f64", th.float64), ("f32", th.float32)):
            for k, a in run_case(ref, name, inputs, dtype).items():
                assert np.isfinite(a).all(), (name, tag, k)
                rec[f"{k}_{tag}"] = a
        path = os.path.join(O.GOLDEN, f"transform_distort_{name}.npz")
        np.savez_compressed(path, **rec)
        culled = int((rec["v_pix_f64"][..., 2] == -1).sum())
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, max |v_pix| {np.abs(rec['v_pix_f64'][..., :2]).max():.0f} px, {culled} culled")
    rows = O.ESTIMATOR_ROWS
    rec = {"rows": rows}
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        for fn in ("estimate_rt_fov", "estimate_fisheye_fov", "estimate_fisheye62_fov"):
            rec[f"{fn}_{tag}"] = getattr(ref, fn)(th.from_numpy(rows.astype(dt))).numpy()
    np.savez_compressed(os.path.join(O.GOLDEN, "transform_distort_estimators.npz"), **rec)
    print("estimators:", {k: a.ravel().tolist() for k, a in rec.items() if k.endswith("f64")})


if __name__ == "__main__":
    main()
