"""TEST INFRASTRUCTURE -- seeded inputs and the case table of the distortion camera models of `transform`
(tests/golden/transform_distort_<case>.npz, written by tests/gen_golden_transform_distort.py from the reference's own
`project_points`; read by test_transform_distort_host.py and test_gpu_transform_distort.py).

Shape: N = 3 views, V = 257 vertices -- one 256-thread block plus one tail lane, the smallest shape that crosses a block
boundary.  Camera-space x/z, y/z ~ N(0, 0.6) and z ~ U(0.5, 2), the first 8 vertices of each view behind the camera;
fov = (0.9, 1.3, 0.7), so a good part of every view lies beyond it and every clamp of the models is exercised on both
sides.  A float32 evaluation must not take another branch than the float64 one: `make_inputs` resamples, in float64,
every vertex that comes within MARGIN (relative) of a clamp or cull boundary of ANY case -- r against fov, |x|, |y|
against fov, the fisheye62 clamp after the distortion, the lookup table's +-1."""
import os

import numpy as np

N, V = 3, 257
SEED = 20240611
MARGIN = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FOV = (0.9, 1.3, 0.7)
RT = (-0.25, 0.08, 2e-3, -3e-3, -0.02, 0.05, -0.01, 0.002)
FISHEYE = (-0.03, 0.02, -0.01, 0.004)
FISHEYE62 = FISHEYE + (-0.002, 0.001, 2e-3, -3e-3)
RT_NOFOV = (-0.3, 0.02, 2e-3, -3e-3)       # estimate_rt_fov ~ 1.14
FISHEYE_NOFOV = (0.2, -0.6, 0.1, 0.0)      # estimate_fisheye_fov ~ 1.205
VIEW_SCALE = (1.0, 0.9, 1.1)               # row n of a coefficient table is the row above times VIEW_SCALE[n]
LUT_SHAPE = (N, 2, 9, 13)                  # not square: pins which axis is normalised by which size
LUT_SPACING = (90.0, 50.0)


def _rows(row):
    return np.asarray(row, dtype=np.float64)[None] * np.asarray(VIEW_SCALE)[:, None]


_MIXED_D = np.stack([_rows(RT[:4])[0], _rows(FISHEYE)[1], _rows(RT[:4])[2]])

# name -> (distortion_mode, coefficient table [N,ncoef], fov given?, lookup table?); "<name>_shared" adds v[:1]
BASE_CASES = {
    "rt4": ("radial-tangential", _rows(RT[:4]), True, False),
    "rt5": ("radial-tangential", _rows(RT[:5]), True, False),
    "rt8": ("radial-tangential", _rows(RT), True, False),
    "fisheye": ("fisheye", _rows(FISHEYE), True, False),
    "fisheye62": ("fisheye62", _rows(FISHEYE62), True, False),
    "fisheye62_lut": ("fisheye62_lut", _rows(FISHEYE62), True, True),
}
CASES = dict(BASE_CASES)
CASES.update({k + "_shared": v for k, v in BASE_CASES.items()})
CASES.update({
    "mixed": (["pinhole", "fisheye", "radial-tangential"], _MIXED_D, True, False),
    "fisheye62_nofov": ("fisheye62", _rows(FISHEYE62), False, False),
    "rt_nofov": ("radial-tangential", _rows(RT_NOFOV), False, False),
    "fisheye_nofov": ("fisheye", _rows(FISHEYE_NOFOV), False, False),
})
CASE_NAMES = list(CASES)

# coefficient rows of the estimator table (8 wide; estimate_rt_fov reads 2, estimate_fisheye_fov 4, estimate_fisheye62_fov 6)
ESTIMATOR_ROWS = np.asarray([
    RT, FISHEYE62, RT_NOFOV + (0.0,) * 4, FISHEYE_NOFOV + (0.0,) * 4,
    (0.1, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),          # monotonic: +inf / tan(pi/2)
    (-0.2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),          # leading zeros
    (0.05, -0.02, 0.01, -0.3, 0.2, -0.4, 0.0, 0.0),     # the k4, k5 tail decides
], dtype=np.float64)


def is_shared(name):
    return name.endswith("_shared")


def _clamp_z(z):
    return np.where(z < 0, np.minimum(z, -1e-8), np.maximum(z, 1e-8))


def _rel(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return np.where(np.isfinite(b), d, np.inf)


def _margins(v_cam, mode, D, fov, focal, princpt, lut):
    """[V] smallest relative distance of one view's camera-space points to a boundary of `mode` (float64)."""
    if mode in (None, "pinhole"):
        return np.full(v_cam.shape[0], np.inf)
    p = v_cam[:, :2] / _clamp_z(v_cam[:, 2:3])
    r = np.sqrt((p * p).sum(-1))
    m = _rel(r, fov)
    if mode == "radial-tangential":
        return np.minimum(m, _rel(np.abs(p), fov).min(-1))
    if mode == "fisheye":
        return m
    rc = np.clip(r, 1e-8, fov)
    th = np.arctan(rc)
    thd = th * (1 + sum(D[k] * th ** (2 * k + 2) for k in range(6)))
    q = p * (thd / rc)[:, None]
    m = np.minimum(m, _rel(np.abs(q), fov).min(-1))
    if lut:
        q = np.clip(q, -fov, fov)
        x, y = q[:, 0], q[:, 1]
        rr = x * x + y * y
        d = q + np.stack(((2 * x * x + rr) * D[6] + 2 * x * y * D[7], 2 * x * y * D[6] + (2 * y * y + rr) * D[7]), -1)
        pix = d @ focal.T + princpt
        pos = pix / np.asarray(LUT_SPACING) / (np.asarray(LUT_SHAPE[2:]) - 1) * 2 - 1
        m = np.minimum(m, _rel(np.abs(pos), 1.0).min(-1))
    return m


def case_fov(name):
    """[N,1] float64: the fov the case is evaluated with (given, or what the model estimates from the coefficients)."""
    mode, D, given, _ = CASES[name]
    if given:
        return np.asarray(FOV, dtype=np.float64)[:, None]
    from drtk_amd.transform import estimate_fisheye_fov, estimate_rt_fov

    return np.asarray((estimate_rt_fov if mode == "radial-tangential" else estimate_fisheye_fov)(D), dtype=np.float64)


def make_inputs():
    """dict of float64 arrays: v [N,V,3], campos, camrot, focal, princpt, fov [N,1], lut [N,2,9,13], lut_spacing [N,2],
    g_pix, g_cam [N,V,3] (the stored upstream gradients of v_pix and v_cam)."""
    rng = np.random.RandomState(SEED)
    campos = 0.1 * rng.randn(N, 3)
    camrot = np.stack([np.linalg.qr(np.eye(3) + 0.05 * rng.randn(3, 3))[0] for _ in range(N)])
    camrot *= np.sign(np.diagonal(camrot, axis1=1, axis2=2))[:, None, :]  # near +identity
    focal = np.tile(np.asarray([[500.0, 1.5], [0.0, 480.0]]), (N, 1, 1))
    princpt = np.tile(np.asarray([320.0, 240.0]), (N, 1))
    lut = 3.0 * rng.randn(*LUT_SHAPE)
    spacing = np.tile(np.asarray(LUT_SPACING), (N, 1))

    def draw(count, behind):
        z = rng.uniform(0.5, 2.0, count) * np.where(behind, -1.0, 1.0)
        xy = 0.6 * rng.randn(count, 2) * z[:, None]
        return np.concatenate([xy, z[:, None]], -1)

    behind = np.arange(V) < 8
    v = np.stack([draw(V, behind) @ camrot[n] + campos[n] for n in range(N)])  # world = R^T cam + campos
    fovs = {name: case_fov(name) for name in CASES}
    for _ in range(100):
        bad = np.zeros((N, V), dtype=bool)
        for name, (mode, D, _, lut_on) in CASES.items():
            for n in range(N):
                src = 0 if is_shared(name) else n
                cam = (v[src] - campos[n]) @ camrot[n].T
                m = _margins(cam, mode[n] if isinstance(mode, list) else mode, D[n], fovs[name][n, 0], focal[n], princpt[n], lut_on)
                bad[src] |= m < MARGIN
        if not bad.any():
            break
        for n in range(N):
            idx = np.nonzero(bad[n])[0]
            if len(idx):
                v[n, idx] = draw(len(idx), behind[idx]) @ camrot[n] + campos[n]
    else:
        raise AssertionError("could not move every vertex away from the clamp boundaries")
    return dict(v=v, campos=campos, camrot=camrot, focal=focal, princpt=princpt, fov=np.asarray(FOV)[:, None], lut=lut,
                lut_spacing=spacing, g_pix=rng.uniform(-1, 1, (N, V, 3)), g_cam=rng.uniform(-1, 1, (N, V, 3)))


def _npz(stem):
    with np.load(os.path.join(GOLDEN, f"transform_distort_{stem}.npz")) as z:
        return {k: z[k] for k in z.files}


def load(name):
    """The fixture of one case with the inputs all cases share: {key: numpy array}."""
    return dict(_npz("inputs"), **_npz(name))


def case_kwargs(name, data, dtype, device="cpu"):
    """(v, cameras dict, distortion kwargs) of a case as torch tensors of `dtype` on `device`, from its fixture `data`."""
    import torch as th

    mode, _, fov_given, lut_on = CASES[name]
    t = lambda a: th.from_numpy(np.asarray(a)).to(dtype).to(device)  # noqa: E731
    v = t(data["v"][:1] if is_shared(name) else data["v"])
    cams = {k: t(data[k]) for k in ("campos", "camrot", "focal", "princpt")}
    kw = dict(distortion_mode=mode, distortion_coeff=t(data["D"]))
    if fov_given:
        kw["fov"] = t(data["fov"])
    if lut_on:
        kw["lut_vector_field"] = t(data["lut"])
        kw["lut_spacing"] = t(data["lut_spacing"])
    return v, cams, kw
