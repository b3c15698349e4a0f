#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/refpy_geometry_{f32,f64}.npz from the REFERENCE'S OWN
drtk.utils.geometry (drtk/utils/geometry.py, pure PyTorch), imported from where it lies through
oracle/gen_golden_refpy.import_reference() (build machine only).  A process of its own: nothing of drtk_amd is
imported.  Single torch thread => deterministic accumulation order.  No test imports this file.

    python tests/gen_golden_geometry.py              # rewrites tests/golden/refpy_geometry_{f32,f64}.npz and the seam archives
    python tests/gen_golden_geometry.py --seam-only  # rewrites tests/golden/refpy_geometry_seam_{f32,f64}.npz alone

Meshes (prefix in the archive):
  band_   a UV sphere band (no pole rows): no degenerate face, 2 views, vi [F,3]; face_dpdt / vert_binormals too
  poles_  a UV sphere with its pole rows: zero-area pole triangles (two coinciding corners), 2 views, vi [F,3]
  multi_  per-view topology vi [N,F,3]: a face that lists a vertex twice, an unreferenced vertex
  seam_   (archives of its own, refpy_geometry_seam_{f32,f64}.npz) the band of sphere(5, 6) with a latitude / longitude
          atlas that has one more column of UV vertices than the mesh (the construction of drtk_amd.synthetic.
          uv_sphere_atlas): T = V + n_lat + 1 and vti != vi, vt perturbed per view, 2 views; the keys of band_
Per mesh: the inputs, the outputs of face_info / vert_normals (also with given fnorms) / face_attribute_to_vert
(/ face_dpdt / vert_binormals), and their VJPs for stored upstream gradients (g_*)."""
import argparse
import math
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden")


def sphere(n_lat, n_lon, poles):
    i = np.arange(n_lat + 1, dtype=np.float64)
    theta = math.pi * (i / n_lat if poles else (i + 1) / (n_lat + 2))
    phi = 2 * math.pi * np.arange(n_lon) / n_lon
    th_, ph_ = np.meshgrid(theta, phi, indexing="ij")
    v = np.stack([np.sin(th_) * np.cos(ph_), np.cos(th_), np.sin(th_) * np.sin(ph_)], -1).reshape(-1, 3)
    vt = np.stack([ph_ / (2 * math.pi) + 0.1 * np.cos(th_), th_ / math.pi], -1).reshape(-1, 2)
    ii, jj = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    jn = (jj + 1) % n_lon
    v00, v01, v10, v11 = ii * n_lon + jj, ii * n_lon + jn, (ii + 1) * n_lon + jj, (ii + 1) * n_lon + jn
    vi = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], 2).reshape(-1, 3)
    return v, vt, vi


def atlas(n_lat, n_lon):
    """The latitude / longitude atlas of sphere(n_lat, n_lon, .) with a column of UV vertices more than the mesh has, so that
    the last column of quads runs to u = 1 instead of wrapping around (drtk_amd.synthetic.uv_sphere_atlas' construction):
    (vt [(n_lat+1)*(n_lon+1), 2] float64, vti [F,3]), the faces in the order of sphere's vi"""
    i, j = np.arange(n_lat + 1, dtype=np.float64), np.arange(n_lon + 1, dtype=np.float64)
    w, u = np.meshgrid(0.02 + 0.96 * i / n_lat, 0.02 + 0.96 * j / n_lon, indexing="ij")
    vt = np.stack([u, w], -1).reshape(-1, 2)
    ii, jj = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    s = n_lon + 1
    v00, v01, v10, v11 = ii * s + jj, ii * s + jj + 1, (ii + 1) * s + jj, (ii + 1) * s + jj + 1
    vti = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], 2).reshape(-1, 3)
    return vt, vti


def views(v, n, rng, scale=0.05):
    """n perturbed copies of v [V,3]: each view a random rotation and a small per-vertex displacement"""
    out = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        out.append(v @ q.T + scale * rng.standard_normal(v.shape))
    return np.stack(out)


def run(drtk, dtype, name, v, vi, vt=None, vti=None, seed=0):
    G = drtk.utils.geometry
    g = th.Generator().manual_seed(seed)
    out = {}

    def t(x, req=False):
        x = th.from_numpy(np.asarray(x)).to(dtype)
        return x.requires_grad_(req)

    def rnd(*shape):
        return th.randn(*shape, generator=g, dtype=th.float64).to(dtype)

    N, V, F = v.shape[0], v.shape[1], vi.shape[-2]
    vi_t = th.from_numpy(vi).long()
    out["v"], out["vi"] = v, vi.astype(np.int32)
    # face_info: all three, with upstream gradients on each
    x = t(v, True)
    fi = G.face_info(x, vi_t)
    gs = {k: rnd(*fi[k].shape) for k in ("normals", "areas", "edges")}
    th.autograd.backward([fi[k] for k in gs], [gs[k] for k in gs])
    for k in gs:
        out[f"face_info_{k}"] = fi[k].detach().numpy()
        out[f"g_face_info_{k}"] = gs[k].numpy()
    out["face_info_grad_v"] = x.grad.numpy()
    # vert_normals from v
    x = t(v, True)
    vn = G.vert_normals(x, vi_t)
    gvn = rnd(N, V, 3)
    vn.backward(gvn)
    out["vert_normals"], out["g_vert_normals"], out["vert_normals_grad_v"] = vn.detach().numpy(), gvn.numpy(), x.grad.numpy()
    # vert_normals with given fnorms (gradient to fnorms)
    fn = t(rnd(N, F, 3).numpy(), True)
    vnf = G.vert_normals(t(v), vi_t, fn)
    vnf.backward(gvn)
    out["fnorms"], out["vert_normals_fnorms"], out["vert_normals_grad_fnorms"] = fn.detach().numpy(), vnf.detach().numpy(), fn.grad.numpy()
    # face_attribute_to_vert, A = 5
    attr = t(rnd(N, F, 5).numpy(), True)
    fv = G.face_attribute_to_vert(t(v), vi_t, attr)
    gfv = rnd(N, V, 5)
    fv.backward(gfv)
    out["attr"], out["face_attribute_to_vert"], out["g_face_attribute_to_vert"] = attr.detach().numpy(), fv.detach().numpy(), gfv.numpy()
    out["face_attribute_to_vert_grad_attr"] = attr.grad.numpy()
    if vt is not None:
        vti_t = th.from_numpy(vti).long()
        out["vt"], out["vti"] = vt, vti.astype(np.int32)
        x, y = t(v, True), t(vt, True)
        dpdt, v012 = G.face_dpdt(x, y, vi_t, vti_t)
        gd, g012 = rnd(*dpdt.shape), rnd(*v012.shape)
        th.autograd.backward([dpdt, v012], [gd, g012])
        out["face_dpdt"], out["face_dpdt_v012"], out["g_face_dpdt"], out["g_face_dpdt_v012"] = dpdt.detach().numpy(), v012.detach().numpy(), gd.numpy(), g012.numpy()
        out["face_dpdt_grad_v"], out["face_dpdt_grad_vt"] = x.grad.numpy(), y.grad.numpy()
        x, y = t(v, True), t(vt, True)
        vb = G.vert_binormals(x, y, vi_t, vti_t)
        gvb = rnd(N, V, 3)
        vb.backward(gvb)
        out["vert_binormals"], out["g_vert_binormals"] = vb.detach().numpy(), gvb.numpy()
        out["vert_binormals_grad_v"], out["vert_binormals_grad_vt"] = x.grad.numpy(), y.grad.numpy()
    return {f"{name}_{k}": (a.astype(np.float32) if dtype == th.float32 and a.dtype == np.float64 else a) for k, a in out.items()}


def seam_mesh():
    """(v [2,V,3], vi [F,3], vt [2,T,2], vti [F,3]) of seam_, from a generator of its own"""
    rng = np.random.default_rng(11)
    n_lat, n_lon = 5, 6
    v, _, vi = sphere(n_lat, n_lon, poles=False)
    vt, vti = atlas(n_lat, n_lon)
    assert vt.shape[0] == v.shape[0] + n_lat + 1 and vti.shape == vi.shape and not np.array_equal(vti, vi)
    return views(v, 2, rng), vi, np.stack([vt, vt + 0.01 * rng.standard_normal(vt.shape)]), vti


def write(tag, arrays):
    path = os.path.join(OUT, f"refpy_geometry_{tag}.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(arrays)} arrays)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seam-only", action="store_true", help="write refpy_geometry_seam_{f32,f64}.npz and leave the other two archives alone")
    only_seam = ap.parse_args().seam_only
    th.set_num_threads(1)
    from gen_golden_refpy import import_reference

    drtk = import_reference()
    seam = seam_mesh()
    for dtype, tag in ((th.float32, "f32"), (th.float64, "f64")):
        write(f"seam_{tag}", run(drtk, dtype, "seam", *seam, seed=4))
    if only_seam:
        return
    rng = np.random.default_rng(7)
    v, vt, vi = sphere(6, 8, poles=False)
    band = (views(v, 2, rng), vi, np.stack([vt, vt + 0.01 * rng.standard_normal(vt.shape)]), vi)
    v, vt, vi = sphere(5, 6, poles=True)
    poles = (views(v, 2, rng, scale=0.0), vi, np.stack([vt, vt]), vi)
    vm = rng.standard_normal((2, 7, 3))  # vertex 6 unreferenced
    vim = np.stack([np.array([[0, 1, 2], [0, 2, 3], [3, 2, 4], [4, 4, 5], [1, 0, 5]]),
                    np.array([[5, 1, 0], [0, 3, 2], [2, 1, 0], [1, 1, 3], [3, 4, 5]])])
    for dtype, tag in ((th.float32, "f32"), (th.float64, "f64")):
        arrays = {}
        arrays.update(run(drtk, dtype, "band", *band, seed=1))
        arrays.update(run(drtk, dtype, "poles", *poles, seed=2))
        arrays.update(run(drtk, dtype, "multi", vm, vim, seed=3))
        write(tag, arrays)


if __name__ == "__main__":
    main()
