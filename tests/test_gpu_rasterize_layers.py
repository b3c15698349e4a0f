"""GPU (-m gpu): `rasterize_layers` -- the K nearest triangles per pixel -- through the C ABI, the torch operator and
the Python API, against recorded layers of the committed scenes (tests/golden/layers_*.npz, from the CPU oracle:
tests/layers_oracle.py), against `rasterize` itself where the answer is known by construction (stacked sheets, a mesh
doubled onto itself, K = 1), and end to end through render / interpolate with the layers folded into the batch.

Every comparison of layers is `th.equal` on the index and on the depth BITS; the one gradient comparison uses the
project's bar for gradients, |d| <= 1e-5 + 1e-5 * max|ref| per tensor."""
import math
import os

import numpy as np
import pytest
import torch as th
from conftest import GOLDEN

import layers_oracle as LO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAXK = 8


def bits(depth):
    return depth.contiguous().view(th.int32)


def same(got, want, what):
    """(depth, index) pairs, bit for bit"""
    (gd, gi), (wd, wi) = got, want
    assert gi.shape == wi.shape and gd.shape == wd.shape, (what, gi.shape, wi.shape)
    assert gi.dtype == th.int32 and gd.dtype == th.float32, what
    assert th.equal(gi.cpu(), wi.cpu()), f"{what}: index differs in {int((gi.cpu() != wi.cpu()).sum())} pixels"
    assert th.equal(bits(gd).cpu(), bits(wd).cpu()), f"{what}: depth bits differ in {int((bits(gd).cpu() != bits(wd).cpu()).sum())} pixels"


def keys_of(depth, index):
    return LO.pack_keys(depth.cpu().numpy(), index.cpu().numpy())


def check_order(depth, index):
    LO.check_layer_properties(depth.cpu().numpy(), index.cpu().numpy())


def routes():
    import drtk_amd
    from drtk_amd import capi

    def op(v, vi, H, W, K):
        vib = vi[None].expand(v.shape[0], -1, -1) if vi.ndim == 2 else vi
        return th.ops.drtk_amd_ext.rasterize_layers(v, vib, H, W, K)

    return {"capi": capi.rasterize_layers, "op": op, "python": drtk_amd.rasterize_layers_with_depth}


def load_layers(scene):
    z = np.load(os.path.join(GOLDEN, "layers_" + scene + ".npz"))
    return th.from_numpy(z["depth"]), th.from_numpy(z["index"])


class depth_order:
    def __init__(self, order):
        self.order = order

    def __enter__(self):
        import drtk_amd

        self.before = drtk_amd.get_depth_order()
        drtk_amd.set_depth_order(self.order)

    def __exit__(self, *exc):
        import drtk_amd

        drtk_amd.set_depth_order(self.before)


# ---------------------------------------------------------------------------------------------------------------------
# recorded layers of the committed scenes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["capi", "op", "python"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("scene", LO.SCENES)
def test_layers_of_the_committed_scenes(scene, K, route):
    v, vi, H, W = LO.scene_inputs(scene)
    wd, wi = load_layers(scene)
    got = routes()[route](v.to(DEV), vi.to(DEV), H, W, K)
    same(got, (wd[:, :K], wi[:, :K]), f"{scene} K={K} {route}")
    if K == 8:
        assert int((got[1][:, 4:] != -1).sum()) == 0  # no pixel of these scenes has more than four fragments
    assert not got[0].requires_grad and not got[1].requires_grad


def test_index_only_entry_point_and_vertices_that_require_grad():
    import drtk_amd

    v, vi, H, W = LO.scene_inputs("spheres_f32")
    wd, wi = load_layers("spheres_f32")
    x = v.to(DEV).requires_grad_(True)
    index = drtk_amd.rasterize_layers(x, vi.to(DEV), H, W, 4)
    assert th.equal(index.cpu(), wi[:, :4]) and not index.requires_grad and index.grad_fn is None
    with th.autocast("cuda", dtype=th.float16):  # the operator computes in float32 under autocast
        d, i = drtk_amd.rasterize_layers_with_depth(v.to(DEV).half(), vi.to(DEV), H, W, 2)
    d2, i2 = drtk_amd.rasterize_layers_with_depth(v.to(DEV).half().float(), vi.to(DEV), H, W, 2)
    same((d, i), (d2, i2), "autocast")


@pytest.mark.parametrize("order", ["strict", "fastmath"])
@pytest.mark.parametrize("scene", LO.SCENES)
def test_layer_0_is_rasterize_under_both_depth_orders(scene, order):
    import drtk_amd

    v, vi, H, W = LO.scene_inputs(scene)
    v, vi = v.to(DEV), vi.to(DEV)
    with depth_order(order):
        d, i = drtk_amd.rasterize_layers_with_depth(v, vi, H, W, 4)
        d0, i0 = drtk_amd.rasterize_with_depth(v, vi, H, W)
        d1, i1 = drtk_amd.rasterize_layers_with_depth(v, vi, H, W, 1)
    same((d[:, 0], i[:, 0]), (d0, i0), f"{scene} {order} layer 0")
    same((d1[:, 0], i1[:, 0]), (d0, i0), f"{scene} {order} K=1")
    check_order(d, i)


# ---------------------------------------------------------------------------------------------------------------------
# ties: a mesh concatenated with itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["spheres_f32", "ragged_f32", "tutorial3_f32"])
def test_fragments_of_equal_depth_both_appear_lower_id_first(scene):
    from drtk_amd import capi

    v, vi, H, W = LO.scene_inputs(scene)
    wd, wi = load_layers(scene)
    F = vi.shape[-2]
    vi2 = th.cat([vi, vi], dim=-2).contiguous()  # ids f and f + F: identical depth
    d, i = capi.rasterize_layers(v.to(DEV), vi2.to(DEV), H, W, 8)
    d, i = d.cpu(), i.cpu()
    for j in range(4):
        same((d[:, 2 * j], i[:, 2 * j]), (wd[:, j], wi[:, j]), f"{scene}: layer {2 * j} of the doubled mesh")
        filled = wi[:, j] >= 0
        assert th.equal(bits(d[:, 2 * j + 1]), bits(wd[:, j])), f"layer {2 * j + 1}: depth bits"
        assert th.equal(i[:, 2 * j + 1], th.where(filled, wi[:, j] + F, wi[:, j])), f"layer {2 * j + 1}: ids"
    check_order(d, i)


# ---------------------------------------------------------------------------------------------------------------------
# K = 1 is rasterize, at the benchmark's geometry
# ---------------------------------------------------------------------------------------------------------------------
BENCH = {2: ("100k", 2048, 8), 3: ("250k", 2048, 8), 4: ("1M", 4096, 2)}  # BASELINE.json configs[k] as bench.py builds them for one GPU


def bench_scene(config, dtype=th.float32):
    from drtk_amd import synthetic as S
    from drtk_amd.transform import transform

    mesh, res, views = BENCH[config]
    nl, no = S.MESH_SIZES[mesh]
    v_world, vi = S.uv_sphere(nl, no, lobes=0.05, device=DEV)
    campos, camrot, focal, princpt = S.ring_cameras(views, res, res, device=DEV)
    v_pix = transform(v_world[None], campos, camrot, focal, princpt).contiguous()
    return v_pix.to(dtype), vi, res


@pytest.mark.parametrize("order", ["strict", "fastmath"])
@pytest.mark.parametrize("dtype", [th.float32, th.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("config", [2, 3, 4])
def test_one_layer_is_rasterize_at_the_benchmark_geometry(config, dtype, order):
    import drtk_amd

    v, vi, res = bench_scene(config, dtype)
    with depth_order(order):
        d, i = drtk_amd.rasterize_layers_with_depth(v, vi, res, res, 1)
        d0, i0 = drtk_amd.rasterize_with_depth(v, vi, res, res)
    assert int((i0 >= 0).sum()) > 0.2 * i0.numel()
    same((d[:, 0], i[:, 0]), (d0, i0), f"configs[{config}] {dtype} {order}")


# ---------------------------------------------------------------------------------------------------------------------
# full-size known answer: stacked sheets
# ---------------------------------------------------------------------------------------------------------------------
def sheet_mesh(H, W, nx, ny, n_views):
    """A single sheet built directly in pixel space: a grid of nx x ny quads over the whole image (so every pixel centre
    has exactly one fragment), warped so that its quads are ~100 times denser near the image borders than at the centre
    (long tile lists: heavy tiles are split), with a smooth positive z in [4.4, 5.6) that differs per view."""
    def warp(u, size):  # monotone, [0,1] -> [-0.5, size - 0.5]; derivative 1 - 0.9 cos(2 pi u)
        return (u - 0.9 * th.sin(2 * math.pi * u) / (2 * math.pi)) * size - 0.5

    ux = th.linspace(0, 1, nx + 1, dtype=th.float64)
    uy = th.linspace(0, 1, ny + 1, dtype=th.float64)
    x, y = warp(ux, W), warp(uy, H)
    x[0], x[-1], y[0], y[-1] = -0.5, W - 0.5, -0.5, H - 0.5
    yy, xx = th.meshgrid(y, x, indexing="ij")
    vs = []
    for n in range(n_views):
        z = 5.0 + 0.5 * th.sin(xx / 190.0 + 0.3 * n) * th.cos(yy / 270.0) + 0.02 * n
        vs.append(th.stack([xx, yy, z], -1).reshape(-1, 3))
    v = th.stack(vs).float()
    j, i = th.meshgrid(th.arange(ny), th.arange(nx), indexing="ij")
    a = (j * (nx + 1) + i).reshape(-1)
    b, c, d = a + 1, a + nx + 1, a + nx + 2
    vi = th.cat([th.stack([a, c, d], -1), th.stack([a, d, b], -1)]).int()
    return v, vi


@pytest.mark.parametrize("n_views", [1, 4], ids=["tiles32", "tiles64"])  # 1 view: 32-pixel tiles, 4 views: 64-pixel tiles
def test_stacked_sheets_peel_in_depth_order_at_full_size(n_views):
    import drtk_amd

    H, W, L = 2048, 1334, 4
    v1, vi1 = sheet_mesh(H, W, 232, 220, n_views)
    F, V = vi1.shape[0], v1.shape[1]
    assert F >= 100_000
    v1, vi1 = v1.to(DEV), vi1.to(DEV)
    # the sheet alone: exactly one fragment on every pixel
    d, i = drtk_amd.rasterize_layers_with_depth(v1, vi1, H, W, 2)
    assert int((i[:, 0] < 0).sum()) == 0 and int((i[:, 1] != -1).sum()) == 0 and float(d[:, 1].abs().max()) == 0.0
    z_range = float(v1[..., 2].max() - v1[..., 2].min())
    step = 2.0
    assert step > z_range
    order = [2, 0, 3, 1]  # the copy at position j of the concatenation is the order[j]-th nearest
    copies = [v1 + th.tensor([0.0, 0.0, step * order[j]], device=DEV) for j in range(L)]
    # ... and three screen-filling triangles behind the sheets (the per-view list of big triangles), nearest last
    big_z = [31.0, 27.0, 23.0]
    s = float(4 * max(H, W))
    big_v = th.cat([th.tensor([[-s, -s, z], [3 * s, -s, z + 1.0], [-s, 3 * s, z + 2.0]]) for z in big_z]).to(DEV)
    v = th.cat(copies + [big_v[None].expand(n_views, -1, -1)], dim=1).contiguous()
    big_vi = (th.arange(9, dtype=th.int32).reshape(3, 3) + L * V).to(DEV)
    vi = th.cat([vi1 + j * V for j in range(L)] + [big_vi]).contiguous()
    K = 8
    d, i = drtk_amd.rasterize_layers_with_depth(v, vi, H, W, K)
    for k in range(L):
        j = order.index(k)
        wd, wi = drtk_amd.rasterize_with_depth(copies[j], vi1, H, W)
        same((d[:, k], i[:, k]), (wd, wi + j * F), f"layer {k} = copy {j}")
    for k, t in ((4, 2), (5, 1), (6, 0)):
        wd, wi = drtk_amd.rasterize_with_depth(v, vi[L * F + t:L * F + t + 1], H, W)
        assert int((wi != 0).sum()) == 0
        same((d[:, k], i[:, k]), (wd, wi + L * F + t), f"layer {k} = big triangle {t}")
    assert int((i[:, 7] != -1).sum()) == 0 and float(d[:, 7].abs().max()) == 0.0
    check_order(d[:1], i[:1])


# ---------------------------------------------------------------------------------------------------------------------
# properties at the benchmark's sphere scene
# ---------------------------------------------------------------------------------------------------------------------
def test_properties_on_the_bench_sphere_scene():
    import drtk_amd

    v, vi, res = bench_scene(2)
    K = 4
    d, i = drtk_amd.rasterize_layers_with_depth(v, vi, res, res, K)
    d0, i0 = drtk_amd.rasterize_with_depth(v, vi, res, res)
    same((d[:, 0], i[:, 0]), (d0, i0), "layer 0")
    assert th.equal(drtk_amd.rasterize(v, vi, res, res), i[:, 0])
    # a closed convex-ish surface: the covered pixels have a back face behind the front one
    assert int((i[:, 1] >= 0).sum()) > 0.9 * int((i0 >= 0).sum())
    for n in range(0, v.shape[0], 3):
        check_order(d[n:n + 1], i[n:n + 1])
    # strict order of the keys everywhere, on the device: depth bits are positive floats, so (bits, id) orders like the key
    for k in range(K - 1):
        a_d, b_d, a_i, b_i = bits(d[:, k]).long(), bits(d[:, k + 1]).long(), i[:, k].long(), i[:, k + 1].long()
        assert int((d[:, k][a_i >= 0] <= 0).sum()) == 0
        later = (b_d > a_d) | ((b_d == a_d) & (b_i > a_i))
        assert bool((later | (b_i < 0)).all()) and bool(((a_i >= 0) | (b_i < 0)).all())
    d2, i2 = drtk_amd.rasterize_layers_with_depth(v, vi, res, res, K)
    same((d2, i2), (d, i), "second run")
    h = v.shape[0] // 2
    da, ia = drtk_amd.rasterize_layers_with_depth(v[:h].contiguous(), vi, res, res, K)
    db, ib = drtk_amd.rasterize_layers_with_depth(v[h:].contiguous(), vi, res, res, K)
    same((th.cat([da, db]), th.cat([ia, ib])), (d, i), "batch split in two")
    # float64 vertices: same contract (the depth stays float32)
    d64, i64 = drtk_amd.rasterize_layers_with_depth(v[:2].double(), vi, res, res, K)
    w64 = drtk_amd.rasterize_with_depth(v[:2].double(), vi, res, res)
    same((d64[:, 0], i64[:, 0]), w64, "float64 layer 0")
    check_order(d64[:1], i64[:1])


# ---------------------------------------------------------------------------------------------------------------------
# limits
# ---------------------------------------------------------------------------------------------------------------------
def test_num_layers_out_of_range_raises():
    import drtk_amd
    from drtk_amd import capi

    v, vi, H, W = LO.scene_inputs("two_triangles_f32")
    v, vi = v.to(DEV), vi.to(DEV)
    for K in (0, 9, -1):
        with pytest.raises(RuntimeError, match="num_layers"):
            drtk_amd.rasterize_layers(v, vi, H, W, K)
        with pytest.raises(RuntimeError, match="num_layers"):
            th.ops.drtk_amd_ext.rasterize_layers(v, vi[None], H, W, K)
        with pytest.raises(capi.DrtkAmdError, match="invalid"):
            capi.rasterize_layers(v, vi, H, W, K)


def test_empty_batches_empty_meshes_and_one_pixel_wide_images():
    import drtk_amd
    from drtk_amd import capi

    v, vi, H, W = LO.scene_inputs("two_triangles_f32")
    v, vi = v.to(DEV), vi.to(DEV)
    for fn in (capi.rasterize_layers, drtk_amd.rasterize_layers_with_depth):
        d, i = fn(v[:0], vi, H, W, 3)  # N = 0
        assert d.shape == (0, 3, H, W) and i.shape == (0, 3, H, W)
        d, i = fn(v, vi[:0], H, W, 3)  # F = 0: every layer empty, every pixel written
        assert d.shape == (1, 3, H, W) and int((i != -1).sum()) == 0 and float(d.abs().max()) == 0.0
    # width 1 (and height 1): the column / row through the triangles
    x = 20
    col = v.clone()
    col[..., 0] -= x
    for (h, w), vv in (((H, 1), col), ((1, W), v - th.tensor([0.0, 30.0, 0.0], device=DEV))):
        d, i = capi.rasterize_layers(vv, vi, h, w, 3)
        wd, wi = LO.layers(vv.cpu(), vi.cpu(), h, w, 3)
        same((d, i), (th.from_numpy(wd), th.from_numpy(wi)), f"{h}x{w}")
        assert int((i[:, 0] >= 0).sum()) > 0


def test_more_views_than_one_launch_takes():
    """70 000 tiny views: the entry point slices the batch into launches of at most 65 535 views, the [N,K,H,W] outputs
    advance by K planes per view"""
    from drtk_amd import capi
    from drtk_amd import synthetic as S

    N, H, W, K = 70000, 4, 4, 3
    v, vi = S.sphere_views(N, 6, 8, H, W)
    wd, wi = LO.layers(v, vi, H, W, K)
    assert int((wi[:, 1] >= 0).sum()) > 0.1 * N * H * W
    same(capi.rasterize_layers(v.to(DEV), vi.to(DEV), H, W, K), (th.from_numpy(wd), th.from_numpy(wi)), "70000 views")


def test_element_aligned_buffers():
    """inputs one element into a flat buffer (tests/fuzz_misaligned.py), outputs at odd element offsets of one"""
    import fuzz_all_ops as FA
    from drtk_amd import capi

    for scene in ("spheres_f32", "ragged_f32", "spheres_f64"):
        v, vi, H, W = LO.scene_inputs(scene)
        wd, wi = load_layers(scene)
        K = 4
        N = v.shape[0]
        vm, vim = FA.misaligned(v), FA.misaligned(vi)
        n = N * K * H * W
        for off in (1, 3):
            flat_d = th.full((n + 8,), float("nan"), device=DEV)
            flat_i = th.full((n + 8,), -777, dtype=th.int32, device=DEV)
            out = (flat_d[off:off + n].view(N, K, H, W), flat_i[off:off + n].view(N, K, H, W))
            assert out[0].data_ptr() % 16 != 0
            d, i = capi.rasterize_layers(vm, vim, H, W, K, out=out)
            same((d, i), (wd[:, :K], wi[:, :K]), f"{scene} at element offset {off}")
            assert int((flat_i[:off] != -777).sum()) == 0 and int((flat_i[off + n:] != -777).sum()) == 0
            assert bool(flat_d[:off].isnan().all()) and bool(flat_d[off + n:].isnan().all())
    # an odd width: no 16-byte row alignment anywhere
    v, vi, H, W = LO.scene_inputs("spheres_f32")
    wd, wi = LO.layers(v, vi, H, W - 3, 3)
    same(capi.rasterize_layers(FA.misaligned(v), FA.misaligned(vi), H, W - 3, 3), (th.from_numpy(wd), th.from_numpy(wi)), "odd width")


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay_with_changed_vertices():
    import drtk_amd
    from drtk_amd import capi
    from drtk_amd import synthetic as S

    H, W, N, K = 192, 256, 3, 4
    v0, vi = S.sphere_views(N, 18, 22, H, W, second_sphere=True, device=DEV)
    v = v0.clone()  # updated in place between replays

    def step():
        d, i = drtk_amd.rasterize_layers_with_depth(v, vi, H, W, K)  # torch op: workspace allocated inside
        d2, i2 = capi.rasterize_layers(v, vi, H, W, K)               # C ABI
        return dict(d=d, i=i, d2=d2, i2=i2)

    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(2):
            step()
    th.cuda.current_stream().wait_stream(side)
    th.cuda.synchronize()
    graph = th.cuda.CUDAGraph()
    with th.cuda.graph(graph):
        out = step()
    for k, shift in enumerate((0.0, 2.75, -6.5)):
        v.copy_(v0 + th.tensor([shift, -0.5 * shift, 0.0], device=DEV))
        graph.replay()
        th.cuda.synchronize()
        got = {n: t.clone() for n, t in out.items()}
        want = step()  # eager, same data
        th.cuda.synchronize()
        assert int((want["i"][:, 1] != -1).sum()) > 0.1 * N * H * W
        same((got["d"], got["i"]), (want["d"], want["i"]), f"replay {k}: operator")
        same((got["d2"], got["i2"]), (want["d2"], want["i2"]), f"replay {k}: C ABI")
        same((got["d"], got["i"]), (got["d2"], got["i2"]), f"replay {k}: operator against C ABI")


# ---------------------------------------------------------------------------------------------------------------------
# end to end: composite two sheets front to back
# ---------------------------------------------------------------------------------------------------------------------
def test_front_to_back_compositing_of_folded_layers_matches_two_separate_rasterize_calls():
    import drtk_amd

    H, W, C = 96, 128, 3

    def sheet(x0, x1, y0, y1, z, nx, ny, tilt):
        x = th.linspace(x0, x1, nx + 1, dtype=th.float64)
        y = th.linspace(y0, y1, ny + 1, dtype=th.float64)
        yy, xx = th.meshgrid(y, x, indexing="ij")
        zz = z + tilt * (xx / W + 0.5 * yy / H)
        v = th.stack([xx, yy, zz], -1).reshape(1, -1, 3).float()
        j, i = th.meshgrid(th.arange(ny), th.arange(nx), indexing="ij")
        a = (j * (nx + 1) + i).reshape(-1)
        vi = th.cat([th.stack([a, a + nx + 1, a + nx + 2], -1), th.stack([a, a + nx + 2, a + 1], -1)]).int()
        return v.to(DEV), vi.to(DEV)

    vA, viA = sheet(3.3, 90.7, 5.2, 80.1, 2.0, 9, 7, 0.4)       # front, translucent (per-vertex alpha)
    vB, viB = sheet(40.6, 124.2, 20.4, 93.3, 4.0, 6, 8, -0.3)   # back
    VA, VB = vA.shape[1], vB.shape[1]
    g = th.Generator().manual_seed(11)
    attrA0 = th.cat([th.rand(1, VA, C, generator=g), 0.2 + 0.6 * th.rand(1, VA, 1, generator=g)], -1).to(DEV)
    attrB0 = th.cat([th.rand(1, VB, C, generator=g), 0.7 + 0.3 * th.rand(1, VB, 1, generator=g)], -1).to(DEV)
    weight = (th.rand(1, C, H, W, generator=g) * 2 - 1).to(DEV)

    def shade(v, vi, attr, index):
        _, bary = drtk_amd.render(v, vi, index)
        img = drtk_amd.interpolate(attr, vi, index, bary) * (index != -1)[:, None]
        return img[:, :C], img[:, C:]

    def over(layers):  # front to back
        out, transmittance = 0.0, 1.0
        for rgb, alpha in layers:
            out = out + transmittance * alpha * rgb
            transmittance = transmittance * (1.0 - alpha)
        return out

    # layers of the union, folded into the batch
    K = 2
    attrA, attrB = attrA0.clone().requires_grad_(True), attrB0.clone().requires_grad_(True)
    v = th.cat([vA, vB], 1)
    vi = th.cat([viA, viB + VA])
    attr = th.cat([attrA, attrB], 1)
    index = drtk_amd.rasterize_layers(v, vi, H, W, K)
    assert int((index[:, 1] != -1).sum()) > 500 and int(((index[:, 0] >= viA.shape[0]) & (index[:, 1] == -1)).sum()) > 500
    rgb, alpha = shade(v.repeat_interleave(K, 0), vi, attr.repeat_interleave(K, 0), index.flatten(0, 1))
    img = over([(rgb[k:k + 1], alpha[k:k + 1]) for k in range(K)])
    (img * weight).sum().backward()

    # the same compositing from two rasterize calls, one per sheet (A is in front wherever both cover)
    refA, refB = attrA0.clone().requires_grad_(True), attrB0.clone().requires_grad_(True)
    ref = over([shade(vA, viA, refA, drtk_amd.rasterize(vA, viA, H, W)), shade(vB, viB, refB, drtk_amd.rasterize(vB, viB, H, W))])
    (ref * weight).sum().backward()

    def close(a, b, what):
        err, tol = float((a.double() - b.double()).abs().max()), 1e-5 + 1e-5 * float(b.abs().max())
        print(f"{what}: max |d| {err:.3e}, bar {tol:.3e}")
        assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"

    close(img.detach(), ref.detach(), "composited image")
    assert float(refA.grad.abs().max()) > 0 and float(refB.grad.abs().max()) > 0
    close(attrA.grad, refA.grad, "gradient of the front sheet's attributes")
    close(attrB.grad, refB.grad, "gradient of the back sheet's attributes")
