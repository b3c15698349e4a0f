"""GPU (-m gpu): bench.py as the driver runs it -- `python bench.py ...` at N = 1 and
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`
for N > 1 -- prints exactly ONE JSON line (rank 0) that carries the contract's keys.  A one-GPU box cannot run RCCL
between ranks, so the two ranks share the GPU and use gloo (bench.py's test switches DRTK_DIST_BACKEND / DRTK_FORCE_DEVICE):
everything around the collective is the real thing -- rank set-up, view sharding, the side-stream gradient reducer on
HIP streams, max-over-ranks timing, rank 0 reporting while the other rank waits at the final barrier.  Small workload:
this checks the launch path and the contract, not performance."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--mesh", "10k", "--res", "512", "--views", "2", "--channels", "3", "--steps", "3", "--warmup", "1", "--kernel-steps", "2", "--full"]
TOP = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
       "dtype", "data", "config", "roofline", "cpu_baseline"}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, extra_env=None):
    env = dict(os.environ)
    env.update(extra_env or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, f"{' '.join(cmd)} exited {r.returncode}\n{r.stderr[-3000:]}"
    # stdout carries the JSON line and NOTHING else (RCCL's version banner, printed to descriptor 1 when a communicator is
    # created, used to land here: bench.py points descriptor 1 at stderr and writes its line to a duplicate of the real one)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), f"expected ONE JSON line and nothing else on stdout, got {len(lines)}:\n{r.stdout[-2000:]}"
    return json.loads(lines[0])


def _check_common(d, n_gpus):
    assert TOP <= set(d), f"missing keys: {sorted(TOP - set(d))}"
    assert d["n_gpus"] == n_gpus and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = pixels of ALL ranks / max-over-ranks time
    px = n_gpus * d["config"]["views_per_gpu"] * d["config"]["height"] * d["config"]["width"]
    assert abs(d["value"] - px / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    rf = d["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "frac_traffic"} <= set(rf)
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    # `traffic` is replayed from a committed PMC collection: the line says whether the priced kernel's source still is what the
    # counters were taken on (None where no collection covers the shape, as on these small test shapes)
    assert "traffic_stale" in rf and (rf["traffic_stale"] is None) == (rf["traffic"] is None)
    assert d["config"]["grad_reset"] == ("set_to_none" if n_gpus == 1 and d["all_reduce"] is None else "flat_zero")
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0 < rf["frac"] < 1
    assert "ms_per_step_median_hipevent" in d and 0 < d["ms_per_step_median_hipevent"] <= d["ms_per_step"] * 1.5
    # ONE HIP kernel is priced: the one with the largest per-launch time among the kernels that stream per-pixel tensors
    ks = d["path_roofline"]["kernels"]
    priced = {k: r for k, r in ks.items() if r["bytes_per_px"]}
    # (within 3 % of the largest: a tie goes to the kernel furthest below the roofline, bench.py)
    t_max = max(r["ms_per_launch"] for r in priced.values())
    tied = [k for k, r in priced.items() if r["ms_per_launch"] >= 0.97 * t_max]
    assert rf["kernel"] == min(tied, key=lambda k: priced[k]["GBps"]) and rf["ms_per_launch"] == priced[rf["kernel"]]["ms_per_launch"]
    P = d["config"]["views_per_gpu"] * d["config"]["height"] * d["config"]["width"]
    assert rf["algorithmic_bytes"] == rf["bytes_per_px"] * P
    assert abs(rf["achieved"] - rf["algorithmic_bytes"] / (rf["ms_per_launch"] * 1e-3) / 1e9) < 1.0
    # every library kernel of the step was timed, each at least once per step, and their sum is t_ops
    for k in ("tile_raster_kernel", "render_kernel", "interpolate_kernel", "edge_dots_kernel", "edge_scatter_pairs_kernel", "render_backward_kernel"):
        assert k in ks and ks[k]["launches_per_step"] >= 1 and ks[k]["ms_per_step"] > 0, k
    assert abs(d["path_roofline"]["t_ops_ms"] - sum(r["ms_per_step"] for r in ks.values() if r["op"] != "outside the four ops")) < 1e-2
    assert d["path_roofline"]["t_ops_ms"] < d["ms_per_step"] * 1.05
    # No kernel may be credited with more than the HBM peak on the bytes it MOVES (a figure above the peak means the
    # kernel is not streaming what it is priced with -- round 2's edge_dots, 8.09 TB/s on 8d's bytes while it skips the
    # background); the same for the counter-based rate wherever a PMC collection covers the kernel.
    for k, r in priced.items():
        assert 0 < r["GBps_moved"] <= rf["peak"], (k, r)
        assert r["bytes_per_px_moved"] <= r["bytes_per_px"] + 1e-9, (k, r)
        if "GBps_traffic" in r:
            assert 0 < r["GBps_traffic"] <= rf["peak"], (k, r)
    assert 0 < rf["frac_moved"] <= rf["frac"] + 1e-3  # (both rounded to four digits)
    pr = d["path_roofline"]
    assert 0 < pr["frac_ops_moved"] <= pr["frac_ops_fused_bytes"] + 1e-3 <= pr["frac_ops"] + 2e-3


def test_single_process_line_carries_roofline_and_cpu_baseline():
    d = _run([sys.executable, "bench.py", *SMALL, "--cpu-sample-views", "1"])
    _check_common(d, 1)
    cb = d["cpu_baseline"]
    assert {"value", "unit", "cores", "kind", "sample"} <= set(cb)
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "Mpix/s"
    # the captured-graph replay of the same step is reported beside the eager headline, with the same loss
    g = d["graph_step"]
    assert "error" not in g, g
    assert g["ms_per_step"] > 0 and abs(g["loss"] - d["loss"]) <= 1e-5 * max(1.0, abs(d["loss"]))
    # the operators alone (no user-side mask / loss), wall clock: beside the headline, and necessarily faster than it
    # ... and the N = 1 step the way the ranks of a group clear their gradients (the scaling curve's like-for-like point)
    fz = d["extensions"]["grad_reset_flat_zero"]
    assert fz["ms_per_step"] > 0 and 0.5 < fz["ms_per_step"] / d["ms_per_step"] < 2.0
    oo = d["extensions"]["operators_only"]
    assert 0 < oo["ms_per_step"] < d["ms_per_step"] and oo["value"] > d["value"]
    assert oo["ms_per_step"] >= d["path_roofline"]["t_ops_ms"] * 0.9  # ... and not faster than its own kernels


def test_gpus_flag_must_match_the_process_group():
    """`python bench.py --gpus 4` without a launcher used to run on ONE GPU and label the line n_gpus = 1 under the
    multi-GPU metric: now it refuses and prints the launch line (it must not spawn or re-exec ranks itself)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", *SMALL], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "torch.distributed.run" in r.stderr and "--nproc-per-node 4" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_textured_workload_line():
    """`--workload textured` (BASELINE configs[4] in small): same contract, its own metric string, fp16-stored leaves."""
    d = _run([sys.executable, "bench.py", "--workload", "textured", "--mesh", "10k", "--res", "512", "--tex", "512", "--views", "2",
              "--steps", "3", "--warmup", "1", "--kernel-steps", "2", "--cpu-sample-views", "1", "--full"])
    assert TOP <= set(d) and "textured" in d["metric"] and "fp16" in d["config"]["workload"]
    ks = d["path_roofline"]["kernels"]
    for k in ("uv_derivative_kernel", "mipmap_forward_lean_kernel", "mipmap_backward_lean_kernel", "tile_raster_kernel", "edge_dots_kernel"):
        assert k in ks and ks[k]["ms_per_step"] > 0, k
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    assert "error" not in d["graph_step"]


@pytest.mark.parametrize("ranks", [2, 8])
def test_ranks_under_torch_distributed_run(ranks):
    """The driver's own launch line with 2 and with 8 ranks (the node size SCALE_rNN.json is collected on) sharing the one
    GPU over gloo: one JSON line from rank 0, exit code 0 on every rank, two collectives per step in the fixed order."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", "--gpus", str(ranks), *SMALL]
    d = _run(cmd, {"DRTK_DIST_BACKEND": "gloo", "DRTK_FORCE_DEVICE": "0"})
    _check_common(d, ranks)
    assert d["cpu_baseline"] is None  # rank 0 at N = 1 only
    assert f"sharded {ranks}-way" in d["config"]["parallelism"] and "all-reduced" in d["config"]["parallelism"]
    ar = d["all_reduce"]
    assert ar["bytes"] == 4 * d["config"]["vertices"] * (3 + d["config"]["channels"]) and ar["collectives_per_step"] == 2
    assert ar["staging_dtype"] == "float32"
    assert ar["ms_launch_to_done"] > 0 and ar["ms_exposed_on_main_stream"] >= 0


def test_one_rank_process_group_over_rccl():
    """The multi-rank code path of bench.py -- reducers launched from the backward pass, the max over ranks of the timing,
    the all_reduce block of the line, barrier and teardown -- against RCCL itself (backend "nccl"), which the two-rank
    gloo leg above cannot reach on a one-GPU box: a process group of ONE rank (DRTK_SINGLE_RANK_GROUP, test-only)."""
    env = {"DRTK_SINGLE_RANK_GROUP": "1", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
           "MASTER_PORT": str(_free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0", "DRTK_DIST_BACKEND": ""}
    d = _run([sys.executable, "bench.py", "--gpus", "1", *SMALL, "--no-graph", "--cpu-sample-views", "0"], env)
    _check_common(d, 1)
    ar = d["all_reduce"]
    assert ar is not None and ar["collectives_per_step"] == 2 and ar["staging_dtype"] == "float32"
    assert ar["bytes"] == 4 * d["config"]["vertices"] * (3 + d["config"]["channels"])
    assert ar["ms_launch_to_done"] > 0 and ar["ms_exposed_on_main_stream"] >= 0


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """Without --full the line carries the headline alone (none of the extra measurements), --steps is the number of timed
    steps, and --dump-outputs writes what the last timed step computed: float32 / float64 .npy files, 64 MB at most.  Two
    runs with the same workload start from the same inputs, so whatever their step counts their last steps agree."""
    import numpy as np

    lean = ["--mesh", "10k", "--res", "512", "--views", "2", "--channels", "3", "--warmup", "1"]
    runs = []
    for steps in (2, 5):
        out = tmp_path / f"steps{steps}"
        d = _run([sys.executable, "bench.py", *lean, "--steps", str(steps), "--dump-outputs", str(out)])
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "loss"} <= set(d)
        assert not {"roofline", "path_roofline", "cpu_baseline", "graph_step", "extensions", "all_reduce"} & set(d)
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["unit"] == "Mpix/s" and d["dtype"] == "f32"
        px = d["config"]["views_per_gpu"] * d["config"]["height"] * d["config"]["width"]
        assert abs(d["value"] - px / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
        files = {f.stem: np.load(f) for f in out.glob("*.npy")}
        assert set(files) == {"loss", "index_img", "depth_img", "bary_img", "img", "grad_v_world", "grad_attr"}
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert abs(float(files["loss"]) - d["loss"]) <= 1e-5 * max(1.0, abs(d["loss"]))
        assert files["index_img"].shape == (2, 512, 512) and files["grad_attr"].shape == (1, d["config"]["vertices"], 3)
        assert files["img"].shape == (1 << 20,)  # 2 x 3 x 512 x 512 elements: a seeded sample
        runs.append(files)
    a, b = runs
    for name in ("index_img", "depth_img", "bary_img"):
        assert np.array_equal(a[name], b[name]), name
    for name in ("loss", "img", "grad_v_world", "grad_attr"):
        tol = 1e-5 + 1e-5 * float(np.abs(b[name]).max())
        assert float(np.abs(a[name].astype(np.float64) - b[name]).max()) <= tol, name


def test_plain_textured_run_dumps_its_outputs(tmp_path):
    """--dump-outputs on the textured workload: the fp16-stored leaves' gradients are written too (the whole texture
    pyramid's as one sampled array), all in float32 / float64 within 64 MB."""
    import numpy as np

    d = _run([sys.executable, "bench.py", "--workload", "textured", "--mesh", "10k", "--res", "512", "--tex", "512", "--views", "2",
              "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert "textured" in d["metric"] and d["steps"] == 2 and d["ms_per_step"] > 0 and "roofline" not in d
    files = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert set(files) == {"loss", "index_img", "depth_img", "bary_img", "img", "grad_v_world", "grad_vt", "grad_tex"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert abs(float(files["loss"]) - d["loss"]) <= 1e-5 * max(1.0, abs(d["loss"]))
    assert files["grad_vt"].shape[-1] == 2 and float(np.abs(files["grad_tex"]).max()) > 0
