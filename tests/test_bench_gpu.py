"""bench.py's multi-rank branch as a dry run on ONE GPU: two ranks over the `gloo` backend sharing the device
(MICROMIX_BENCH_BACKEND=gloo).  Not a measurement -- it checks that the script the driver launches for N > 1 runs to its JSON line:
rendezvous, K-shard layer, settle phase with the ranks in step, timed region, GEMM / all-reduce split, row-parallel figure, MLP
pairing.  (With >= 2 GPUs tests/test_tp_rccl_gpu.py covers the RCCL path itself.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_dry_run(tmp_path):
    """the driver's own form of the command: `python bench.py --gpus 2 ...` with no rendezvous in the environment -- bench.py starts its
    ranks itself (torch.distributed.run as a child process) and relays rank 0's line; --full for the split, row-parallel and MLP figures"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MICROMIX_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    details = str(tmp_path / "bench_details_tp2.json")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--details", details]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 6144, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["parallelism"].startswith("tp2")
    assert d["tp"]["gemm_us"] > 0 and d["tp"]["allreduce_us"] > 0 and d["tp"]["allreduce_payload_bytes"] == 4096 * 4096 * 2
    assert d["row_parallel_no_exchange"]["global_rows"] == 8192 and d["tp_mlp"]["mlp_us"] > 0
    with open(details) as f:
        full = json.load(f)
    assert {"gemm_us_max_over_ranks", "allreduce_us_max_over_ranks", "allreduce_payload_bytes", "rank0_roofline"} <= set(full["tp"])


def test_bench_line_is_short_and_complete(tmp_path):
    """one rank, --full with few steps: ONE line under 6 KB with every figure beside the headline"""
    details = str(tmp_path / "bench_details_test.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--details", details],
                       capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 6144
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["roofline"]["frac"] > 0.2 and d["cpu_baseline"]["value"] > 0
    assert set(d["mixed"]) >= {"q_o_all_fp4", "q_o_3072_896_128", "down_12288_1024_1024"} and d["roofline"]["zero_operands"]["kernel_us"] > 0
    assert "power" in d and "llama_layer" in d and "quantizers" in d
    assert d["graph_launch_ms_per_step"] > 0 and d["details"] == details and os.path.exists(details)


def test_plain_run_times_the_headline_only():
    """without --full: the headline keys, nothing measured beside them, no details file, and at most 30 s spent outside the
    warm-up and timed steps (a new process: imports, inputs, operands and the settle phase included)"""
    import time
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "TFLOP/s" and d["value"] == pytest.approx(2.0 * 4096 ** 3 / (d["ms_per_step"] * 1e-3) / 1e12, rel=1e-3)
    assert d["metric"].startswith("mixed-MX GEMM TFLOPS") and d["dtype"] == "mxfp8 x mxfp4 -> f32 acc -> bf16" and d["prewarm_s"] >= 1.5
    extras = ("roofline", "cpu_baseline", "power", "mixed", "few_tiles", "decode", "small_m", "small_m_hbm", "quantizers", "qlinear",
              "llama_layer", "published_config", "graph_launch_ms_per_step", "details")
    assert not [k for k in extras if k in d]
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 < 30.0, f"{wall:.1f} s"


def test_dump_outputs_are_the_timed_product(tmp_path):
    """--dump-outputs after the timed steps: the last step's [M, N] product, equal from run to run (fixed inputs), and equal to the same
    GEMM computed again in this process on the bench's inputs; `steps` and `ms_per_step` in the line are the timed steps'"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from micromix_amd import mixedgemm
    dumps = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "1", "--no-extras",
                            "--details", str(tmp_path / f"details_{run}.json"), "--dump-outputs", d],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
        assert line["steps"] == 7 and line["ms_per_step"] > 0
        dumps.append({n: np.load(os.path.join(d, f"{n}.npy")) for n in ("out_rows", "out_row_sum", "out_col_sum")})
    for n in dumps[0]:
        assert dumps[0][n].dtype in (np.float32, np.float64) and np.array_equal(dumps[0][n], dumps[1][n]), n
    dev = torch.device("cuda:0")
    x, w, idx = (t.to(dev) for t in bench.synth_inputs())
    a = mixedgemm.reorder_quantize_x(x, idx, *bench.SPLIT)
    b = mixedgemm.reorder_quantize_w4(w, idx, *bench.SPLIT)
    want = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5]).cpu()
    bench.dump_outputs(str(tmp_path / "here"), want)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], np.load(tmp_path / "here" / f"{n}.npy")), n
