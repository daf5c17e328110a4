"""bench.py's plain run: --steps sets the timed steps, the line carries ms_per_step, the secondary measurements stay behind
--full, and --dump-outputs writes the Q1 result of the last timed step exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BENCH = os.path.join(ROOT, "bench.py")


def load_dump(d):
    import bench
    a, r = np.load(os.path.join(d, "q1_result.npy")), np.load(os.path.join(d, "q1_result_residual.npy"))
    assert a.dtype == np.float64 and r.dtype == np.float64 and a.shape == r.shape and a.shape[1] == len(bench.Q1_COLUMNS)
    out = {}
    for ra, rr in zip(a, r):
        v = [int(x) + int(y) for x, y in zip(ra, rr)]
        out[(bytes([v[0]]), bytes([v[1]]))] = dict(zip(bench.Q1_COLUMNS[2:], v[2:]))
    return out


def test_dump_outputs_holds_wide_sums_exactly(tmp_path):
    import bench
    rows = {(b"N", b"O"): dict(sum_qty=12345, sum_base_price=2**53 + 1, sum_disc_price=2**100 + 12345, sum_charge=-(2**70) - 7, sum_disc=5, count=9),
            (b"A", b"F"): dict(sum_qty=1, sum_base_price=2, sum_disc_price=3, sum_charge=2**63 + 1, sum_disc=5, count=6)}
    bench.dump_outputs(str(tmp_path), rows)
    assert load_dump(str(tmp_path)) == rows
    keys = np.load(os.path.join(tmp_path, "q1_result.npy"))[:, :2]
    assert keys.tolist() == [[ord("A"), ord("F")], [ord("N"), ord("O")]]       # ordered by the two keys


def test_zero_steps_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_result(gpu, tmp_path):
    """A plain run at 8 M rows: the line's steps / ms_per_step / value agree, nothing of --full ran, and the dumped table is
    the CPU oracle's Q1 over the same seeded rows."""
    from databend_amd import tpch
    from tests import oracle_lib
    n, steps = 8_000_000, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rows", str(n),
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert len(out["roofline"]["kernel_ms_min_median_max"]) == 3
    for key in ("hand_written_kernel", "multi_gpu_readiness", "q1_operator_plan", "cpu_baseline", "q3_sf100", "distributed_plan_stages",
                "scan_side_zstd", "ann", "q1_block_size_sweep"):
        assert out[key] is None, key
    li = tpch.LineitemTorch(n, seed=2)
    exp = oracle_lib.q1_run(li.host(), tpch.Q1_CUTOFF, threads=8)
    assert load_dump(str(tmp_path)) == exp
