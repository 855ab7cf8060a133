"""CPU: `python bench.py --gpus N` with no torchrun environment starts N ranks itself and prints ONE JSON line
(round-2 review, item 2: without this an 8-GPU node would yield eight N = 1 numbers), and the torchrun form of the
driver contract keeps working.  `--dry-run` runs everything of an N-rank run except the device work: launcher, process
group (gloo here), the nnz-balanced row cut, one collective, rank 0's line.  A plain run measures the headline alone;
`--full` adds the companions."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    return env


def _one_line(out):
    lines = [x for x in out.splitlines() if x.strip()]
    assert len(lines) == 1, lines                       # the contract: ONE JSON line on stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_bench_launches_its_own_ranks(n, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--steps", "3",
                        "--warmup", "1"], cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _one_line(r.stdout)
    assert line["n_gpus"] == n and line["ranks_in_process_group"] == n
    assert len(line["extra"]["nnz_per_rank"]) == n and all(x > 0 for x in line["extra"]["nnz_per_rank"])
    assert line["steps"] == 3 and line["warmup"] == 1


def test_bench_under_torchrun_form(tmp_path):
    """the driver's own launch line (torch.distributed.run sets WORLD_SIZE): no second launcher level"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--dry-run"], cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _one_line(r.stdout)
    assert line["n_gpus"] == 2 and len(line["extra"]["nnz_per_rank"]) == 2
    assert "launching" not in r.stderr


def test_bench_single_gpu_dry_run_needs_no_launcher(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run"], cwd=str(tmp_path), env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _one_line(r.stdout)
    assert line["n_gpus"] == 1 and "launching" not in r.stderr


def test_bench_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: float32 / float64 .npy files under 64 MB in all at the headline table's size (1.5M x 64), the sampled
    rows are the table's own values at ids that do not depend on the table, and every row's float64 sum is there."""
    import numpy as np
    import torch
    import bench
    n = 1_500_000
    E = torch.rand(n, 64, generator=torch.Generator().manual_seed(5)) - 0.5
    bench.dump_outputs(str(tmp_path / "a"), E)
    bench.dump_outputs(str(tmp_path / "b"), torch.zeros(n, 64))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["propagated_row_sums.npy", "propagated_rows_sample.npy", "propagated_rows_sample_ids.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 2 ** 20
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    ids = got["propagated_rows_sample_ids"]
    assert np.array_equal(ids, np.load(tmp_path / "b" / "propagated_rows_sample_ids.npy"))
    assert ids.shape == (bench.DUMP_SAMPLE_ROWS,) and np.all(np.diff(ids) > 0) and ids[-1] < n
    np.testing.assert_array_equal(got["propagated_rows_sample"], E.numpy()[ids.astype(np.int64)])
    np.testing.assert_allclose(got["propagated_row_sums"], E.double().sum(1).numpy(), rtol=0, atol=1e-12)


def test_bench_plain_run_leaves_companions_to_full():
    """a plain run measures the headline alone; --full turns every companion on, the --no-* options refine --full, and
    --headline-only is a plain run whatever else is given"""
    import bench
    parts = ("no_extra", "no_cpu_baseline", "no_pmc", "no_configs")
    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not plain.full and all(getattr(plain, p) for p in parts)
    full = bench.parse_args(["--full"])
    assert full.full and not any(getattr(full, p) for p in parts)
    some = bench.parse_args(["--full", "--no-configs", "--no-pmc"])
    assert some.full and some.no_configs and some.no_pmc and not some.no_extra and not some.no_cpu_baseline
    hl = bench.parse_args(["--full", "--headline-only"])
    assert not hl.full and all(getattr(hl, p) for p in parts)


@pytest.mark.gpu
def test_bench_plain_run_prints_the_headline_alone(tmp_path):
    """the whole plain single-GPU run on the device: one line with the headline fields, no companion measured"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _one_line(r.stdout)
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert line["roofline"]["launches_timed"] == 2 * 3
    for key in ("cpu_baseline", "cpu_baseline_full_eval", "secondary", "extra"):
        assert key not in line, key
    assert "under_load_after" not in line["telemetry"]
