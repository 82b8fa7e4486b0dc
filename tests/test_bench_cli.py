"""bench.py command-line behaviour: without a GPU, and (gpu-marked) what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_launcher_starts_the_ranks_itself():
    """`python bench.py --gpus 2` with WORLD_SIZE unset (how the driver calls bench.py) must launch torch.distributed.run as
    a child and relay its return code.  Without a GPU every rank stops at 'No HIP GPUs are available': that message coming from
    the ranks (twice: one per rank) shows the launch happened; the exit code is the launcher's (non-zero), not a usage error."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MPF_BENCH_REHEARSAL="1", MPF_BENCH_N="256", MPF_BENCH_NB="64", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert "must run under torch.distributed.run" not in out.stderr
    assert out.stderr.count("No HIP GPUs are available") + out.stderr.count("bench.py needs a GPU") >= 2, out.stderr[-3000:]


def test_cpu_only_leg_prints_one_object():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-only", "--cpu-n", "512"], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["value"] > 0 and d["kind"] == "reference" and d["cores"] >= 1


def test_steps_below_one_is_a_usage_error():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr, out.stderr[-2000:]


def test_dump_outputs_is_single_gpu_only():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", "d"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--dump-outputs needs --gpus 1" in out.stderr, out.stderr[-2000:]


def test_dump_sample_is_fixed_in_bounds_and_small():
    import numpy as np
    import bench
    n = 32768
    rows, cols = bench.dump_sample_index(n)
    again = bench.dump_sample_index(n)
    assert np.array_equal(rows, again[0]) and np.array_equal(cols, again[1])
    assert 0 < len(rows) <= bench.DUMP_LU_SAMPLE and rows.min() >= 0 and rows.max() < n and cols.min() >= 0 and cols.max() < n
    flat = cols * n + rows
    assert np.all(np.diff(flat) > 0)   # distinct, column-major order
    assert 8 * (len(rows) + n + 1) <= 64 << 20   # lu_sample + ipiv + info
    assert bench.DUMP_LU_FULL_MAX_BYTES + 8 * (n + 1) <= 64 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 4096])
def test_dump_outputs_are_the_last_timed_factorization(oracle, tmp_path, n):
    """--dump-outputs writes the last timed step's IPIV, info and LU (whole at N = 1024, the fixed sample at N = 4096): the
    oracle's bits for the same input."""
    import numpy as np
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--nb", "256", "--steps", "2", "--warmup", "1",
                          "--legs", "none", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    files = sorted(os.listdir(d))
    assert files == (["info.npy", "ipiv.npy", "lu.npy"] if n == 1024 else ["info.npy", "ipiv.npy", "lu_sample.npy"])
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    got = {f[:-4]: np.load(d / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    LU_o, ip_o = oracle.mpf(oracle.matgen_skip(n), 256)
    assert got["info"].tolist() == [0.0]
    assert np.array_equal(got["ipiv"], ip_o.astype(np.float64))
    if n == 1024:
        assert got["lu"].shape == (n, n) and np.array_equal(got["lu"].view(np.uint64), LU_o.view(np.uint64))
    else:
        import bench
        rows, cols = bench.dump_sample_index(n)
        assert np.array_equal(got["lu_sample"].view(np.uint64), LU_o[rows, cols].view(np.uint64))
