"""bench.py --dump-outputs (tools/bench_dump.py): float32 / float64 files, at most 64 MB in all, larger arrays as a seeded sample of
rows that depends on the shapes only.  CPU tensors and arrays stand in for the device buffers; the bench's own runs are in
tests/test_gpu_bench_contract.py."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_dump  # noqa: E402


def test_small_outputs_are_written_whole_in_float32_or_float64(tmp_path):
    count = torch.arange(7, dtype=torch.int32)
    out = torch.linspace(-1, 1, 21, dtype=torch.float32).reshape(7, 3)
    half = np.linspace(0, 1, 5).astype(np.float16)
    f64 = np.linspace(0, 1, 4)
    flags = np.array([True, False, True])
    w = bench_dump.dump_outputs(str(tmp_path), {"count": count, "out": out, "half": half, "f64": f64, "flags": flags})
    assert w == {"count": [7], "out": [7, 3], "half": [5], "f64": [4], "flags": [3]}
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in w)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in w}
    assert got["count"].dtype == np.float64 and np.array_equal(got["count"], np.arange(7))
    assert got["out"].dtype == np.float32 and np.array_equal(got["out"], out.numpy())
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], half.astype(np.float32))
    assert got["f64"].dtype == np.float64 and np.array_equal(got["f64"], f64)
    assert got["flags"].dtype == np.float64 and np.array_equal(got["flags"], [1.0, 0.0, 1.0])


def test_large_outputs_are_cut_to_a_seeded_sample_of_rows(tmp_path):
    limit = 1_000_000
    n_rows, C = 10001, 64                                        # 2.6 MB of rows; the counts, 80 kB in float64, stay whole
    count = torch.randint(0, 1000, (n_rows,), dtype=torch.int32)
    out = torch.randn(n_rows, C)
    w = bench_dump.dump_outputs(str(tmp_path / "a"), {"count": count, "out": out}, limit=limit)
    k = w["out"][0]
    assert w == {"count": [n_rows], "out_rows": [k], "out": [k, C]} and 1000 < k < n_rows
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    rows = np.load(tmp_path / "a" / "out_rows.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n_rows
    assert np.array_equal(np.load(tmp_path / "a" / "out.npy"), out.numpy()[rows.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "count.npy"), count.numpy().astype(np.float64))      # small: whole
    # the sample is a function of the shapes alone: other values, same rows
    bench_dump.dump_outputs(str(tmp_path / "b"), {"count": count, "out": torch.zeros(n_rows, C)}, limit=limit)
    assert np.array_equal(np.load(tmp_path / "b" / "out_rows.npy"), rows)


def test_the_flagship_shapes_fit_the_limit():
    # R2: hit counts [200001] int32 written whole, feature sums [200001, 512] fp32 (410 MB) sampled
    k, big = bench_dump.plan({"count": ((200001,), np.int32), "out": ((200001, 512), np.float32)})
    assert big == ["out"] and k > 20000
    assert 200001 * 8 + k * (512 * 4 + 8) + 3 * 4096 <= bench_dump.LIMIT_BYTES
    assert bench_dump.plan({"count": ((10001,), np.int32), "out": ((10001, 32), np.float32)}) == (None, [])      # S0: whole


def test_bench_refuses_zero_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and "{" not in r.stdout
