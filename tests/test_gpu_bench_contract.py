"""bench.py's output contract on the plumbing workload (S0: 10k voxels x 8 views x 64x64x32): ONE JSON line with the
metric, and with --full the roofline object and the CPU baseline at N=1; the two-rank code path (views r::2 + all-reduce)
rehearsed with gloo on one GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _last_json(out):
    lines = [ln for ln in out.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_line_single_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "S0", "--steps", "2", "--warmup", "1",
                        "--full", "--cpu-views", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "Mvoxel-views/sec" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["value"] - 10000 * 8 / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]      # ms_per_step is printed to 3 decimals
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and rf["avg_launch_ms"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == d["unit"] and cb["sample"]
    assert d["box_miss_voxels"] == 0


def test_plain_bench_line_is_the_headline_alone():
    # without --full: set-up, warm-up, the timed steps and the line -- no pre-pass, roofline, checks or CPU baselines
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "S0", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "step_ms", "phase_ms_per_step"):
        assert k in d, k
    assert d["metric"] == "Mvoxel-views/sec" and d["unit"] == "Mvoxel-views/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and abs(d["value"] - 10000 * 8 / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
    for k in ("roofline", "cpu_baseline", "cpu_baseline_1t", "cpu_torch_loop", "checksum", "hit_pixels_per_step", "per_call"):
        assert k not in d, k
    assert "ms_per_pass_after_timed_region" not in d["pool_placement"]


def _load_dump(path):
    got = {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}
    assert all(f.endswith(".npy") for f in os.listdir(path)) and all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path)) <= 64 * 10 ** 6
    return got


def test_bench_dumps_the_last_timed_step_the_same_way_twice(tmp_path):
    """--dump-outputs: the hit counts and feature sums of the last timed step, whole at S0, equal to what the line reports; the inputs
    are seeded, so a second process with the same arguments writes the same counts and the same sums."""
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "S0", "--steps", "3", "--warmup", "1",
                            "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _last_json(r.stdout)
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert d["dumped_outputs"]["arrays"] == {"count": [10001], "out": [10001, 32]}
        got = _load_dump(tmp_path / name)
        assert set(got) == {"count", "out"} and got["count"].dtype == np.float64 and got["out"].dtype == np.float32
        assert int(got["count"].sum()) == d["hit_pixels_per_step"]
        assert abs(got["out"].astype(np.float64).sum() - d["checksum"]) <= 1e-6 * d["checksum_abs"]
        runs.append(got)
    assert np.array_equal(runs[0]["count"], runs[1]["count"])
    a, b = runs[0]["out"], runs[1]["out"]
    assert (np.abs(a - b) / (np.abs(a).max(axis=1, keepdims=True) + 1e-30)).max() <= 1e-6


def test_bench_dump_samples_the_rows_of_outputs_beyond_64_mb(tmp_path):
    # R1's feature sums are 80001 x 512 fp32 = 164 MB: a seeded sample of rows beside their indices, the hit counts whole
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "R1", "--views", "4", "--steps", "1", "--warmup", "0",
                        "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    got = _load_dump(tmp_path)
    assert set(got) == {"count", "out", "out_rows"} and got["count"].shape == (80001,)
    k = got["out_rows"].shape[0]
    assert got["out"].shape == (k, 512) and 20000 < k < 80001 and d["dumped_outputs"]["arrays"]["out"] == [k, 512]
    assert np.all(np.diff(got["out_rows"]) > 0) and got["out_rows"][-1] <= 80000
    assert int(got["count"].sum()) == d["hit_pixels_per_step"]
    hit = got["count"][got["out_rows"].astype(np.int64)] > 0                  # rows no pixel reached stay zero
    assert np.all(got["out"][~hit] == 0) and np.all(np.abs(got["out"][hit]).max(axis=1) > 0)


def _no_launcher_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


@pytest.mark.parametrize("ranks", [2, 4])
def test_bench_gloo_rehearsal_started_by_bench_itself(ranks):
    """`python bench.py --gpus N` with NO launcher: the parent starts the N ranks as a child torchrun before touching the GPU
    and relays rank 0's line.  gloo + --single-device rehearse the multi-rank step on the one GPU of the box: the step runs
    through VoxelFeatureAggregator.add_views / add_final_views; the TIMED collective arm is the one a short untimed calibration
    of both arms found faster (round 5: no arm is the default by guess), both arms are in the line, the integers travel in one
    tensor, and the line shows the ranks' spread."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--workload", "S0", "--steps", "2", "--warmup", "1",
                        "--dist-backend", "gloo", "--single-device", "--full"], capture_output=True, text=True, timeout=900, env=_no_launcher_env())
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == ranks and d["scaling"] == "strong" and "cpu_baseline" not in d
    # north_star's collective is the default, named in the line; the headline pays it inside the pass
    c = d["collective"]
    assert "all-reduce" in d["config"]["parallelism"] and c["op"] == "all-reduce"
    assert 0 < c["collective_ms_exposed"] < d["ms_per_step"]
    assert d["hit_pixels_per_step"] > 0 and d["value"] > 0 and d["reduced_hit_pixels"] > 0
    arms, cal, timed = c["arms"], c["calibration"], c["timed_arm"]
    assert set(arms) == {"split", "whole"} == set(cal["ms"]) and c["timed_arm_chosen_by"] == cal["chosen_by"]
    assert timed == cal["pick"] and all(2 <= n <= 6 for n in cal["settling_steps"].values())
    # the rule that picked it (tools/bench_calibrate.py): the smaller minimum when both arms are steady, the steady arm when one of
    # them had a step more than 3x its own minimum, split when both had
    unsteady = [arm for arm in ("split", "whole") if max(cal["samples_ms"][arm]) > 3.0 * min(cal["samples_ms"][arm])]
    if not unsteady:
        assert timed == min(cal["ms"], key=cal["ms"].get) and cal["chosen_by"].startswith("calibration"), cal
    elif len(unsteady) == 1:
        assert timed != unsteady[0] and cal["chosen_by"].startswith("the steady arm"), cal
    else:
        assert timed == "split" and cal["chosen_by"].startswith("fallback"), cal
    other = "whole" if timed == "split" else "split"
    assert arms[timed]["ms_per_step"] == d["ms_per_step"] and arms[other]["ms_per_step"] > 0
    # (whether the timed region then confirms the calibration is not asserted: N processes on one GPU over gloo's host staging
    # swing by 2x from step to step -- profiles/r05_multi_rank_rehearsals.log has the lines)
    if timed == "split":
        # the pass's last call is cut into two row ranges; the first half's rows are reduced under the second half's gather
        assert 0 < c["split"]["rows_reduced_under_the_last_gather"] < c["split"]["of"] == 10001
    else:
        assert c["split"] is None
    assert "one int32 tensor" in c["collectives_per_pass"]
    pr = c["per_rank"]
    assert 0 < pr["projection_ms"]["min"] <= pr["projection_ms"]["max"] < d["ms_per_step"]
    assert pr["collective_ms_exposed"]["min"] <= pr["collective_ms_exposed"]["max"] == c["collective_ms_exposed"]
    assert "VoxelFeatureAggregator" in c["through"]


def test_bench_refuses_more_ranks_than_gpus():
    # one GPU on the box: `--gpus 2` over RCCL must fail loudly, never run on one GPU and print "n_gpus": 1
    import torch
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--workload", "S0"], capture_output=True, text=True,
                       timeout=300, env=_no_launcher_env())
    assert r.returncode != 0 and "visible GPU" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_two_ranks_allreduce_variant():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29535", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--workload", "S0", "--steps", "2", "--warmup", "1", "--dist-backend", "gloo",
                        "--single-device", "--collective", "reduce", "--no-other-arm", "--no-split-collective", "--full"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]          # bench verifies reduced counts exactly and sums against the ranks' own
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and "reduce to rank 0" in d["config"]["parallelism"]
    assert d["collective"]["split"] is None and d["collective"]["timed_arm"] == "whole" and set(d["collective"]["arms"]) == {"whole"}


def test_bench_two_ranks_at_the_r2_shape():
    """BASELINE config 4's own workload shape on the one-GPU box: 200k voxels, 968x548x512 fp32 maps, views r::2 (16 per
    rank, 17.4 GB of maps each), one all-reduce of {sum f32 [200001,512], count} -- over gloo, both ranks on cuda:0.
    bench.py itself asserts that the reduced hit counts equal the sum of the ranks' single-rank totals EXACTLY and the
    reduced feature sums, per channel, the sum of the ranks' single-rank checksums; here additionally against a
    single-rank run of the same 32 views."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    # every run's pool holds all of its views (32 maps for the single rank, 16 per rank), so view v reads the map seeded by v in both
    common = ["--workload", "R2", "--views", "32", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline"]
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common, capture_output=True, text=True, timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = _last_json(r1.stdout)
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                         "--master-addr", "127.0.0.1", "--master-port", "29537", os.path.join(ROOT, "bench.py"),
                         "--gpus", "2", "--dist-backend", "gloo", "--single-device"] + common,
                        capture_output=True, text=True, timeout=900, env=env)
    assert r2.returncode == 0, r2.stderr[-3000:]
    two = _last_json(r2.stdout)
    assert two["n_gpus"] == 2 and two["config"]["workload"].startswith("R2: 200000 voxels x 32 views x 968x548x512")
    assert two["collective"]["op"] == "all-reduce" and two["collective"]["bytes_per_rank"] == 200001 * 512 * 4 + 2 * 200001 * 4
    # the scene the two ranks reduced IS the scene one rank projects: hit pixels exactly, channel checksum to fp32 rounding
    assert two["reduced_hit_pixels"] == one["hit_pixels_per_step"]
    assert abs(two["reduced_checksum"] - one["checksum"]) <= 1e-6 * one["checksum_abs"]


def _check_common(d):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    rf = d["roofline"]
    assert d["value"] > 0 and rf["bound"] in ("hbm", "l1_miss_queue") and rf["achieved"] > 0
    if rf["bound"] == "l1_miss_queue":
        # config 5 (no HBM roofline claim): the line says what the counters say bounds the kernel; its peak comes from the
        # committed counter pass of THIS build and is null for any other kernel sources; the HBM figure stays beside it
        assert abs(rf["hbm_frac"] - rf["achieved"] / rf["hbm_peak"]) < 1e-3
        assert (rf["peak"] is None and rf["frac"] is None) or abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    else:
        assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3


def test_bench_config2_r1_leg():
    # BASELINE config 2 at its own shape (80k voxels, 484x274x512), a 12-view slice of it to keep the test short
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "R1", "--views", "12", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_common(d)
    assert d["config"]["workload"].startswith("R1: 80000 voxels x 12 views x 484x274x512") and d["box_miss_voxels"] == 0


def test_bench_config5_rgb_leg():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "R4", "--views", "16", "--chunk", "8",
                        "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_common(d)
    assert d["config"]["workload"].startswith("R4: 500000 voxels x 16 views") and d["voxel_view_hits_per_step"] > 500000


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_bench_entry_point_leg(mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--entry", mode, "--views", "10", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_common(d)
    e = d["entry"]
    assert e["mode"] == mode and e["ms_per_view"] > 0 and e["dropin_ms_per_view"] > 0 and e["rows_out"] > 1000
    assert "R1 through the entry point" in d["config"]["workload"]


def test_bench_contiguous_allocation_option():
    # --alloc contiguous: resident buffers from hipExtMallocWithFlags(hipDeviceMallocContiguous), reported in the line
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "S0", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--alloc", "contiguous"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert set(d["pool_placement"]["allocation"].values()) <= {"contiguous", "default"}
    assert d["pool_placement"]["allocation"]["feature_pool"] == "contiguous" and d["value"] > 0


def _overlapped(d):
    """Phase 1 of call j+1 really ran UNDER the gather of call j: beside a gather the (throttled) march takes several times
    its solo time, so the sum of the phases' own durations exceeds the pass by far; when the two streams share a hardware
    queue the phases run one after the other and the pass IS their sum."""
    ph = d["phase_ms_per_step"]
    # judged on the MEDIAN step of the timed region (HIP events at the head of every step): one slow step of five -- a box hiccup --
    # does not decide, a lost overlap shows in every step; no second process is started (round 5 re-ran the bench once on failure,
    # which would have hidden an overlap lost in half of the processes)
    return d["step_ms"]["median"] < 0.9 * (ph["first_hit"] + ph["gather"])


def test_job_mode_overlap_survives_a_single_hardware_queue():
    """The runtime multiplexes streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues per priority level; with ONE queue
    a normal-priority side stream lands on the caller's queue and the march queues up behind the gather (R2 pass 64.8 ms
    instead of 52, profiles/r03_hw_queue_sharing.log).  The library's side stream has the device's highest priority: its
    queue comes from another pool, whatever the process created before."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "R1", "--steps", "5", "--warmup", "1",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["phase_ms_per_step"]["overlapped"] is True
    assert _overlapped(d), (d["ms_per_step"], d["step_ms"], d["phase_ms_per_step"])


def test_bench_multi_rank_path_over_a_one_rank_rccl_communicator():
    """`--rehearse-dist`: the N > 1 control flow of bench.py (the aggregator's add_views / add_final_views, collective inside
    the pass, exact verification of the reduced counts, both collective arms) with backend nccl = RCCL and ONE rank -- the only way RCCL can run this code on a one-GPU
    box.  RCCL initialised before the first pipelined call used to cost the march/gather overlap (63 vs 54 ms per R2
    pass): asserted here on the R1 workload."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "R1", "--steps", "5", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--rehearse-dist", "--min-calls", "2"],      # two calls: something to overlap
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 1 and d["collective"]["backend"] == "nccl" and d["collective"]["op"] == "all-reduce"
    assert d["collective"]["collective_ms_exposed"] >= 0 and set(d["collective"]["arms"]) == {"split", "whole"}
    cal = d["collective"]["calibration"]
    assert d["collective"]["timed_arm"] == cal["pick"] and set(cal["ms"]) == {"split", "whole"} and cal["settling_steps"]["split"] >= 2
    assert d["collective"]["timed_arm_chosen_by"] == cal["chosen_by"]
    assert d["reduced_hit_pixels"] == d["hit_pixels_per_step"]
    assert "rehearsal" in d["config"]["parallelism"] and "cpu_baseline" not in d
    assert _overlapped(d), (d["ms_per_step"], d["step_ms"], d["phase_ms_per_step"])
