"""bench.py's plain run, --full and --dump-outputs.

CPU: dump_outputs on the oracle's results of a small batch (layout, the
defined core entries, the size cap and its fixed sample) and the argument
checks.  GPU: a plain run times exactly --steps steps, carries none of
--full's legs and dumps what the oracle computes for the same batch; a --full
run of the same arguments carries the legs and dumps the same arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300
FULL_ONLY = ("deterministic", "host_lowering_res_per_s", "end_to_end", "end_to_end_device", "solve_batch_api",
             "kernel_only", "roofline", "latency", "cpu_baseline", "verified_bit_exact_vs_oracle", "inproc")


@pytest.fixture(scope="module")
def batch():
    """bench.py --problems N's batch (config 2, default seed) and the oracle's results for it."""
    _, lw32, _, _ = bench.lowered_config(2, N, 1000, "packed", True)
    return oracle.solve_batch(lw32.rec_off, lw32.rec, 0, 2)


def defined_core(o, n):
    return np.concatenate([o["core"][int(o["core_off"][p]):int(o["core_off"][p]) + int(o["core_len"][p])]
                           for p in range(n)] + [np.zeros(0, np.int32)])


def check_dump(d, o, n):
    """The files of a dump directory against a result dict."""
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in bench.DUMP_KEYS)
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in bench.DUMP_KEYS}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
    for k in ("status", "flags", "core_len", "steps"):
        assert np.array_equal(got[k], o[k][:n].astype(np.float64)), k
    for k in ("installed", "inst_off", "core_off"):
        assert np.array_equal(got[k], o[k].astype(np.float64)), k
    assert np.array_equal(got["core"], defined_core(o, n).astype(np.float64))
    return got


def test_dump_outputs_layout(batch, tmp_path):
    o = {k: v.copy() for k, v in batch.items()}
    assert o["core_len"].sum() > 0 and (o["core_len"] == 0).any()  # (both kinds of problem in the batch)
    # words behind a problem's core are not part of the result: poison them
    poisoned = dict(o, core=o["core"].copy())
    for p in range(N):
        poisoned["core"][int(o["core_off"][p]) + int(o["core_len"][p]):int(o["core_off"][p + 1])] = -7
    bench.dump_outputs(str(tmp_path / "a"), poisoned, N)
    check_dump(str(tmp_path / "a"), o, N)
    # rank suffix
    bench.dump_outputs(str(tmp_path / "b"), o, N, ".rank1")
    assert sorted(os.listdir(tmp_path / "b")) == sorted(k + ".rank1.npy" for k in bench.DUMP_KEYS)


def test_dump_outputs_cap_is_a_fixed_sample(batch, tmp_path):
    cap = 8 * len(bench.DUMP_KEYS) * 100  # 100 elements per array
    a = bench.dump_outputs(str(tmp_path / "a"), batch, N, max_bytes=cap)
    b = bench.dump_outputs(str(tmp_path / "b"), batch, N, max_bytes=cap)
    total = 0
    for k in bench.DUMP_KEYS:
        x, y = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(x, y) and np.array_equal(x, a[k]) and np.array_equal(y, b[k])
        assert len(x) <= 100
        total += x.nbytes
    assert total <= cap
    # the sample is elements of the array in their order: N problems' steps, 100 of them
    steps = np.load(tmp_path / "a" / "steps.npy")
    idx = np.sort(np.random.default_rng(0).choice(N, 100, replace=False))
    assert np.array_equal(steps, batch["steps"][:N][idx].astype(np.float64))


def _bench(*args):
    return subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_kernel_only_is_a_full_leg():
    r = _bench("--kernel-only")
    assert r.returncode != 0 and "--full" in r.stderr
    r = _bench("--full", "--kernel-only", "--dump-outputs", "x")
    assert r.returncode != 0 and "--dump-outputs" in r.stderr


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_oracles_results(batch, tmp_path):
    # (2 jobs in flight: --full's determinism check reads every job's result buffer, so each must be used)
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--problems", str(N), "--depth", "2"]
    r = _bench(*common, "--dump-outputs", str(tmp_path / "plain"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "resolutions/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["metric"] == bench.METRIC and line["ms_per_step"] > 0
    # value is the batch over the step time (ms_per_step is rounded to 4 decimals, value to 1)
    rel = 5e-5 / line["ms_per_step"] + 0.05 / line["value"] + 1e-9
    assert abs(line["value"] - N / (line["ms_per_step"] * 1e-3)) <= 1.01 * rel * line["value"]
    assert not [k for k in FULL_ONLY if k in line]
    plain = check_dump(str(tmp_path / "plain"), batch, N)

    r = _bench(*common, "--full", "--cpu-seconds", "0.2", "--kernel-steps", "2", "--e2e-steps", "2",
               "--dump-outputs", str(tmp_path / "full"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["full"] is True
    assert [k for k in FULL_ONLY if k not in line] == ["inproc"]
    assert line["deterministic"] is True and line["verified_bit_exact_vs_oracle"] is True
    assert line["kernel_only"]["identical_to_host_path"] is True
    assert line["end_to_end_device"]["records_equal_host_lowering"] is True
    full = check_dump(str(tmp_path / "full"), batch, N)
    assert all(np.array_equal(plain[k], full[k]) for k in bench.DUMP_KEYS)
