"""bench.py's own options on one GPU: a plain run stops after the timed steps, `--dump-outputs`
writes what the last timed step computed, and `--full` adds the other legs.  One small batch
(40 pairs of 600 x 600, two fill bands) keeps each run to the start-up of a Python process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS, LEN = 40, 600
FULL_ONLY = ("roofline", "serial_ms_per_step", "e2e_ms_per_step", "parity", "parity_exact", "configs", "dropin_e2e",
             "dropin_single_call", "cpu_baseline")


def run_bench(extra, steps=3):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--pairs", str(PAIRS), "--len", str(LEN), "--steps", str(steps),
           "--warmup", "1"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import bench
    import seqalib_amd as sa
    from util import linear_rescore, oracle_sw_scores
    line = run_bench(["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GCUPS" and line["higher_is_better"] is True and line["value"] > 0
    # ms_per_step is the time of one timed step: the value's own time per step, to its two decimals
    assert abs(PAIRS * LEN * LEN / line["value"] / 1e6 - line["ms_per_step"]) < 0.006 + 1e-4 * line["ms_per_step"]
    assert not [k for k in FULL_ONLY if k in line]
    # another number of steps ends in the other output set: the same files
    run_bench(["--dump-outputs", str(tmp_path / "b")], steps=2)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ops_sample.npy", "ops_sample_pairs.npy", "results.npy"] == sorted(os.listdir(tmp_path / "b"))
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n)), n
    res, idx, ops = a["results.npy"], a["ops_sample_pairs.npy"], a["ops_sample.npy"]
    assert res.dtype == np.float64 and res.shape == (PAIRS, len(bench.DUMP_FIELDS))
    assert ops.dtype == np.float32 and ops.shape == (PAIRS, 2 * LEN + 1) and list(idx) == list(range(PAIRS))
    # the dumped batch is the seeded one, and what was dumped is the alignment of each pair
    s1, o1, s2, o2 = sa.synth_dna_batch(bench.SEED_BASE, PAIRS, LEN, LEN, threads=2)
    assert np.array_equal(res[:, :3], oracle_sw_scores(bench.SCORING, s1, o1, s2, o2, threads=4))
    assert not res[:, bench.DUMP_FIELDS.index("flags")].any()
    nops = res[:, bench.DUMP_FIELDS.index("nops")].astype(np.int64)
    assert np.array_equal(np.count_nonzero(ops, axis=1), nops)
    packed = np.zeros(int(o1[-1] + o2[-1]) + PAIRS, dtype=np.uint8)
    for p in range(PAIRS):
        off = int(o1[p] + o2[p]) + p
        packed[off:off + nops[p]] = ops[p, :nops[p]]
    rec = np.zeros(PAIRS, dtype=sa.RESULT_DTYPE)
    rec["nops"] = nops
    assert np.array_equal(linear_rescore(bench.SCORING, rec, packed, o1, o2), res[:, 0])


def test_full_run_adds_the_other_legs():
    line = run_bench(["--full", "--configs", "", "--cpu-pairs", "8", "--cpu-pairs-1t", "2", "--dropin-pairs", "40",
                      "--dropin-reps", "1", "--latency-reps", "5", "--e2e-steps", "1", "--serial-steps", "1"])
    assert line["full"] is True and line["parity_exact"] is True
    assert not [k for k in FULL_ONLY if k not in line]
    assert line["roofline"]["bound"] == "valu" and line["e2e_ms_per_step"] > 0 and line["serial_ms_per_step"] > 0
    assert line["cpu_baseline"]["value"] > 0 and "error" not in line["dropin_e2e"]
