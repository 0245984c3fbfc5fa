#!/usr/bin/env python3
"""Score call against align call on identical inputs, in one process (needs the GPU).

Three batches through the host API (sa_score_batch / sa_align_batch), the calls alternating so
both see the same machine state:

  sw20    1,000 x 1024^2 Smith-Waterman over 20 letters     (int32 kernels, record-free fill)
  lg20    1,000 x 1024^2 LocalGotoh over 20 letters          (int32 kernels, record-free fill)
  dna     10,000 x 4096^2 Smith-Waterman over DNA            (T16 / score-only fills, walks skipped)

Per batch and call kind: wall time per call (host clock around the blocking call: median, min,
max over --reps calls after --warmup), the run-to-run spread, fill launches per call, and -- in a
second pass with $SEQALIB_KERNEL_TIMING set -- the fill-kernel time (HIP events around the fill
launches alone).  The results of the two calls are compared on (score, end_i, end_j) at the sizes
timed.  Writes one JSON document (--out) and prints a table.

    python tools/score_bench.py --out profiles/score_bench.json
    python tools/score_bench.py --scale 0.1 --reps 2       # a quick rehearsal at a tenth of the pairs
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seqalib_amd as sa  # noqa: E402

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def letters_batch(seed, npairs, m, n):
    rng = np.random.default_rng(seed)
    s1 = AA[rng.integers(0, 20, npairs * m)]
    s2 = AA[rng.integers(0, 20, npairs * n)]
    # every fourth pair related (a copy with 15 % substitutions), so scores and end cells vary
    a = s1.reshape(npairs, m)
    b = s2.reshape(npairs, n)
    k = min(m, n)
    rel = np.arange(npairs) % 4 == 0
    keep = rng.random((int(rel.sum()), k)) >= 0.15
    b[rel, :k] = np.where(keep, a[rel, :k], b[rel, :k])
    o1 = np.arange(npairs + 1, dtype=np.uint64) * m
    o2 = np.arange(npairs + 1, dtype=np.uint64) * n
    return s1, o1, s2, o2


BATCHES = {
    "sw20": dict(algo=sa.SA_SW, scoring=(-1, 1, -1), npairs=1000, m=1024, n=1024, dna=False),
    "lg20": dict(algo=sa.SA_LOCAL_GOTOH, scoring=(-3, -1, 1, -1, True), npairs=1000, m=1024, n=1024, dna=False),
    "dna": dict(algo=sa.SA_SW, scoring=(-1, 1, -1), npairs=10000, m=4096, n=4096, dna=True),
}


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs),
                spread_pct=100.0 * (max(xs) - min(xs)) / statistics.median(xs), calls=len(xs))


def run_batch(eng, name, spec, reps, warmup, scale):
    npairs = max(1, int(round(spec["npairs"] * scale)))
    sc = sa.ScoringSystem(*spec["scoring"])
    if spec["dna"]:
        batch = sa.synth_dna_batch(4242, npairs, spec["m"], spec["n"], threads=16)
    else:
        batch = letters_batch(4242, npairs, spec["m"], spec["n"])
    out = None

    def align():
        nonlocal out
        res, ops = eng.align_packed(spec["algo"], sc, *batch, out=out)
        out = (res, ops)
        return res

    def score():
        return eng.score_packed(spec["algo"], sc, *batch)

    kinds = {"align": align, "score": score}
    wall = {k: [] for k in kinds}
    launches, plans, last = {}, {}, {}
    os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    for it in range(warmup + reps):
        for k, fn in kinds.items():   # alternating
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= warmup:
                wall[k].append(dt)
            launches[k] = eng.last_timings()[2]
            plans[k] = eng.last_plan_ex()
    same = all((last["align"][f] == last["score"][f]).all() for f in ("score", "end_i", "end_j"))
    # second pass: events around the fill kernels alone
    os.environ["SEQALIB_KERNEL_TIMING"] = "1"
    kern = {k: [] for k in kinds}
    stream = {k: [] for k in kinds}
    try:
        for it in range(1 + reps):
            for k, fn in kinds.items():
                fn()
                f, s = eng.last_kernel_timings()
                if it >= 1:
                    kern[k].append(f)
                    stream[k].append(s)
    finally:
        os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    doc = dict(batch=name, algo=sa.ALGO_NAMES[spec["algo"]], scoring=list(spec["scoring"]), npairs=npairs, m=spec["m"],
               n=spec["n"], alphabet="ACGT" if spec["dna"] else "20 letters", results_equal=bool(same))
    for k in kinds:
        doc[k] = dict(wall=stats(wall[k]), fill_kernel=stats(kern[k]), fill_stream=stats(stream[k]),
                      fill_launches_per_call=launches[k],
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    a, s = doc["align"], doc["score"]
    doc["score_over_align_wall"] = s["wall"]["median_ms"] / a["wall"]["median_ms"]
    doc["score_over_align_fill_kernel"] = s["fill_kernel"]["median_ms"] / a["fill_kernel"]["median_ms"]
    # the one condition: the score call is not slower than the align call beyond the align call's own spread
    doc["score_not_slower"] = s["wall"]["median_ms"] <= a["wall"]["max_ms"]
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--batches", default="sw20,lg20,dna")
    args = ap.parse_args()
    eng = sa.Engine(0)
    docs = []
    for name in args.batches.split(","):
        doc = run_batch(eng, name, BATCHES[name], args.reps, args.warmup, args.scale)
        docs.append(doc)
        a, s = doc["align"], doc["score"]
        print(f"{name:5s} {doc['npairs']:6d} x {doc['m']}x{doc['n']}  wall ms: align {a['wall']['median_ms']:9.3f} "
              f"[{a['wall']['min_ms']:.3f}, {a['wall']['max_ms']:.3f}]  score {s['wall']['median_ms']:9.3f} "
              f"[{s['wall']['min_ms']:.3f}, {s['wall']['max_ms']:.3f}]  fill kernel ms: align {a['fill_kernel']['median_ms']:.3f} "
              f"score {s['fill_kernel']['median_ms']:.3f}  launches {a['fill_launches_per_call']}/{s['fill_launches_per_call']}  "
              f"records {a['plan']['records']}/{s['plan']['records']}  equal {doc['results_equal']}", flush=True)
    eng.close()
    result = dict(tool="tools/score_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale, batches=docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0 if all(d["results_equal"] for d in docs) else 1


if __name__ == "__main__":
    sys.exit(main())
