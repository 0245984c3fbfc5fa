#!/usr/bin/env python3
"""The ends-free banded calls against the banded global calls on identical inputs, in one process
(needs the GPU).

Two DNA batches, NW and GlobalGotoh, through the host API, the sides alternating so all see the same
machine state, each side on a context of its own:

  fit      2,000 pairs, a 150-symbol read (3 % substitutions) somewhere in a 1000-symbol window, w = 16,
           SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END
  overlap  2,000 pairs of 2000 x 2000, Seq2 = Seq1 shifted by up to 60 symbols (3 % substitutions), w = 64,
           SA_FREE_SEQ1_BEGIN | SA_FREE_SEQ2_END

  free   sa_align_batch_banded_ends_free of this tree with the flags above
  free0  the same call with free_ends = 0 (results and ops must equal base's)
  base   sa_align_batch_banded / _banded_affine with SA_NW / SA_GLOBAL_GOTOH, on this tree or -- with
         --base-lib PATH -- on another build of the engine (the parent commit's libseqalib_hip.so)
         loaded beside this one

Per row and side: fill and walk kernel time (sa_last_timings: median, min, max over --reps calls after
--warmup) and wall time per call (host clock around the blocking call).  fill_ratio_base_over_free is
base's median fill time over free's: below 1 the ends-free fill is the slower one.  Writes one JSON
document (--out) and prints a table.

    python tools/banded_free_bench.py --base-lib parent/libseqalib_hip.so --out profiles/banded_free_bench.json
    python tools/banded_free_bench.py --scale 0.05 --reps 2      # a quick rehearsal
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import seqalib_amd as sa  # noqa: E402
from banded_bench import ACGT, band_cells, stats  # noqa: E402
from banded_matrix_bench import OtherBandedEngine  # noqa: E402

ALGOS = {"nw": (sa.SA_NW, (-2, 2, -3)), "gg": (sa.SA_GLOBAL_GOTOH, (-3, -1, 2, -3))}
FIT = sa.SA_FREE_SEQ2_BEGIN | sa.SA_FREE_SEQ2_END
OVERLAP = sa.SA_FREE_SEQ1_BEGIN | sa.SA_FREE_SEQ2_END


def substituted(rng, s, percent=3):
    hit = rng.integers(0, 100, s.shape) < percent
    return np.where(hit, ACGT[rng.integers(0, 4, s.shape)], s)


def fit_batch(seed, npairs, read=150, window=1000):
    rng = np.random.default_rng(seed)
    win = ACGT[rng.integers(0, 4, (npairs, window))]
    off = rng.integers(0, window - read + 1, npairs)
    reads = substituted(rng, np.stack([win[p, off[p]:off[p] + read] for p in range(npairs)]))
    o1 = np.arange(npairs + 1, dtype=np.uint64) * read
    o2 = np.arange(npairs + 1, dtype=np.uint64) * window
    return np.ascontiguousarray(reads.reshape(-1)), o1, np.ascontiguousarray(win.reshape(-1)), o2


def overlap_batch(seed, npairs, length=2000, max_shift=60):
    rng = np.random.default_rng(seed)
    s1 = ACGT[rng.integers(0, 4, (npairs, length))]
    tail = ACGT[rng.integers(0, 4, (npairs, length))]
    shift = rng.integers(0, max_shift + 1, npairs)
    s2 = substituted(rng, np.stack([np.concatenate([s1[p, shift[p]:], tail[p, :shift[p]]]) for p in range(npairs)]))
    o = np.arange(npairs + 1, dtype=np.uint64) * length
    return np.ascontiguousarray(s1.reshape(-1)), o, np.ascontiguousarray(s2.reshape(-1)), o.copy()


CASES = {"fit": dict(npairs=2000, make=fit_batch, w=16, free_ends=FIT, shape="150 in 1000"),
         "overlap": dict(npairs=2000, make=overlap_batch, w=64, free_ends=OVERLAP, shape="2000 x 2000")}


def run_row(engines, name, batch, w, free_ends, reps, warmup):
    algo, args = ALGOS[name]
    sc = sa.ScoringSystem(*args)
    base_call = engines["base"].align_banded_affine_packed if algo == sa.SA_GLOBAL_GOTOH else engines["base"].align_banded_packed
    kinds = {"free": lambda: engines["free"].align_banded_ends_free_packed(algo, sc, *batch, w, free_ends),
             "free0": lambda: engines["free0"].align_banded_ends_free_packed(algo, sc, *batch, w, 0),
             "base": lambda: base_call(algo, sc, *batch, w)}
    wall = {k: [] for k in kinds}
    fill = {k: [] for k in kinds}
    walk = {k: [] for k in kinds}
    last, plans, launches = {}, {}, {}
    for it in range(warmup + reps):
        for k, fn in kinds.items():   # alternating
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            f, t, nl = engines[k].last_timings()
            if it >= warmup:
                wall[k].append(dt)
                fill[k].append(f)
                walk[k].append(t)
            launches[k] = nl
            plans[k] = engines[k].last_plan_ex()
    cells, bmax, full_cells = band_cells(batch[1], batch[3], w)
    (fres, _), (zres, zops), (bres, bops) = last["free"], last["free0"], last["base"]
    doc = dict(algo=sa.ALGO_NAMES[algo], scoring=list(args), w=w, free_ends=free_ends, B_max=bmax, in_band_cells=cells,
               full_cells=full_cells, free0_results_equal_base=bool((zres == bres).all()),
               free0_ops_equal_base=bool(np.array_equal(zops, bops)),
               free_scores_not_below_base=bool((fres["score"] >= bres["score"]).all()),
               free_scores_above_base=int((fres["score"] > bres["score"]).sum()))
    for k in kinds:
        doc[k] = dict(fill=stats(fill[k]), walk=stats(walk[k]), wall=stats(wall[k]), fill_launches_per_call=launches[k],
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    doc["fill_ratio_base_over_free"] = doc["base"]["fill"]["median_ms"] / doc["free"]["fill"]["median_ms"]
    doc["fill_ratio_base_over_free0"] = doc["base"]["fill"]["median_ms"] / doc["free0"]["fill"]["median_ms"]
    doc["wall_ratio_base_over_free"] = doc["base"]["wall"]["median_ms"] / doc["free"]["wall"]["median_ms"]
    doc["free_fill_cells_per_s"] = cells / (doc["free"]["fill"]["median_ms"] * 1e-3)
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--cases", default="fit,overlap")
    ap.add_argument("--algos", default="nw,gg")
    ap.add_argument("--base-lib", default=None, help="another build of libseqalib_hip.so for the banded global side")
    args = ap.parse_args()
    # every side has a context (workspace, I/O cache) of its own
    engines = {"free": sa.Engine(0), "free0": sa.Engine(0),
               "base": OtherBandedEngine(args.base_lib) if args.base_lib else sa.Engine(0)}
    rows = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/banded_free_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale,
                               base_side="other build" if args.base_lib else "this build", rows=rows), fh, indent=1)
                fh.write("\n")

    for case in args.cases.split(","):
        spec = CASES[case]
        npairs = max(1, int(round(spec["npairs"] * args.scale)))
        batch = spec["make"](99, npairs)
        for name in args.algos.split(","):
            doc = run_row(engines, name, batch, spec["w"], spec["free_ends"], args.reps, args.warmup)
            doc.update(case=case, shape=f"{npairs} x {spec['shape']}", alphabet="ACGT")
            rows.append(doc)
            write()   # (after every row: a run that is cut short keeps what it measured)
            f, z, b = doc["free"], doc["free0"], doc["base"]
            print(f"{case:>8s} {doc['shape']:>20s} {name} w {spec['w']:3d} B<={doc['B_max']:4d} R {f['plan']['R']:2d}  fill ms: free "
                  f"{f['fill']['median_ms']:.3f} [{f['fill']['min_ms']:.3f}, {f['fill']['max_ms']:.3f}] free0 {z['fill']['median_ms']:.3f} "
                  f"[{z['fill']['min_ms']:.3f}, {z['fill']['max_ms']:.3f}] base {b['fill']['median_ms']:.3f} [{b['fill']['min_ms']:.3f}, "
                  f"{b['fill']['max_ms']:.3f}] base/free {doc['fill_ratio_base_over_free']:.3f} base/free0 "
                  f"{doc['fill_ratio_base_over_free0']:.3f}  walk ms {f['walk']['median_ms']:.3f}/{b['walk']['median_ms']:.3f}  wall ms "
                  f"{f['wall']['median_ms']:.2f}/{b['wall']['median_ms']:.2f}  free0 == base {doc['free0_results_equal_base']}/"
                  f"{doc['free0_ops_equal_base']}  freed scores above base {doc['free_scores_above_base']}/{npairs}", flush=True)
    for k in ("free", "free0") + (() if args.base_lib else ("base",)):
        engines[k].close()
    write()
    ok = all(r["free0_results_equal_base"] and r["free0_ops_equal_base"] and r["free_scores_not_below_base"] for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
