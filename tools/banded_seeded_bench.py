#!/usr/bin/env python3
"""The seeded banded calls against the ends-free banded calls on identical pairs, in one process (needs
the GPU).

Three DNA batches, NW and GlobalGotoh, through the host API, the two sides alternating so both see the
same machine state, each side on a context of its own:

  fit      2,000 pairs, a 150-symbol read (3 % substitutions) somewhere in a 1000-symbol window,
           SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END; seeded at the planted diagonal, w = 16; base w = 16
  contig   the same, the windows 100,000 symbols long (the corridor band would be 99,883 diagonals wide:
           the base side refuses the batch, which is recorded)
  overlap  2,000 pairs of 2000 x 2000, Seq2 = Seq1 shifted by up to 60 symbols (3 % substitutions),
           SA_FREE_SEQ1_BEGIN | SA_FREE_SEQ2_END; seeded at minus the shift, w = 16; base w = 64 (the
           corridor band that holds every shift)

  seeded  sa_align_batch_banded_seeded of this tree
  base    sa_align_batch_banded_ends_free, on this tree or -- with --base-lib PATH -- on another build of
          the engine (the parent commit's libseqalib_hip.so) loaded beside this one

Per row and side: fill and walk kernel time (sa_last_timings: median, min, max over --reps calls after
--warmup) and wall time per call (host clock around the blocking call).  fill_ratio_base_over_seeded is
base's median fill time over seeded's: above 1 the seeded fill is the faster one.  Writes one JSON
document (--out) and prints a table.

    python tools/banded_seeded_bench.py --base-lib parent/libseqalib_hip.so --out profiles/banded_seeded_bench.json
    python tools/banded_seeded_bench.py --scale 0.05 --reps 2      # a quick rehearsal
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import seqalib_amd as sa  # noqa: E402
from banded_bench import ACGT, stats  # noqa: E402
from banded_free_bench import FIT, OVERLAP, substituted  # noqa: E402
from submat_bench import OtherEngine  # noqa: E402

ALGOS = {"nw": (sa.SA_NW, (-2, 2, -3)), "gg": (sa.SA_GLOBAL_GOTOH, (-3, -1, 2, -3))}


class OtherEndsFreeEngine(OtherEngine):
    """OtherEngine with the ends-free banded call declared."""

    def __init__(self, path, device=0):
        super().__init__(path, device)
        vp = C.c_void_p
        self.L.sa_align_batch_banded_ends_free.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32,
                                                           C.c_uint32, vp, vp, C.c_uint64]


def fit_batch(seed, npairs, read=150, window=1000):
    """(s1, o1, s2, o2, diag): diag[p] is the window position the read was taken from."""
    rng = np.random.default_rng(seed)
    win = ACGT[rng.integers(0, 4, (npairs, window), dtype=np.uint8)]
    off = rng.integers(0, window - read + 1, npairs)
    reads = substituted(rng, np.stack([win[p, off[p]:off[p] + read] for p in range(npairs)]))
    o1 = np.arange(npairs + 1, dtype=np.uint64) * read
    o2 = np.arange(npairs + 1, dtype=np.uint64) * window
    return np.ascontiguousarray(reads.reshape(-1)), o1, np.ascontiguousarray(win.reshape(-1)), o2, off.astype(np.int32)


def contig_batch(seed, npairs):
    return fit_batch(seed, npairs, window=100000)


def overlap_batch(seed, npairs, length=2000, max_shift=60):
    rng = np.random.default_rng(seed)
    s1 = ACGT[rng.integers(0, 4, (npairs, length))]
    tail = ACGT[rng.integers(0, 4, (npairs, length))]
    shift = rng.integers(0, max_shift + 1, npairs)
    s2 = substituted(rng, np.stack([np.concatenate([s1[p, shift[p]:], tail[p, :shift[p]]]) for p in range(npairs)]))
    o = np.arange(npairs + 1, dtype=np.uint64) * length
    return np.ascontiguousarray(s1.reshape(-1)), o, np.ascontiguousarray(s2.reshape(-1)), o.copy(), (-shift).astype(np.int32)


CASES = {"fit": dict(npairs=2000, make=fit_batch, w=16, base_w=16, free_ends=FIT, shape="150 in 1000"),
         "contig": dict(npairs=2000, make=contig_batch, w=16, base_w=16, free_ends=FIT, shape="150 in 100000"),
         "overlap": dict(npairs=2000, make=overlap_batch, w=16, base_w=64, free_ends=OVERLAP, shape="2000 x 2000")}


def seeded_cells(o1, o2, diag, w):
    """(in-band cells, widest clipped band) of the batch."""
    m = np.diff(o1).astype(np.int64)
    n = np.diff(o2).astype(np.int64)
    total, bmax = 0, 0
    for mm, nn, k in zip(m, n, diag.astype(np.int64)):
        lo, hi = max(k - w, -mm), min(k + w, nn)
        i = np.arange(max(0, -hi), min(mm, nn - lo) + 1)
        total += int((np.minimum(nn, i + hi) - np.maximum(0, i + lo) + 1).sum())
        bmax = max(bmax, hi - lo + 1)
    return total, int(bmax)


def run_row(engines, name, batch, spec, reps, warmup):
    algo, args = ALGOS[name]
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2, diag = batch
    w, base_w, fe = spec["w"], spec["base_w"], spec["free_ends"]
    kinds = {"seeded": lambda: engines["seeded"].align_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diag, w, fe),
             "base": lambda: engines["base"].align_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, base_w, fe)}
    refused = None
    try:
        kinds["base"]()
    except sa.SeqalibError as e:   # the corridor band does not hold this shape
        refused = str(e)
        del kinds["base"]
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
    cells, bmax = seeded_cells(o1, o2, diag, w)
    doc = dict(algo=sa.ALGO_NAMES[algo], scoring=list(args), w=w, base_w=base_w, free_ends=fe, B_max=bmax, in_band_cells=cells,
               base_refused=refused)
    for k in kinds:
        doc[k] = dict(fill=stats(fill[k]), walk=stats(walk[k]), wall=stats(wall[k]), fill_launches_per_call=launches[k],
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    doc["seeded_fill_cells_per_s"] = cells / (doc["seeded"]["fill"]["median_ms"] * 1e-3)
    if refused is None:
        sres, bres = last["seeded"][0], last["base"][0]
        doc["scores_equal_base"] = int((sres["score"] == bres["score"]).sum())
        doc["scores_below_base"] = int((sres["score"] < bres["score"]).sum())
        doc["fill_ratio_base_over_seeded"] = doc["base"]["fill"]["median_ms"] / doc["seeded"]["fill"]["median_ms"]
        doc["wall_ratio_base_over_seeded"] = doc["base"]["wall"]["median_ms"] / doc["seeded"]["wall"]["median_ms"]
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--cases", default="fit,contig,overlap")
    ap.add_argument("--algos", default="nw,gg")
    ap.add_argument("--base-lib", default=None, help="another build of libseqalib_hip.so for the ends-free side")
    args = ap.parse_args()
    # every side has a context (workspace, I/O cache) of its own
    engines = {"seeded": sa.Engine(0), "base": OtherEndsFreeEngine(args.base_lib) if args.base_lib else sa.Engine(0)}
    rows = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/banded_seeded_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale,
                               base_side="other build" if args.base_lib else "this build", rows=rows), fh, indent=1)
                fh.write("\n")

    for case in args.cases.split(","):
        spec = CASES[case]
        npairs = max(1, int(round(spec["npairs"] * args.scale)))
        batch = spec["make"](99, npairs)
        for name in args.algos.split(","):
            doc = run_row(engines, name, batch, spec, args.reps, args.warmup)
            doc.update(case=case, shape=f"{npairs} x {spec['shape']}", alphabet="ACGT")
            rows.append(doc)
            write()   # (after every row: a run that is cut short keeps what it measured)
            s = doc["seeded"]
            line = (f"{case:>8s} {doc['shape']:>22s} {name} w {spec['w']:3d} B<={doc['B_max']:4d} R {s['plan']['R']:2d}  fill ms: seeded "
                    f"{s['fill']['median_ms']:.3f} [{s['fill']['min_ms']:.3f}, {s['fill']['max_ms']:.3f}]")
            if doc["base_refused"] is None:
                b = doc["base"]
                line += (f" base (w {spec['base_w']}, R {b['plan']['R']}) {b['fill']['median_ms']:.3f} [{b['fill']['min_ms']:.3f}, "
                         f"{b['fill']['max_ms']:.3f}] base/seeded {doc['fill_ratio_base_over_seeded']:.2f}  walk ms "
                         f"{s['walk']['median_ms']:.3f}/{b['walk']['median_ms']:.3f}  wall ms {s['wall']['median_ms']:.2f}/"
                         f"{b['wall']['median_ms']:.2f}  scores equal {doc['scores_equal_base']}/{npairs} below {doc['scores_below_base']}")
            else:
                line += f" base refused  walk ms {s['walk']['median_ms']:.3f}  wall ms {s['wall']['median_ms']:.2f}"
            print(line, flush=True)
    engines["seeded"].close()
    if not args.base_lib:
        engines["base"].close()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
