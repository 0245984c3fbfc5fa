#!/usr/bin/env python3
"""Banded call against the full call on identical inputs, in one process (needs the GPU).

Related pairs (the mutation model of sa_synth_mutate: 10 % substitutions, 2 % insertions, 2 %
deletions), over DNA and over 20 letters, through the host API, the banded and the full call
alternating so both see the same machine state:

  4096    1,000 x 4096^2  NW and SW at w = 16, 64, 256
  16384     200 x 16384^2 NW and SW at w = 64, 256

--algos gg,lg runs the affine rows instead (GlobalGotoh / LocalGotoh, scoring (-3, -1, 1, -1), the banded
affine calls against the full affine calls, w = 16, 64, 256 at both sizes; profiles/banded_affine_bench.json).

The full side is sa_align_batch; where that call cannot hold its records it is sa_score_batch (and
the banded side sa_score_batch_banded), which the row says.  Per row: wall time per call (host
clock around the blocking call: median, min, max over --reps calls after --warmup), fill and walk
kernel time of the banded call (sa_last_timings), and -- in a second pass with
$SEQALIB_KERNEL_TIMING set -- the fill kernels alone of both calls.  From these: the in-band cells
per second of the banded fill and the speed-up over the full call.  Writes one JSON document
(--out) and prints a table.

    python tools/banded_bench.py --out profiles/banded_bench.json
    python tools/banded_bench.py --scale 0.05 --reps 2      # a quick rehearsal
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
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def related_batch(seed, npairs, length, alphabet):
    """npairs x (random sequence of `length`, its mutated copy), packed."""
    rng = np.random.default_rng(seed)
    k = len(alphabet)
    src = alphabet[rng.integers(0, k, (npairs, length))]
    r = rng.integers(0, 100, (npairs, length))
    fresh = alphabet[rng.integers(0, k, (npairs, length))]
    count = np.where(r < 10, 1, np.where(r < 12, 2, np.where(r < 14, 0, 1)))
    s2, o2 = [], np.zeros(npairs + 1, dtype=np.uint64)
    for p in range(npairs):
        c = count[p]
        out = np.repeat(src[p], c)
        first = np.cumsum(c) - c            # where each position's output starts
        sub = r[p] < 12                     # substituted, or a fresh symbol inserted before the copy
        out[first[sub]] = fresh[p][sub]
        s2.append(out)
        o2[p + 1] = o2[p] + len(out)
    o1 = np.arange(npairs + 1, dtype=np.uint64) * length
    return np.ascontiguousarray(src.reshape(-1)), o1, np.concatenate(s2), o2


def band_cells(o1, o2, w):
    m = np.diff(o1).astype(np.int64)
    n = np.diff(o2).astype(np.int64)
    total, bmax = 0, 0
    for mm, nn in zip(m, n):
        lo, hi = min(0, nn - mm) - w, max(0, nn - mm) + w
        i = np.arange(mm + 1)
        total += int((np.minimum(nn, i + hi) - np.maximum(0, i + lo) + 1).sum())
        bmax = max(bmax, hi - lo + 1)
    return total, int(bmax), int((m * n).sum())


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), calls=len(xs))


def run_row(eng, algo, batch, w, reps, warmup):
    affine = algo in (sa.SA_GLOBAL_GOTOH, sa.SA_LOCAL_GOTOH)
    sc = sa.ScoringSystem(-3, -1, 1, -1) if affine else sa.ScoringSystem(-1, 1, -1)
    align_banded = eng.align_banded_affine_packed if affine else eng.align_banded_packed
    score_banded = eng.score_banded_affine_packed if affine else eng.score_banded_packed
    mode = "align"
    try:
        eng.align_packed(algo, sc, *batch)
    except sa.SeqalibError:
        mode = "score"   # the full align call cannot hold its records

    def full():
        return eng.align_packed(algo, sc, *batch)[0] if mode == "align" else eng.score_packed(algo, sc, *batch)

    def banded():
        if mode == "align":
            return align_banded(algo, sc, *batch, w)[0]
        return score_banded(algo, sc, *batch, w)

    kinds = {"banded": banded, "full": full}
    wall = {k: [] for k in kinds}
    dev = {k: [] for k in kinds}
    last, plans, launches = {}, {}, {}
    os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    for it in range(warmup + reps):
        for k, fn in kinds.items():   # alternating
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            f, t, nl = eng.last_timings()
            if it >= warmup:
                wall[k].append(dt)
                dev[k].append((f, t))
            launches[k] = nl
            plans[k] = eng.last_plan_ex()
    os.environ["SEQALIB_KERNEL_TIMING"] = "1"
    kern = {k: [] for k in kinds}
    try:
        for it in range(1 + reps):
            for k, fn in kinds.items():
                fn()
                if it >= 1:
                    kern[k].append(eng.last_kernel_timings()[0])
    finally:
        os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    cells, bmax, full_cells = band_cells(batch[1], batch[3], w)
    doc = dict(algo=sa.ALGO_NAMES[algo], w=w, B_max=bmax, calls=mode, in_band_cells=cells, full_cells=full_cells,
               scores_equal=int((last["banded"]["score"] == last["full"]["score"]).sum()),
               scores_not_above=bool((last["banded"]["score"] <= last["full"]["score"]).all()))
    for k in kinds:
        doc[k] = dict(wall=stats(wall[k]), fill_kernel=stats(kern[k]),
                      fill_ms=statistics.median(x[0] for x in dev[k]), walk_ms=statistics.median(x[1] for x in dev[k]),
                      fill_launches_per_call=launches[k],
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    b, f = doc["banded"], doc["full"]
    doc["banded_fill_cells_per_s"] = cells / (b["fill_kernel"]["median_ms"] * 1e-3)
    doc["full_fill_cells_per_s"] = full_cells / (f["fill_kernel"]["median_ms"] * 1e-3)
    doc["speedup_wall"] = f["wall"]["median_ms"] / b["wall"]["median_ms"]
    doc["speedup_fill_kernel"] = f["fill_kernel"]["median_ms"] / b["fill_kernel"]["median_ms"]
    # in-band cells per second at which the banded fill kernel would equal the full call's fill kernel
    doc["break_even_cells_per_s"] = cells / (f["fill_kernel"]["median_ms"] * 1e-3)
    return doc


SHAPES = {"4096": dict(npairs=1000, length=4096, ws=(16, 64, 256)),
          "16384": dict(npairs=200, length=16384, ws=(64, 256), affine_ws=(16, 64, 256))}
ALGOS = {"nw": sa.SA_NW, "sw": sa.SA_SW, "gg": sa.SA_GLOBAL_GOTOH, "lg": sa.SA_LOCAL_GOTOH}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--shapes", default="4096,16384")
    ap.add_argument("--alphabets", default="dna,aa")
    ap.add_argument("--algos", default="nw,sw")
    args = ap.parse_args()
    eng = sa.Engine(0)
    rows = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/banded_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale, rows=rows),
                          fh, indent=1)
                fh.write("\n")

    for shape in args.shapes.split(","):
        spec = SHAPES[shape]
        npairs = max(1, int(round(spec["npairs"] * args.scale)))
        for alpha in args.alphabets.split(","):
            batch = related_batch(99, npairs, spec["length"], ACGT if alpha == "dna" else AA)
            for an in args.algos.split(","):
                algo = ALGOS[an]
                for w in (spec.get("affine_ws", spec["ws"]) if an in ("gg", "lg") else spec["ws"]):
                    doc = run_row(eng, algo, batch, w, args.reps, args.warmup)
                    doc.update(shape=f"{npairs} x {spec['length']}^2", alphabet="ACGT" if alpha == "dna" else "20 letters")
                    rows.append(doc)
                    write()   # (after every row: a long run that is cut short keeps what it measured)
                    b, f = doc["banded"], doc["full"]
                    print(f"{doc['shape']:>16s} {alpha:3s} {an} w {w:3d} B<={doc['B_max']:4d} {doc['calls']:5s}  wall ms: banded "
                          f"{b['wall']['median_ms']:8.2f} [{b['wall']['min_ms']:.2f}, {b['wall']['max_ms']:.2f}] full "
                          f"{f['wall']['median_ms']:8.2f} [{f['wall']['min_ms']:.2f}, {f['wall']['max_ms']:.2f}] x{doc['speedup_wall']:.2f}"
                          f"  fill kernel ms: banded {b['fill_kernel']['median_ms']:.3f} full {f['fill_kernel']['median_ms']:.3f} "
                          f"x{doc['speedup_fill_kernel']:.2f}  walk ms {b['walk_ms']:.2f}/{f['walk_ms']:.2f}  banded GCUPS "
                          f"{doc['banded_fill_cells_per_s'] / 1e9:.1f} (break-even {doc['break_even_cells_per_s'] / 1e9:.1f})  "
                          f"R {b['plan']['R']}  equal {doc['scores_equal']}/{npairs}", flush=True)
    eng.close()
    write()
    return 0 if all(r["scores_not_above"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
