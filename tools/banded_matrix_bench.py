#!/usr/bin/env python3
"""The banded matrix call against (a) the banded LUT call and (b) the full matrix call, on identical
inputs, in one process (needs the GPU).

Related 20-letter pairs (banded_bench.related_batch), SW and GlobalGotoh by default, through the host
API, the three calls alternating so all see the same machine state, each side on a context of its own:

  4096    1,000 x 4096^2  at w = 16, 64, 256
  16384     200 x 16384^2 at w = 16, 64, 256

  bm    sa_align_batch_banded_matrix of this tree with the two-valued table S = match / mismatch
  lut   sa_align_batch_banded / _banded_affine with a match table that is not the identity (the LUT
        fill kernels), on this tree or -- with --lut-lib PATH -- on another build of the engine (the
        parent commit's libseqalib_hip.so) loaded beside this one.  Results and ops must be identical.
  full  sa_align_batch_matrix of this tree with the same table (sa_score_batch_matrix against
        sa_score_batch_banded_matrix where the full call cannot hold its records, which the row says)

Per row: wall time per call (host clock around the blocking call: median, min, max over --reps calls
after --warmup), fill and walk kernel time (sa_last_timings), and -- in a second pass with
$SEQALIB_KERNEL_TIMING set -- the fill kernels alone.  Writes one JSON document (--out) and prints a
table.

    python tools/banded_matrix_bench.py --lut-lib parent/libseqalib_hip.so --out profiles/banded_matrix_bench.json
    python tools/banded_matrix_bench.py --scale 0.05 --reps 2      # a quick rehearsal
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import seqalib_amd as sa  # noqa: E402
from banded_bench import AA, band_cells, related_batch, stats  # noqa: E402
from submat_bench import OtherEngine  # noqa: E402

ALGOS = {"sw": (sa.SA_SW, (-1, 1, -1)), "nw": (sa.SA_NW, (-1, 1, -1)),
         "gg": (sa.SA_GLOBAL_GOTOH, (-3, -1, 1, -1)), "lg": (sa.SA_LOCAL_GOTOH, (-3, -1, 1, -1))}
SHAPES = {"4096": dict(npairs=1000, length=4096, ws=(16, 64, 256)),
          "16384": dict(npairs=200, length=16384, ws=(16, 64, 256))}


class OtherBandedEngine(OtherEngine):
    """OtherEngine with the banded calls declared."""

    def __init__(self, path, device=0):
        super().__init__(path, device)
        vp = C.c_void_p
        for fn in ("sa_align_batch_banded", "sa_align_batch_banded_affine"):
            getattr(self.L, fn).argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64]


def run_row(eng, lut_eng, full_eng, name, batch, w, reps, warmup):
    algo, args = ALGOS[name]
    affine = len(args) == 4
    sc = sa.ScoringSystem(*args)
    ma, mi = (args[2], args[3]) if affine else (args[1], args[2])
    tab = np.where(np.eye(256, dtype=bool), ma, mi).astype(np.int16)
    lut = np.eye(256, dtype=np.uint8)
    lut[0, 0] = 1
    lut[255, 254] = 1   # not the identity (bytes the batch does not use): the LUT fill kernels run
    lut_call = lut_eng.align_banded_affine_packed if affine else lut_eng.align_banded_packed
    full_mode = "align"
    try:
        full_eng.align_matrix_packed(algo, sc, *batch, tab, lut)
    except sa.SeqalibError:
        full_mode = "score"   # the full align call cannot hold its records

    def full():
        if full_mode == "align":
            return full_eng.align_matrix_packed(algo, sc, *batch, tab, lut)
        return full_eng.score_matrix_packed(algo, sc, *batch, tab, lut), None

    def bm_for_full():   # the banded matrix call of the kind the full side runs
        return eng.score_banded_matrix_packed(algo, sc, *batch, tab, w, lut), None

    kinds = {"bm": (eng, lambda: eng.align_banded_matrix_packed(algo, sc, *batch, tab, w, lut)),
             "lut": (lut_eng, lambda: lut_call(algo, sc, *batch, w, lut)),
             "full": (full_eng, full)}
    if full_mode == "score":
        kinds["bm_score"] = (eng, bm_for_full)
    wall = {k: [] for k in kinds}
    dev = {k: [] for k in kinds}
    last, plans, launches = {}, {}, {}
    os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    for it in range(warmup + reps):
        for k, (e, fn) in kinds.items():   # alternating
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            f, t, nl = e.last_timings()
            if it >= warmup:
                wall[k].append(dt)
                dev[k].append((f, t))
            launches[k] = nl
            plans[k] = e.last_plan_ex()
    os.environ["SEQALIB_KERNEL_TIMING"] = "1"
    kern = {k: [] for k in kinds}
    try:
        for it in range(1 + reps):
            for k, (e, fn) in kinds.items():
                fn()
                if it >= 1:
                    kern[k].append(e.last_kernel_timings()[0])
    finally:
        os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    cells, bmax, full_cells = band_cells(batch[1], batch[3], w)
    (bres, bops), (lres, lops) = last["bm"], last["lut"]
    doc = dict(algo=sa.ALGO_NAMES[algo], scoring=list(args), w=w, B_max=bmax, in_band_cells=cells, full_cells=full_cells,
               full_calls=full_mode, results_equal_lut=bool((bres == lres).all()), ops_equal_lut=bool(np.array_equal(bops, lops)),
               scores_equal_full=int((bres["score"] == last["full"][0]["score"]).sum()),
               scores_not_above_full=bool((bres["score"] <= last["full"][0]["score"]).all()))
    for k in kinds:
        doc[k] = dict(wall=stats(wall[k]), fill_kernel=stats(kern[k]),
                      fill_ms=statistics.median(x[0] for x in dev[k]), walk_ms=statistics.median(x[1] for x in dev[k]),
                      fill_launches_per_call=launches[k],
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    vs_full = "bm" if full_mode == "align" else "bm_score"
    doc["fill_kernel_ratio_bm_over_lut"] = doc["bm"]["fill_kernel"]["median_ms"] / doc["lut"]["fill_kernel"]["median_ms"]
    doc["wall_ratio_bm_over_lut"] = doc["bm"]["wall"]["median_ms"] / doc["lut"]["wall"]["median_ms"]
    doc["speedup_fill_kernel_over_full"] = doc["full"]["fill_kernel"]["median_ms"] / doc[vs_full]["fill_kernel"]["median_ms"]
    doc["speedup_wall_over_full"] = doc["full"]["wall"]["median_ms"] / doc[vs_full]["wall"]["median_ms"]
    doc["bm_fill_cells_per_s"] = cells / (doc["bm"]["fill_kernel"]["median_ms"] * 1e-3)
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--shapes", default="4096,16384")
    ap.add_argument("--algos", default="sw,gg")
    ap.add_argument("--lut-lib", default=None, help="another build of libseqalib_hip.so for the banded LUT side")
    args = ap.parse_args()
    eng = sa.Engine(0)
    lut_eng = OtherBandedEngine(args.lut_lib) if args.lut_lib else sa.Engine(0)
    full_eng = sa.Engine(0)   # every side has a context (workspace, I/O cache) of its own
    rows = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/banded_matrix_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale,
                               lut_side="other build" if args.lut_lib else "this build", rows=rows), fh, indent=1)
                fh.write("\n")

    for shape in args.shapes.split(","):
        spec = SHAPES[shape]
        npairs = max(1, int(round(spec["npairs"] * args.scale)))
        batch = related_batch(99, npairs, spec["length"], AA)
        for name in args.algos.split(","):
            for w in spec["ws"]:
                doc = run_row(eng, lut_eng, full_eng, name, batch, w, args.reps, args.warmup)
                doc.update(shape=f"{npairs} x {spec['length']}^2", alphabet="20 letters")
                rows.append(doc)
                write()   # (after every row: a long run that is cut short keeps what it measured)
                b, l, f = doc["bm"], doc["lut"], doc["full"]
                print(f"{doc['shape']:>16s} {name} w {w:3d} B<={doc['B_max']:4d}  fill kernel ms: bm {b['fill_kernel']['median_ms']:.3f} "
                      f"[{b['fill_kernel']['min_ms']:.3f}, {b['fill_kernel']['max_ms']:.3f}] lut {l['fill_kernel']['median_ms']:.3f} "
                      f"[{l['fill_kernel']['min_ms']:.3f}, {l['fill_kernel']['max_ms']:.3f}] ratio {doc['fill_kernel_ratio_bm_over_lut']:.3f}"
                      f"  wall ms: bm {b['wall']['median_ms']:.2f} [{b['wall']['min_ms']:.2f}, {b['wall']['max_ms']:.2f}] lut "
                      f"{l['wall']['median_ms']:.2f} [{l['wall']['min_ms']:.2f}, {l['wall']['max_ms']:.2f}] ratio "
                      f"{doc['wall_ratio_bm_over_lut']:.3f}  walk ms {b['walk_ms']:.2f}/{l['walk_ms']:.2f}  equal "
                      f"{doc['results_equal_lut']}/{doc['ops_equal_lut']}  | full ({doc['full_calls']}) fill kernel "
                      f"{f['fill_kernel']['median_ms']:.3f} wall {f['wall']['median_ms']:.2f} [{f['wall']['min_ms']:.2f}, "
                      f"{f['wall']['max_ms']:.2f}]: banded x{doc['speedup_fill_kernel_over_full']:.2f} kernel, "
                      f"x{doc['speedup_wall_over_full']:.2f} wall  R {b['plan']['R']}  scores equal "
                      f"{doc['scores_equal_full']}/{npairs}", flush=True)
    eng.close()
    full_eng.close()
    write()
    ok = all(r["results_equal_lut"] and r["ops_equal_lut"] and r["scores_not_above_full"] for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
