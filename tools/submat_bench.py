#!/usr/bin/env python3
"""Matrix align call against the LUT align call on identical inputs, in one process (needs the GPU).

1,000 x 4096^2 related 20-letter pairs (the mutation model of tools/banded_bench.py), SW and
GlobalGotoh, through the host API:

  matrix   sa_align_batch_matrix with the table S = match on the diagonal, mismatch elsewhere
  lut      sa_align_batch with a match table equal to byte equality (the int32 LUT kernels)

Both sides run the same plan and return the same results (checked), so the difference is the cell:
one 16-bit LDS gather of the score against one LDS read of a match bit and a select.  The two calls
alternate, --warmup + --reps times; per side: wall time per call (median, min, max), fill and walk
time (sa_last_timings) and, in a second pass with $SEQALIB_KERNEL_TIMING, the fill kernel alone.

--lut-lib PATH runs the LUT side on another build of the engine (the parent commit's
libseqalib_hip.so) loaded beside this tree's, so a change of the shared fill code shows too.

    python tools/submat_bench.py --out profiles/submat_bench.json
    python tools/submat_bench.py --scale 0.05 --reps 2      # a quick rehearsal
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
from banded_bench import AA, related_batch, stats  # noqa: E402

ALGOS = {"sw": (sa.SA_SW, (-1, 1, -1)), "gg": (sa.SA_GLOBAL_GOTOH, (-3, -1, 1, -1))}


class OtherEngine(sa.Engine):
    """An Engine on another build of the library (only what this tool calls is declared)."""

    def __init__(self, path, device=0):
        sa.load_library()   # (binds the HIP runtime first, as the package does)
        L = C.CDLL(path)
        vp, i32p = C.c_void_p, C.POINTER(C.c_int)
        L.sa_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.sa_destroy.argtypes = [vp]
        L.sa_destroy.restype = None
        L.sa_last_error.argtypes = [vp]
        L.sa_last_error.restype = C.c_char_p
        L.sa_status_string.argtypes = [C.c_int]
        L.sa_status_string.restype = C.c_char_p
        L.sa_align_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64]
        L.sa_last_timings.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i32p]
        L.sa_last_kernel_timings.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.sa_last_plan_ex.argtypes = [vp, i32p, i32p, i32p, i32p]
        self.L = L
        h = vp()
        if L.sa_create(device, C.byref(h)) != 0:
            raise sa.SeqalibError(f"sa_create on {path} failed: {L.sa_last_error(None).decode()}")
        self.h = h
        self.device = device


def run_algo(eng, lut_eng, name, batch, reps, warmup):
    algo, args = ALGOS[name]
    sc = sa.ScoringSystem(*args)
    ma, mi = (args[2], args[3]) if len(args) == 4 else (args[1], args[2])
    tab = np.where(np.eye(256, dtype=bool), ma, mi).astype(np.int16)
    lut = np.eye(256, dtype=np.uint8)
    lut[0, 0] = 1
    lut[255, 254] = 1   # not the identity: the host keeps the table (the int32 LUT kernels run)
    kinds = {"matrix": (eng, lambda: eng.align_matrix_packed(algo, sc, *batch, tab)),
             "lut": (lut_eng, lambda: lut_eng.align_packed(algo, sc, *batch, lut))}
    wall = {k: [] for k in kinds}
    dev = {k: [] for k in kinds}
    last, plans = {}, {}
    os.environ.pop("SEQALIB_KERNEL_TIMING", None)
    for it in range(warmup + reps):
        for k, (e, fn) in kinds.items():   # alternating
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            f, t, _ = e.last_timings()
            if it >= warmup:
                wall[k].append(dt)
                dev[k].append((f, t))
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
    (mres, mops), (lres, lops) = last["matrix"], last["lut"]
    cells = int((np.diff(batch[1]).astype(np.int64) * np.diff(batch[3]).astype(np.int64)).sum())
    doc = dict(algo=sa.ALGO_NAMES[algo], scoring=list(args), cells=cells,
               results_equal=bool((mres == lres).all()), ops_equal=bool(np.array_equal(mops, lops)))
    for k in kinds:
        doc[k] = dict(wall=stats(wall[k]), fill_kernel=stats(kern[k]),
                      fill_ms=statistics.median(x[0] for x in dev[k]), walk_ms=statistics.median(x[1] for x in dev[k]),
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
        doc[k]["fill_gcups"] = cells / (doc[k]["fill_kernel"]["median_ms"] * 1e-3) / 1e9
    doc["fill_kernel_ratio_matrix_over_lut"] = doc["matrix"]["fill_kernel"]["median_ms"] / doc["lut"]["fill_kernel"]["median_ms"]
    doc["wall_ratio_matrix_over_lut"] = doc["matrix"]["wall"]["median_ms"] / doc["lut"]["wall"]["median_ms"]
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the batch's pairs (rehearsals)")
    ap.add_argument("--algos", default="sw,gg")
    ap.add_argument("--lut-lib", default=None, help="another build of libseqalib_hip.so for the LUT side")
    args = ap.parse_args()
    eng = sa.Engine(0)
    lut_eng = OtherEngine(args.lut_lib) if args.lut_lib else eng
    npairs = max(1, int(round(1000 * args.scale)))
    batch = related_batch(99, npairs, 4096, AA)
    rows = []
    for name in args.algos.split(","):
        doc = run_algo(eng, lut_eng, name, batch, args.reps, args.warmup)
        doc.update(shape=f"{npairs} x 4096^2", alphabet="20 letters", lut_side="other build" if args.lut_lib else "this build")
        rows.append(doc)
        m, l = doc["matrix"], doc["lut"]
        print(f"{doc['shape']:>14s} {name}  fill kernel ms: matrix {m['fill_kernel']['median_ms']:.3f} "
              f"[{m['fill_kernel']['min_ms']:.3f}, {m['fill_kernel']['max_ms']:.3f}] lut {l['fill_kernel']['median_ms']:.3f} "
              f"[{l['fill_kernel']['min_ms']:.3f}, {l['fill_kernel']['max_ms']:.3f}] ratio {doc['fill_kernel_ratio_matrix_over_lut']:.3f}"
              f"  wall ms: matrix {m['wall']['median_ms']:.2f} [{m['wall']['min_ms']:.2f}, {m['wall']['max_ms']:.2f}] lut "
              f"{l['wall']['median_ms']:.2f} [{l['wall']['min_ms']:.2f}, {l['wall']['max_ms']:.2f}]  walk ms {m['walk_ms']:.2f}/{l['walk_ms']:.2f}"
              f"  GCUPS {m['fill_gcups']:.0f}/{l['fill_gcups']:.0f}  R {m['plan']['R']}/{l['plan']['R']} W {m['plan']['W']}/{l['plan']['W']}"
              f"  equal {doc['results_equal'] and doc['ops_equal']}", flush=True)
    if lut_eng is not eng:
        lut_eng.close()
    eng.close()
    result = dict(tool="tools/submat_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    return 0 if all(r["results_equal"] and r["ops_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
