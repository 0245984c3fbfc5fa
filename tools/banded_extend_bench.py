#!/usr/bin/env python3
"""The banded extension calls against what a user did before them: the seeded banded calls with diag = 0 and
SA_FREE_SEQ1_END | SA_FREE_SEQ2_END on identical pairs, in one process (needs the GPU).

Two DNA batches of 2,000 pairs of 2,000 symbols, NW (-2, 1, -3) and GlobalGotoh (-4, -1, 1, -3), w = 16, the
score call and the align call, the two sides alternating so both see the same machine state, each side on a
context of its own:

  diverging  150 related symbols (3 % substitutions), then 1,850 unrelated ones; xdrop = 30.  The tool first
             asserts, on the model of tests/extend_model.py, that every pair of the batch stops before a quarter
             of its steps, and reports the worst and the mean fraction of steps swept
  related    8 % edits throughout (6 % substitutions, 2 % insertions and deletions in turn); xdrop = SA_XDROP_OFF and
             xdrop = 30, under which the model stops no pair of a sample (--model-pairs: here the model has to
             run the whole sweep of every pair it looks at)

  extend  sa_score_batch_banded_extend / sa_align_batch_banded_extend of this tree
  base    sa_score_batch_banded_seeded / sa_align_batch_banded_seeded, on this tree or -- with --base-lib PATH --
          on another build of the engine (the parent commit's libseqalib_hip.so) loaded beside this one

Per row and side: fill and walk kernel time (sa_last_timings: median, min, max over --reps calls after
--warmup) and wall time per call.  fill_ratio_extend_over_base is extend's median fill time over base's;
below_base says whether extend's whole [min, max] lies below base's.  Writes one JSON document (--out) and
prints a table.

    python tools/banded_extend_bench.py --base-lib parent/libseqalib_hip.so --out profiles/banded_extend_bench.json
    python tools/banded_extend_bench.py --scale 0.05 --reps 2      # a quick rehearsal
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seqalib_amd as sa  # noqa: E402
from banded_bench import ACGT, stats  # noqa: E402
from banded_free_bench import substituted  # noqa: E402
from extend_model import extend_band, extend_fill_np  # noqa: E402
from submat_bench import OtherEngine  # noqa: E402

ALGOS = {"nw": (sa.SA_NW, (-2, 1, -3)), "gg": (sa.SA_GLOBAL_GOTOH, (-4, -1, 1, -3))}
BOTH_ENDS = sa.SA_FREE_SEQ1_END | sa.SA_FREE_SEQ2_END
W, LENGTH, XDROP = 16, 2000, 30


class OtherSeededEngine(OtherEngine):
    """OtherEngine with the seeded banded calls declared."""

    def __init__(self, path, device=0):
        super().__init__(path, device)
        vp = C.c_void_p
        self.L.sa_align_batch_banded_seeded.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32,
                                                        C.c_uint32, vp, vp, C.c_uint64]
        self.L.sa_score_batch_banded_seeded.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32,
                                                        C.c_uint32, vp]


def diverging_batch(seed, npairs, head=150):
    rng = np.random.default_rng(seed)
    s1 = ACGT[rng.integers(0, 4, (npairs, LENGTH))]
    s2 = ACGT[rng.integers(0, 4, (npairs, LENGTH))]
    s2[:, :head] = substituted(rng, s1[:, :head])
    o = np.arange(npairs + 1, dtype=np.uint64) * LENGTH
    return np.ascontiguousarray(s1.reshape(-1)), o, np.ascontiguousarray(s2.reshape(-1)), o.copy()


def related_batch(seed, npairs, percent=8):
    """Seq2 = Seq1 with `percent` of its symbols edited: three quarters substituted, a quarter inserted before or
    deleted in turn -- so the path stays within a diagonal of the main one and no pair leaves a band of 16 --
    cut or padded to the same length."""
    rng = np.random.default_rng(seed)
    s1 = ACGT[rng.integers(0, 4, (npairs, LENGTH))]
    rows = []
    for p in range(npairs):
        r = rng.integers(0, 400, LENGTH)
        fresh = ACGT[rng.integers(0, 4, LENGTH)]
        sub, indel = r < 3 * percent, (r >= 3 * percent) & (r < 4 * percent)
        turn = np.cumsum(indel) % 2
        ins, dele = indel & (turn == 1), indel & (turn == 0)
        count = np.where(ins, 2, np.where(dele, 0, 1))
        out = np.repeat(np.where(sub, fresh, s1[p]), count)
        first = np.cumsum(count) - count
        out[first[ins]] = fresh[ins]
        out = np.concatenate([out, ACGT[rng.integers(0, 4, LENGTH)]])[:LENGTH]
        rows.append(out)
    o = np.arange(npairs + 1, dtype=np.uint64) * LENGTH
    return np.ascontiguousarray(s1.reshape(-1)), o, np.ascontiguousarray(np.stack(rows).reshape(-1)), o.copy()


CASES = {"diverging": dict(make=diverging_batch, xdrops=(XDROP,), stops=True),
         "related": dict(make=related_batch, xdrops=(sa.SA_XDROP_OFF, XDROP), stops=False)}


def model_sample(algo, args, batch, xdrop, count):
    """The fraction of its steps each of the first `count` pairs sweeps under the model (1.0: it does not stop)."""
    s1, o1, s2, o2 = batch
    out = []
    for p in range(count):
        a, b = s1[int(o1[p]):int(o1[p + 1])].tobytes(), s2[int(o2[p]):int(o2[p + 1])].tobytes()
        stop = extend_fill_np(algo, args, a, b, W, xdrop)[4]
        tend = extend_band(len(a), len(b), W)[2]
        out.append(1.0 if stop is None else (stop + 1) / (tend + 1))
    return out


def run_row(engines, name, batch, xdrop, mode, reps, warmup):
    algo, args = ALGOS[name]
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = batch
    zero = np.zeros(len(o1) - 1, dtype=np.int32)
    ext, base = engines["extend"], engines["base"]
    if mode == "score":
        kinds = {"extend": lambda: ext.score_banded_extend_packed(algo, sc, s1, o1, s2, o2, W, xdrop),
                 "base": lambda: base.score_banded_seeded_packed(algo, sc, s1, o1, s2, o2, zero, W, BOTH_ENDS)}
    else:
        kinds = {"extend": lambda: ext.align_banded_extend_packed(algo, sc, s1, o1, s2, o2, W, xdrop)[0],
                 "base": lambda: base.align_banded_seeded_packed(algo, sc, s1, o1, s2, o2, zero, W, BOTH_ENDS)[0]}
    wall = {k: [] for k in kinds}
    fill = {k: [] for k in kinds}
    walk = {k: [] for k in kinds}
    last, plans = {}, {}
    for it in range(warmup + reps):
        for k, fn in kinds.items():   # alternating
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            f, t, _ = engines[k].last_timings()
            if it >= warmup:
                wall[k].append(dt)
                fill[k].append(f)
                walk[k].append(t)
            plans[k] = engines[k].last_plan_ex()
    doc = dict(algo=sa.ALGO_NAMES[algo], scoring=list(args), w=W, xdrop=xdrop, mode=mode,
               dropped=int((last["extend"]["flags"] == sa.SA_FLAG_DROPPED).sum()),
               mean_end_step_fraction=float(((last["extend"]["end_i"] + last["extend"]["end_j"]) / (2.0 * LENGTH)).mean()))
    for k in kinds:
        doc[k] = dict(fill=stats(fill[k]), walk=stats(walk[k]), wall=stats(wall[k]),
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    doc["fill_ratio_extend_over_base"] = doc["extend"]["fill"]["median_ms"] / doc["base"]["fill"]["median_ms"]
    doc["wall_ratio_extend_over_base"] = doc["extend"]["wall"]["median_ms"] / doc["base"]["wall"]["median_ms"]
    doc["below_base"] = doc["extend"]["fill"]["max_ms"] < doc["base"]["fill"]["min_ms"]
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--cases", default="diverging,related")
    ap.add_argument("--algos", default="nw,gg")
    ap.add_argument("--modes", default="score,align")
    ap.add_argument("--model-pairs", type=int, default=24, help="pairs of the related batch the model checks before the run")
    ap.add_argument("--base-lib", default=None, help="another build of libseqalib_hip.so for the seeded side")
    args = ap.parse_args()
    npairs = max(1, int(round(2000 * args.scale)))
    batches = {case: CASES[case]["make"](99, npairs) for case in args.cases.split(",")}
    # what the batches are meant to do, on the model, before any time is taken
    swept = {}
    for case, batch in batches.items():
        for name in args.algos.split(","):
            algo, sc = ALGOS[name]
            # (a pair that stops costs the model a tenth of its sweep: every diverging pair is checked)
            frac = model_sample(algo, sc, batch, XDROP, npairs if CASES[case]["stops"] else min(args.model_pairs, npairs))
            if CASES[case]["stops"]:
                assert max(frac) < 0.25, (case, name, max(frac))
            else:
                assert min(frac) == 1.0, (case, name, min(frac))
            swept[case, name] = dict(mean=float(np.mean(frac)), worst=float(max(frac)), pairs=len(frac))
    # every side has a context (workspace, I/O cache) of its own
    engines = {"extend": sa.Engine(0), "base": OtherSeededEngine(args.base_lib) if args.base_lib else sa.Engine(0)}
    rows = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/banded_extend_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale,
                               base_side="other build" if args.base_lib else "this build", rows=rows), fh, indent=1)
                fh.write("\n")

    for case, batch in batches.items():
        for name in args.algos.split(","):
            for xdrop in CASES[case]["xdrops"]:
                for mode in args.modes.split(","):
                    doc = run_row(engines, name, batch, xdrop, mode, args.reps, args.warmup)
                    doc.update(case=case, shape=f"{npairs} x {LENGTH} x {LENGTH}", alphabet="ACGT",
                               model_steps_swept=swept[case, name]["mean"] if xdrop >= 0 else 1.0,
                               model_steps_swept_worst=swept[case, name]["worst"] if xdrop >= 0 else 1.0,
                               model_pairs_checked=swept[case, name]["pairs"])
                    if CASES[case]["stops"]:
                        assert doc["dropped"] == npairs, doc["dropped"]
                    elif xdrop < 0:
                        assert doc["dropped"] == 0, doc["dropped"]   # (under xdrop = 30 the count is reported: the model saw a sample)
                    rows.append(doc)
                    write()   # (after every row: a run that is cut short keeps what it measured)
                    e, b = doc["extend"], doc["base"]
                    print(f"{case:>9s} {name} {mode:5s} xdrop {xdrop:3d} R {e['plan']['R']}  fill ms: extend {e['fill']['median_ms']:.3f} "
                          f"[{e['fill']['min_ms']:.3f}, {e['fill']['max_ms']:.3f}] base {b['fill']['median_ms']:.3f} [{b['fill']['min_ms']:.3f}, "
                          f"{b['fill']['max_ms']:.3f}] extend/base {doc['fill_ratio_extend_over_base']:.3f} (steps swept "
                          f"{doc['model_steps_swept']:.3f}, worst {doc['model_steps_swept_worst']:.3f} of {doc['model_pairs_checked']} pairs) below {doc['below_base']}  walk ms {e['walk']['median_ms']:.3f}/"
                          f"{b['walk']['median_ms']:.3f}  wall ms {e['wall']['median_ms']:.2f}/{b['wall']['median_ms']:.2f}  dropped "
                          f"{doc['dropped']}/{npairs}", flush=True)
    engines["extend"].close()
    if not args.base_lib:
        engines["base"].close()
    write()
    bad = [r for r in rows if r["case"] == "diverging" and not r["below_base"]]
    if bad:
        print(f"FAIL: {len(bad)} diverging rows whose extend fill does not lie wholly below the base's", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
