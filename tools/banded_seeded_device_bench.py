#!/usr/bin/env python3
"""The device-resident seeded banded calls against the host-buffer seeded calls on identical pairs, in one
process (needs the GPU).

The three DNA batches of tools/banded_seeded_bench.py (fit: 150 in 1,000; contig: 150 in 100,000; overlap:
2000 x 2000; 2,000 pairs each, w = 16), NW and GlobalGotoh, the two sides alternating so both see the same machine
state, each side on a context of its own:

  host    sa_align_batch_banded_seeded: copies both sequence sets to the device on every call
  device  sa_align_batch_banded_seeded_device: the sequences are resident -- one buffer per side, uploaded once
          outside the timed region -- and a pair is a slice of each (start, length), its seed diagonal and its ops
          offset, resident as well.  In the contig case that buffer is the 200 MB of windows the host side uploads
          on every call.

Per row and side: wall time per call (host clock; the device side from enqueue to the stream's synchronisation),
fill and walk kernel time (sa_last_timings), and for the device side the planner's share of fill_ms: fill_ms less
the fill kernels alone (sa_last_kernel_timings; the device calls run with SEQALIB_KERNEL_TIMING set).  Median,
min and max over --reps calls after --warmup.  Every result and op of the two sides is compared once.  Writes one
JSON document (--out) and prints a table.

    python tools/banded_seeded_device_bench.py --out profiles/banded_seeded_device_bench.json
    python tools/banded_seeded_device_bench.py --scale 0.05 --reps 2      # a quick rehearsal
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import seqalib_amd as sa  # noqa: E402
from banded_bench import stats  # noqa: E402
from banded_seeded_bench import ALGOS, CASES  # noqa: E402


def dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def run_row(engines, name, batch, spec, reps, warmup):
    algo, args = ALGOS[name]
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2, diag = batch
    npairs = len(diag)
    w, fe = spec["w"], spec["free_ends"]
    len1, len2 = np.diff(o1).astype(np.uint32), np.diff(o2).astype(np.uint32)
    ops_off = o1[:-1] + o2[:-1] + np.arange(npairs, dtype=np.uint64)
    ops_bytes = int(o1[-1] + o2[-1]) + npairs
    max_m, max_n = int(len1.max()), int(len2.max())
    # resident: uploaded once, outside the timed region
    d = dict(seq1=dev(s1), start1=dev(o1[:-1]), len1=dev(len1), seq2=dev(s2), start2=dev(o2[:-1]), len2=dev(len2),
             diag=dev(diag.astype(np.int32)), ops_off=dev(ops_off))
    d_res = torch.zeros(npairs * 32, dtype=torch.uint8, device="cuda")
    d_ops = torch.zeros(ops_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def device_call():
        os.environ["SEQALIB_KERNEL_TIMING"] = "1"
        try:
            engines["device"].align_banded_seeded_device(
                algo, sc, d["seq1"].data_ptr(), len(s1), d["start1"].data_ptr(), d["len1"].data_ptr(), d["seq2"].data_ptr(), len(s2),
                d["start2"].data_ptr(), d["len2"].data_ptr(), npairs, max_m, max_n, d["diag"].data_ptr(), w, fe, d_res.data_ptr(),
                d_ops.data_ptr(), d["ops_off"].data_ptr(), ops_bytes)
        finally:
            del os.environ["SEQALIB_KERNEL_TIMING"]
        engines["device"].wait()

    kinds = {"host": lambda: engines["host"].align_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diag, w, fe), "device": device_call}
    wall = {k: [] for k in kinds}
    fill = {k: [] for k in kinds}
    walk = {k: [] for k in kinds}
    planner, fill_kernels = [], []
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
                if k == "device":
                    fk = engines[k].last_kernel_timings()[0]
                    fill_kernels.append(fk)
                    planner.append(f - fk)
            launches[k] = nl
            plans[k] = engines[k].last_plan_ex()
    hres, hops = last["host"]
    dres = d_res.cpu().numpy().view(sa.RESULT_DTYPE)
    dops = d_ops.cpu().numpy()
    same_ops = sum(int(np.array_equal(hops[int(o):int(o) + int(n)], dops[int(o):int(o) + int(n)])) for o, n in zip(ops_off, hres["nops"]))
    doc = dict(algo=sa.ALGO_NAMES[algo], scoring=list(args), w=w, free_ends=fe, max_m=max_m, max_n=max_n,
               resident_bytes=int(len(s1) + len(s2)), results_equal=int(sum(a.tobytes() == b.tobytes() for a, b in zip(hres, dres))),
               ops_equal=same_ops, pairs=npairs)
    for k in kinds:
        doc[k] = dict(fill=stats(fill[k]), walk=stats(walk[k]), wall=stats(wall[k]), launches_per_call=launches[k],
                      plan=dict(kernel=plans[k][0], R=plans[k][1], W=plans[k][2], records=plans[k][3]))
    doc["device"]["planner"] = stats(planner)
    doc["device"]["fill_kernels"] = stats(fill_kernels)
    doc["wall_ratio_host_over_device"] = doc["host"]["wall"]["median_ms"] / doc["device"]["wall"]["median_ms"]
    h = doc["host"]["fill"]
    doc["device_fill_kernels_within_host_spread"] = bool(h["min_ms"] <= doc["device"]["fill_kernels"]["median_ms"] <= h["max_ms"])
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each batch's pairs (rehearsals)")
    ap.add_argument("--cases", default="fit,contig,overlap")
    ap.add_argument("--algos", default="nw,gg")
    args = ap.parse_args()
    engines = {"host": sa.Engine(0), "device": sa.Engine(0)}   # every side has a context of its own
    rows = []

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="tools/banded_seeded_device_bench.py", reps=args.reps, warmup=args.warmup, scale=args.scale,
                               rows=rows), fh, indent=1)
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
            h, dv = doc["host"], doc["device"]
            print(f"{case:>8s} {doc['shape']:>22s} {name}  wall ms host {h['wall']['median_ms']:.3f} device {dv['wall']['median_ms']:.3f} "
                  f"[{dv['wall']['min_ms']:.3f}, {dv['wall']['max_ms']:.3f}]  fill ms host {h['fill']['median_ms']:.3f} "
                  f"[{h['fill']['min_ms']:.3f}, {h['fill']['max_ms']:.3f}] device {dv['fill']['median_ms']:.3f} = planner "
                  f"{dv['planner']['median_ms']:.3f} + fills {dv['fill_kernels']['median_ms']:.3f}  walk ms {h['walk']['median_ms']:.3f}/"
                  f"{dv['walk']['median_ms']:.3f}  chunks {dv['launches_per_call']}  equal {doc['results_equal']}/{npairs} ops "
                  f"{doc['ops_equal']}/{npairs}", flush=True)
    for e in engines.values():
        e.close()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
