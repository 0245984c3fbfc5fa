#!/usr/bin/env python3
"""Generate tests/golden/banded_errors.json: the status and sa_last_error(NULL) text of the banded and
matrix entry points on calls that answer without a context (every batch call passes ctx = NULL, so no
device is touched).  tests/test_banded_errors.py replays the file against the current library.

The file pins behaviour, it does not define it: regenerate it only from a library whose answers are the
ones to keep (it was written from the commit before the banded host layer became its own translation
unit).  Usage:  python tests/golden/make_banded_errors.py [path/to/libseqalib_hip.so]

A case is {"fn", "args", "rc", "err"}.  args are the C arguments in order -- after ctx for the batch
calls -- as JSON: a number, null (a NULL pointer), or one of
  {"scoring": [gap, match, mismatch, gap_open, gap_extend, allow_mismatch]}
  {"u64": [...]} / {"i32": [...]}          an array of that type
  {"bytes": [len, mod, base]}              len bytes, byte k = base + k % mod
  {"table": [fill, diagonal]}              a 256 x 256 int16 table
  {"out": nbytes}                          a zeroed output buffer
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "banded_errors.json")
SW, NW, LG, GG, HB, MM = range(6)
PLAN_QUERIES = ("sa_banded_plan_query", "sa_banded_affine_plan_query", "sa_banded_seeded_plan_query", "sa_matrix_plan_query")


class _Scoring(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("gap", "match", "mismatch", "gap_open", "gap_extend", "allow_mismatch")]


def _materialise(a, keep):
    if a is None or isinstance(a, int):
        return a
    (kind, v), = a.items()
    if kind == "scoring":
        obj = _Scoring(*v)
        keep.append(obj)
        return C.addressof(obj)
    if kind == "u64":
        arr = np.array(v, dtype=np.uint64)
    elif kind == "i32":
        arr = np.array(v, dtype=np.int32)
    elif kind == "bytes":
        n, mod, base = v
        arr = (np.arange(n, dtype=np.uint32) % mod + base).astype(np.uint8) if mod > 1 else np.full(n, base, dtype=np.uint8)
    elif kind == "table":
        arr = np.full((256, 256), v[0], dtype=np.int16)
        np.fill_diagonal(arr, v[1])
    elif kind == "out":
        arr = np.zeros(max(v, 1), dtype=np.uint8)
    else:
        raise ValueError(kind)
    keep.append(arr)
    return arr.ctypes.data


# The C signatures: p pointer, i int, u uint32_t, U uint64_t.
_HEAD = "pipppppu"   # ctx, algo, scoring, seq1, off1, seq2, off2, npairs
_MID = {"banded": "pu", "banded_affine": "pu", "banded_ends_free": "puu", "banded_seeded": "ppuu",
        "banded_matrix": "ppu", "matrix": "pp"}
_SIG = {"sa_banded_plan_query": "iuuuuppp", "sa_banded_affine_plan_query": "iuuuuppp",
        "sa_banded_seeded_plan_query": "iUUiuuppp", "sa_matrix_plan_query": "ipuuuipppp"}
for _fam, _mid in _MID.items():
    _SIG["sa_align_batch_" + _fam] = _HEAD + _mid + "ppU"
    _SIG["sa_score_batch_" + _fam] = _HEAD + _mid + "p"
_CTYPE = {"p": C.c_void_p, "i": C.c_int, "u": C.c_uint32, "U": C.c_uint64}


def run_case(L, case):
    """(rc, sa_last_error(NULL)) of one case.  The thread's error text is first set to a known value
    (sa_wait(NULL): "ctx is NULL"), so a call that succeeds is seen to leave it alone."""
    keep = []
    args = [_materialise(a, keep) for a in case["args"]]
    if case["fn"] not in PLAN_QUERIES:
        args.insert(0, None)   # ctx
    sig = _SIG[case["fn"]]
    assert len(sig) == len(args), case
    fn = getattr(L, case["fn"])
    last_error = L.sa_last_error
    last_error.restype, last_error.argtypes = C.c_char_p, [C.c_void_p]
    L.sa_wait(C.c_void_p(None))
    rc = C.c_int(fn(*[_CTYPE[t](a) for t, a in zip(sig, args)])).value
    return rc, last_error(None).decode()


# ------------------------------------------------------------------------------------- the cases
LIN = {"scoring": [-1, 1, -1, 0, 0, 1]}
LIN_NOMIS = {"scoring": [-1, 2, 0, 0, 0, 0]}
AFF = {"scoring": [0, 1, -1, -3, -1, 1]}
AFF_NOMIS = {"scoring": [0, 2, 0, -3, -1, 0]}
AFF_EXT = {"scoring": [0, 1, -1, -3, 1, 1]}       # gap_extend > 0
LIN_BIG = {"scoring": [-1, 3000000, -1, 0, 0, 1]}   # 201 * 3,000,000 >= 2^29
AFF_BIG = {"scoring": [0, 3000000, -1, -3, -1, 1]}
B31 = 2 ** 31
L24 = 2 ** 24
FIT = 12   # SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END


def offs(*lens):
    o = [0]
    for x in lens:
        o.append(o[-1] + x)
    return {"u64": o}


def batch(family, algo, sc, band=4, lens=None, off1=None, off2=None, npairs=None, free_ends=FIT, diag="auto",
          submat="auto", seqs=False, bufs=False):
    """The align and the score call of one family on the same arguments (after ctx).  lens: [(m, n), ...]
    -> offsets; off1 / off2 override them; seqs: sequence buffers of 'A' ... (else NULL); bufs: result and
    ops buffers (else NULL, ops_cap 0)."""
    if lens is not None:
        off1 = offs(*[m for m, _ in lens]) if off1 is None else off1
        off2 = offs(*[n for _, n in lens]) if off2 is None else off2
        npairs = len(lens) if npairs is None else npairs
    npairs = 0 if npairs is None else npairs
    t1 = off1["u64"][-1] if off1 else 0
    t2 = off2["u64"][-1] if off2 else 0
    s1 = s2 = None
    if seqs is True:
        s1, s2 = {"bytes": [t1, 1, 65]}, {"bytes": [t2, 1, 65]}
    elif seqs:
        s1, s2 = seqs
    head = [algo, sc, s1, off1, s2, off2, npairs]
    if diag == "auto":
        diag = {"i32": [0] * npairs} if npairs else None
    if submat == "auto":
        submat = {"table": [-1, 2]}
    mid = {"banded": [None, band], "banded_affine": [None, band], "banded_ends_free": [None, band, free_ends],
           "banded_seeded": [None, diag, band, free_ends], "banded_matrix": [submat, None, band],
           "matrix": [submat, None]}[family]
    res = {"out": 32 * npairs} if bufs else None
    ops_cap = t1 + t2 + npairs + 1 if bufs else 0
    ops = {"out": ops_cap} if bufs else None
    return [{"fn": "sa_align_batch_" + family, "args": head + mid + [res, ops, ops_cap]},
            {"fn": "sa_score_batch_" + family, "args": head + mid + [res]}]


def plan(kind, *args):
    return [{"fn": "sa_%splan_query" % kind, "args": list(args) + [None, None, None]}]


def matrix_plan(algo, sc, max_m, max_n, npairs, nsym):
    return [{"fn": "sa_matrix_plan_query", "args": [algo, sc, max_m, max_n, npairs, nsym, None, None, None, None]}]


def cases():
    out = []
    one = [(100, 100)]
    # ---- the linear band: its prologue, then the context (the per-pair limits need one)
    f = "banded"
    out += batch(f, NW, LIN) + batch(f, SW, LIN) + batch(f, HB, LIN) + batch(f, NW, LIN, lens=one)
    out += batch(f, NW, None) + batch(f, 9, LIN) + batch(f, -1, LIN)
    for a in (LG, GG, MM):
        out += batch(f, a, LIN)
    out += batch(f, NW, LIN, band=B31) + batch(f, NW, LIN, band=2 ** 32 - 1) + batch(f, NW, LIN_NOMIS, band=0)
    out += batch(f, NW, LIN_NOMIS, band=1) + batch(f, NW, LIN, band=0)
    out += batch(f, 9, None) + batch(f, 9, LIN, band=B31) + batch(f, MM, LIN, band=B31) + batch(f, LG, LIN_NOMIS, band=0)
    # (what the linear calls leave to the context: none of these answers before "ctx is NULL")
    out += batch(f, NW, LIN, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2) + batch(f, NW, LIN, lens=[(L24, 10)])
    out += batch(f, NW, LIN_BIG, lens=one) + batch(f, NW, LIN, lens=[(5000, 5000)], band=2100)
    # ---- the affine band: prologue, per-pair limits, context
    f = "banded_affine"
    out += batch(f, LG, AFF) + batch(f, GG, AFF) + batch(f, GG, AFF, lens=one) + batch(f, LG, AFF, lens=one)
    out += batch(f, GG, None) + batch(f, 9, AFF) + batch(f, 6, AFF)
    for a in (SW, NW, HB, MM):
        out += batch(f, a, AFF)
    out += batch(f, GG, AFF_EXT) + batch(f, GG, AFF, band=B31) + batch(f, GG, AFF_NOMIS, band=0) + batch(f, LG, AFF, band=0)
    out += batch(f, 9, None) + batch(f, SW, AFF_EXT) + batch(f, GG, AFF_EXT, band=B31)
    out += batch(f, GG, AFF, band=B31, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2)
    out += batch(f, GG, AFF_NOMIS, band=0, lens=[(L24, 10)])
    out += batch(f, GG, AFF, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2)
    out += batch(f, GG, AFF, off1=offs(5, 5), off2={"u64": [0, 5, 3]}, npairs=2)
    out += batch(f, GG, AFF, off1={"u64": [0, L24, 3]}, off2=offs(5, 5), npairs=2)    # pair 0 too long, pair 1 decreasing
    out += batch(f, GG, AFF, off1={"u64": [0, 5, 3, 3 + L24]}, off2=offs(5, 5, 5), npairs=3)
    out += batch(f, GG, AFF, lens=[(L24, 10)]) + batch(f, GG, AFF, lens=[(10, L24)])
    out += batch(f, GG, AFF_BIG, lens=one) + batch(f, GG, AFF_BIG, lens=[(L24, 10)])
    out += batch(f, GG, AFF, lens=[(3000, 3000)], band=1100) + batch(f, GG, AFF_BIG, lens=[(3000, 3000)], band=1100)
    out += batch(f, LG, AFF, lens=[(2 ** 21, 2 ** 21)], band=1000) + batch(f, GG, AFF, lens=[(2 ** 21, 2 ** 21)], band=1000)
    out += batch(f, GG, AFF, off1=offs(5), off2=None, npairs=1)    # a NULL offsets array: the limits wait for the context
    # ---- the ends-free band
    f = "banded_ends_free"
    for a, sc in ((NW, LIN), (HB, LIN), (GG, AFF)):
        out += batch(f, a, sc) + batch(f, a, sc, lens=one) + batch(f, a, sc, free_ends=0) + batch(f, a, sc, free_ends=15)
        out += batch(f, a, None) + batch(f, a, sc, free_ends=16) + batch(f, a, sc, free_ends=2 ** 32 - 1)
        out += batch(f, a, sc, band=B31) + batch(f, a, sc, band=B31, free_ends=16)
        out += batch(f, a, sc, lens=[(L24, 10)]) + batch(f, a, sc, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2)
    out += batch(f, 9, LIN) + batch(f, 9, LIN, free_ends=16) + batch(f, 9, None, free_ends=16)
    for a in (SW, LG, MM):
        out += batch(f, a, LIN) + batch(f, a, LIN, free_ends=16) + batch(f, a, LIN, band=B31)
    out += batch(f, NW, LIN_NOMIS, band=0) + batch(f, GG, AFF_NOMIS, band=0) + batch(f, GG, AFF_EXT) + batch(f, GG, AFF_EXT, band=B31)
    out += batch(f, NW, LIN_BIG, lens=one) + batch(f, GG, AFF_BIG, lens=one) + batch(f, HB, LIN_BIG, lens=[(L24, 10)])
    out += batch(f, NW, LIN, lens=[(5000, 5000)], band=2100) + batch(f, GG, AFF, lens=[(3000, 3000)], band=1100)
    out += batch(f, NW, LIN, lens=[(3000, 3000)], band=1100) + batch(f, NW, LIN_BIG, lens=[(5000, 5000)], band=2100)
    out += batch(f, NW, LIN_NOMIS, band=0, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2)
    # ---- the seeded band
    f = "banded_seeded"
    two = [(5, 5), (5, 20)]
    for a, sc in ((NW, LIN), (HB, LIN), (GG, AFF)):
        out += batch(f, a, sc) + batch(f, a, sc, lens=one) + batch(f, a, None) + batch(f, a, sc, free_ends=16)
        out += batch(f, a, sc, band=B31) + batch(f, a, sc, band=B31, free_ends=16)
        out += batch(f, a, sc, lens=two, diag=None) + batch(f, a, sc, lens=two, diag=None, band=B31)
        out += batch(f, a, sc, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2, diag=None)
        out += batch(f, a, sc, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2)
        for bad in (-6, 21):
            out += batch(f, a, sc, lens=two, diag={"i32": [0, bad]})
        for good in (-5, 20):
            out += batch(f, a, sc, lens=two, diag={"i32": [0, good]}, free_ends=15)
        out += batch(f, a, sc, lens=two, diag={"i32": [6, 21]})                                 # both pairs: the first is named
        out += batch(f, a, sc, lens=[(L24, 10), (5, 20)], diag={"i32": [0, 21]})                # pair 0 too long, pair 1's seed outside
        out += batch(f, a, sc, lens=[(5, 20), (L24, 10)], diag={"i32": [10, 0]}, band=2, free_ends=0)
        out += batch(f, a, sc, lens=two, diag={"i32": [0, 10]}, band=2, free_ends=0)            # neither
        out += batch(f, a, sc, lens=two, diag={"i32": [0, 10]}, band=2, free_ends=4)            # no legal end
        out += batch(f, a, sc, lens=two, diag={"i32": [0, 10]}, band=2, free_ends=8)            # no legal begin
        out += batch(f, a, sc, lens=two, diag={"i32": [0, 10]}, band=2, free_ends=FIT)
        out += batch(f, a, sc, lens=[(L24, 10)]) + batch(f, a, sc, lens=[(100, 9000)], diag={"i32": [4000]}, band=2048)
    out += batch(f, 9, LIN) + batch(f, 9, LIN, free_ends=16) + batch(f, 9, None)
    for a in (SW, LG, MM):
        out += batch(f, a, LIN) + batch(f, a, LIN, band=B31) + batch(f, a, LIN, free_ends=16) + batch(f, a, LIN, lens=two, diag=None)
    out += batch(f, NW, LIN_NOMIS, band=0) + batch(f, GG, AFF_NOMIS, band=0) + batch(f, GG, AFF_EXT)
    out += batch(f, GG, AFF_EXT, lens=two, diag={"i32": [0, 21]}) + batch(f, NW, LIN_NOMIS, band=0, lens=two, diag={"i32": [0, 21]})
    out += batch(f, GG, AFF_EXT, lens=two, diag=None) + batch(f, GG, AFF_EXT, lens=two, diag={"i32": [0, 10]}, band=2, free_ends=0)
    out += batch(f, NW, LIN_BIG, lens=one) + batch(f, GG, AFF_BIG, lens=one)
    out += batch(f, NW, LIN_BIG, lens=two, diag={"i32": [0, 10]}, band=2, free_ends=0)
    out += batch(f, GG, AFF, lens=[(100, 9000)], diag={"i32": [4000]}, band=1024)
    out += batch(f, GG, AFF, lens=[(100, 9000)], diag={"i32": [4000]}, band=1023)
    # ---- the matrix calls and the matrix band: table and buffer checks come before the context
    many = ({"bytes": [130, 65, 33]}, {"bytes": [10, 1, 65]})
    for f in ("matrix", "banded_matrix"):
        k = dict(bufs=True, seqs=True)
        for a, sc in ((SW, LIN), (NW, LIN), (LG, AFF), (GG, AFF)):
            out += batch(f, a, sc, lens=one, **k) + batch(f, a, sc, lens=[], off1=offs(), off2=offs())
            out += batch(f, a, None, lens=one, **k) + batch(f, a, sc, lens=one, submat=None, **k)
            out += batch(f, a, sc, lens=one, band=B31, **k) + batch(f, a, sc, lens=one, band=B31, submat=None, **k)
            out += batch(f, a, sc, lens=one, band=0, **k)
        for a in (HB, MM):
            out += batch(f, a, LIN, lens=one, **k) + batch(f, a, LIN, lens=one, band=B31, **k) + batch(f, a, LIN, lens=one, submat=None, **k)
        out += batch(f, 9, LIN, lens=one, **k) + batch(f, 9, None, lens=one, **k) + batch(f, 9, LIN, lens=one, band=B31, **k)
        out += batch(f, GG, AFF_EXT, lens=one, **k) + batch(f, GG, AFF_EXT, lens=one, band=B31, **k) + batch(f, LG, AFF_EXT, lens=one, submat=None, **k)
        out += batch(f, MM, AFF_EXT, lens=one, **k)
        out += batch(f, NW, LIN, submat=None) + batch(f, NW, LIN)                                # NULL offsets
        out += batch(f, NW, LIN, off1=offs(5), off2=None, npairs=1, **k)
        out += batch(f, NW, LIN, lens=one, seqs=True) + batch(f, NW, LIN, lens=one, seqs=True, submat=None)   # NULL results / ops
        out += batch(f, NW, LIN, lens=one, bufs=True) + batch(f, NW, LIN, lens=[(0, 0)], bufs=True)           # NULL sequences
        out += batch(f, NW, LIN, lens=[(0, 7)], bufs=True) + batch(f, NW, LIN, lens=[(0, 7)], seqs=True, bufs=True)
        out += batch(f, NW, LIN, off1={"u64": [2, 5]}, off2=offs(5), npairs=1, **k)
        out += batch(f, NW, LIN, off1=offs(5), off2={"u64": [1, 5]}, npairs=1, **k)
        out += batch(f, NW, LIN, off1={"u64": [2, 5, 3]}, off2=offs(5, 5), npairs=2, **k)
        out += batch(f, NW, LIN, off1={"u64": [0, 5, 3]}, off2=offs(5, 5), npairs=2, **k)
        out += batch(f, NW, LIN, off1={"u64": [0, 130, 10]}, off2=offs(5, 5), npairs=2, seqs=many, bufs=True)
        out += batch(f, NW, LIN, lens=[(130, 10)], seqs=many, bufs=True)                          # 65 symbols
        out += batch(f, NW, LIN, lens=[(128, 10)], seqs=({"bytes": [128, 64, 33]}, {"bytes": [10, 1, 33]}), bufs=True)   # 64
        out += batch(f, NW, LIN, lens=[(130, 5), (0, 5)], seqs=many, bufs=True)
        out += batch(f, NW, LIN, lens=[(L24, 10)], **k) + batch(f, GG, AFF, lens=[(10, L24)], **k)
        big = {"table": [-1, 32767]}
        out += batch(f, NW, LIN, lens=[(9000, 9000)], submat=big, **k) + batch(f, GG, AFF, lens=[(9000, 9000)], submat=big, **k)
        out += batch(f, SW, LIN, lens=[(9000, 9000)], submat={"table": [-32768, 1]}, **k)
        out += batch(f, NW, LIN, lens=[(L24, 9000)], submat=big, **k)
        out += batch(f, NW, LIN, lens=[(5000, 5000)], band=2100, **k) + batch(f, GG, AFF, lens=[(3000, 3000)], band=1100, **k)
        out += batch(f, NW, LIN, lens=[(9000, 9000)], band=2100, submat=big, **k)
        out += batch(f, NW, LIN_NOMIS, lens=one, band=0, **k) + batch(f, GG, AFF_NOMIS, lens=one, band=0, **k)
    out += batch("banded_matrix", SW, LIN, lens=[(2 ** 20, 2 ** 20)], band=1100, **k)
    out += batch("banded_matrix", LG, AFF, lens=[(2 ** 21, 2 ** 21)], band=600, **k)
    # ---- the plan queries
    for kind, good, bad in (("banded_", (SW, NW, HB), (LG, GG, MM)), ("banded_affine_", (LG, GG), (SW, NW, HB, MM))):
        for a in good:
            out += plan(kind, a, 100, 100, 4, 1) + plan(kind, a, 100, 100, 0, 1) + plan(kind, a, 100, 100, B31, 1)
            out += plan(kind, a, L24, 100, 4, 1) + plan(kind, a, 100, L24, 4, 1) + plan(kind, a, L24, 100, B31, 1)
            out += plan(kind, a, 5000, 5000, 2100, 1) + plan(kind, a, 3000, 3000, 1100, 1)
            out += plan(kind, a, 2 ** 21, 2 ** 21, 1000, 1) + plan(kind, a, 2 ** 20, 2 ** 20, 2047, 1)
        for a in bad + (9, -1):
            out += plan(kind, a, 100, 100, 4, 1) + plan(kind, a, 100, 100, B31, 1) + plan(kind, a, L24, 100, 4, 1)
    kind = "banded_seeded_"
    for a in (NW, HB, GG):
        out += plan(kind, a, 100, 100, 0, 4, FIT) + plan(kind, a, 100, 100, 0, 4, 16) + plan(kind, a, 100, 100, 0, B31, FIT)
        out += plan(kind, a, 100, 100, 0, B31, 16) + plan(kind, a, L24, 10, 0, 4, FIT) + plan(kind, a, 10, L24, 0, 4, FIT)
        out += plan(kind, a, L24, 10, 11, 4, FIT) + plan(kind, a, 5, 20, -6, 4, FIT) + plan(kind, a, 5, 20, 21, 4, FIT)
        for fe in (0, 4, 8, FIT):
            out += plan(kind, a, 5, 20, 10, 2, fe)
        out += plan(kind, a, 100, 9000, 0, 3996, FIT) + plan(kind, a, 100, 9000, 0, 1948, FIT) + plan(kind, a, 100, 9000, 0, 1947, FIT)
        out += plan(kind, a, 5, 20, 21, 2, 16)
    for a in (SW, LG, MM, 9):
        out += plan(kind, a, 100, 100, 0, 4, FIT) + plan(kind, a, 100, 100, 0, B31, FIT) + plan(kind, a, 100, 100, 0, 4, 16)
        out += plan(kind, a, L24, 10, 0, 4, FIT)
    for a, sc in ((SW, LIN), (NW, LIN), (LG, AFF), (GG, AFF)):
        out += matrix_plan(a, sc, 100, 100, 10, 20) + matrix_plan(a, None, 100, 100, 10, 20) + matrix_plan(a, sc, 100, 100, 10, -1)
        out += matrix_plan(a, sc, 100, 100, 10, 65) + matrix_plan(a, sc, 100, 100, 10, 64) + matrix_plan(a, sc, L24, 100, 10, 20)
        out += matrix_plan(a, sc, 100, L24, 10, 65) + matrix_plan(a, sc, L24, 100, 10, -1)
    for a in (HB, MM, 9):
        out += matrix_plan(a, LIN, 100, 100, 10, 20) + matrix_plan(a, LIN, 100, 100, 10, -1) + matrix_plan(a, None, 100, 100, 10, 20)
    seen, unique = set(), []
    for c in out:   # (families that ignore an argument repeat a call: keep the first)
        key = json.dumps(c, sort_keys=True)
        if key not in seen:
            seen.add(key)
            unique.append(c)
    return unique


def main():
    here_root = os.path.dirname(os.path.dirname(HERE))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here_root, "seqalib_amd", "lib", "libseqalib_hip.so")
    L = C.CDLL(path)
    done = []
    for case in cases():
        rc, err = run_case(L, case)
        done.append(dict(case, rc=rc, err=err))
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in done) + "\n]\n")
    texts = sorted({c["err"] for c in done})
    print(f"{len(done)} cases, {len(texts)} distinct messages -> {FIXTURE}")
    for t in texts:
        print("   ", t)


if __name__ == "__main__":
    main()
