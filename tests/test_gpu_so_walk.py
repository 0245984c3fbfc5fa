"""The quad traceback of the score-only fill (traceback_so4_kernel, sa_traceback_so.hip), walk by
walk: batches built so that every way a walk can move through, leave and stop in the recomputed
blocks occurs, under both lane counts per pair (SEQALIB_TB_LP = 4 and 8), for Smith-Waterman and
Needleman-Wunsch.

Method of tests/test_gpu_so.py: the same batch runs score-only (SEQALIB_SO=1: no records, the tags
recomputed block by block) and with tagged records (SEQALIB_SO=0); every result field and op stream
must be equal, and every pair is checked against the full-matrix oracle.

The batches (1,040 pairs; the special pairs first, so that they share waves -- 16 pairs per wave at
LP = 4, 8 at LP = 8 -- with each other and with empty and short pairs):
  * R = 32, two bands (rows up to 2,400): the U run of the deletion pair crosses row 2,048, where
    the top row of a block comes from lane 63 of the band above;
  * R = 16, one band (rows up to 1,024 = 64 R; 64 R + 1 rows would make the plan R = 32, so that
    shape is in the R = 32 batch as 2,048 / 2,049).
A run of L moves at columns below 32 in a lane other than the first needs fewer rows above it than
columns (R = 16: row 20, lane 1); in the R = 32 batch row 20 is lane 0, whose first blocks have no
left snapshot but start at column 0, and the blocks that start left of column 0 are crossed by the
diagonal and border-bound walks instead.  Smith-Waterman cannot put a long L run near column 0 at
all (the alignment before it must outweigh it), so its L run is the pair with 300 rows above it.
"""
import os

import numpy as np
import pytest

import seqalib_amd as sa
from util import oracle_align, oracle_batch

pytestmark = pytest.mark.gpu
BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py)

SW = (-1, 1, -1)
NW = (-1, 2, -1)
THREADS = 16
FIELDS = ("score", "end_i", "end_j", "start_i", "start_j", "nops", "flags")
NPAIRS = 1040
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, k):
    return ACGT[rng.integers(0, 4, k)]


def _subst(rng, a, rate):
    b = a.copy()
    hit = rng.random(len(b)) < rate
    b[hit] = ACGT[(np.searchsorted(ACGT, b[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    return b


def special_pairs(R, rng):
    """name -> (seq1, seq2); see the module docstring."""
    M = 64 * R
    long_m = 2400 if R == 32 else M
    d0 = 1990 if R == 32 else 500            # first deleted row (0-based); the run is 120 long
    sub = 0.10 if R == 32 else 0.04          # (keeps the R = 32 scores under the f16 cell's retry threshold)
    # (linear gaps cost the same wherever they stand, so an alignment spreads a long gap over chance
    # matches; a run of T in sequences drawn from A, C, G cannot match anything and stays one run)
    A = ACGT[rng.integers(0, 3, long_m)]
    A[d0:d0 + 120] = ord("T")
    B = ACGT[rng.integers(0, 3, 700)]
    C = _rand(rng, 60)
    sp = {}
    sp["deleted_run"] = (A, np.concatenate([_subst(rng, A[:d0 - 40], sub), A[d0 - 40:d0], A[d0 + 120:d0 + 160],
                                            _subst(rng, A[d0 + 160:], sub)]))
    sp["empty_1"] = (_rand(rng, 0), _rand(rng, 5))
    ins = np.full(160, ord("T"), np.uint8)
    sp["inserted_run_row300"] = (B, np.concatenate([B[:300], ins, B[300:]]))
    sp["empty_2"] = (_rand(rng, 5), _rand(rng, 0))
    ident = _rand(rng, 1500 if R == 32 else 1000)
    sp["identical"] = (ident, ident.copy())                      # pure diagonal; end cell (m, n)
    sp["m1"] = (_rand(rng, 1), _rand(rng, 40))
    sp["inserted_run_row20"] = (B[:500], np.concatenate([B[:20], ins, B[20:500]]))
    sp["one_one"] = (C[:1], C[:1].copy())
    # second half of the first LP = 4 wave
    sp["m_64R"] = (A[:M], _subst(rng, A[:M], 0.12)[:M - 7])
    if R == 32:
        sp["m_64R_plus_1"] = (A[:M + 1], _subst(rng, A[:M + 1], 0.12))
        hot = _rand(rng, 2100)
        sp["above_f16_threshold"] = (hot, hot.copy())            # SW score 2,100: flagged, re-run in int32
    sp["n17"] = (B[:100], _subst(rng, B[40:57], 0.1))
    sp["n31"] = (B[:100], _subst(rng, B[30:61], 0.1))
    sp["n33"] = (B[:100], _subst(rng, B[30:63], 0.1))
    sp["n63"] = (B[:90], _subst(rng, B[10:73], 0.1))
    sp["n1"] = (B[:50], B[7:8].copy())
    # SW stops: H == 0 inside a block (a common core in unrelated flanks), on row 0, on column 0
    sp["stop_mid_block"] = (np.concatenate([_rand(rng, 75), C, _rand(rng, 40)]),
                            np.concatenate([_rand(rng, 47), C, _rand(rng, 30)]))
    sp["stop_row0"] = (np.concatenate([C, _rand(rng, 50)]), np.concatenate([_rand(rng, 300), C]))
    sp["stop_col0"] = (np.concatenate([_rand(rng, 900 if R == 32 else 600), C]), np.concatenate([C, _rand(rng, 50)]))
    # NW: the walk reaches the border far from (0, 0) -- column 0 deep in the band, and row 0
    sp["border_col0"] = (B, B[420:].copy())
    sp["border_row0"] = (B[380:].copy(), B)
    sp["border_col0_long"] = (A[:long_m - 50], A[long_m - 450:long_m - 50].copy())
    return sp


_BATCH = {}


def batch(R):
    """(s1, o1, s2, o2, index of each special pair)."""
    if R in _BATCH:
        return _BATCH[R]
    rng = np.random.default_rng(1000 + R)
    sp = special_pairs(R, rng)
    names = list(sp)
    pairs = [sp[k] for k in names]
    # a second copy of the long walks beside short pairs in a later wave, then ragged short pairs
    for k in ("identical", "deleted_run", "inserted_run_row300"):
        pairs.extend([(_rand(rng, 9), _rand(rng, 12)), sp[k], (_rand(rng, 0), _rand(rng, 0))])
    while len(pairs) < NPAIRS:
        m, n = int(rng.integers(0, 130)), int(rng.integers(0, 130))
        a = _rand(rng, m)
        if len(pairs) % 4 == 3 and m > 8:
            keep = rng.random(m) > 0.05
            b = _subst(rng, a, 0.08)[keep]
            at = np.nonzero(rng.random(len(b)) < 0.05)[0]
            b = np.insert(b, at, _rand(rng, len(at)))
        else:
            b = _rand(rng, n)
        pairs.append((a, b))
    o1 = np.zeros(NPAIRS + 1, np.uint64)
    o2 = np.zeros(NPAIRS + 1, np.uint64)
    o1[1:] = np.cumsum([len(a) for a, _ in pairs])
    o2[1:] = np.cumsum([len(b) for _, b in pairs])
    s1 = np.concatenate([a for a, _ in pairs]).astype(np.uint8)
    s2 = np.concatenate([b for _, b in pairs]).astype(np.uint8)
    _BATCH[R] = (s1, o1, s2, o2, {k: i for i, k in enumerate(names)})
    return _BATCH[R]


AG_CT = np.zeros((256, 256), np.uint8)   # a non-identity match table on the 4-symbol alphabet: A~G, C~T
for _x in b"ACGT":
    AG_CT[_x, _x] = 1
for _x, _y in (b"AG", b"GA", b"CT", b"TC"):
    AG_CT[_x, _y] = 1

_ORACLE = {}


def oracle(R, algo, scoring, lut):
    """Full-matrix oracle results of every pair of batch(R), computed once per (scoring, table):
    list of (score, end_i, end_j, start_i, start_j, ops bytes)."""
    key = (R, algo, scoring, lut is not None)
    if key in _ORACLE:
        return _ORACLE[key]
    s1, o1, s2, o2, _ = batch(R)
    out = []
    if lut is None:
        res, ops = oracle_batch(algo, scoring, s1, o1, s2, o2, threads=THREADS)
        for p in range(NPAIRS):
            off = int(o1[p] + o2[p]) + p
            out.append((int(res["score"][p]), int(res["end_i"][p]), int(res["end_j"][p]), int(res["start_i"][p]),
                        int(res["start_j"][p]), ops[off:off + int(res["nops"][p])].tobytes()))
    else:
        for p in range(NPAIRS):
            o = oracle_align(algo, scoring, s1[int(o1[p]):int(o1[p + 1])].tobytes(), s2[int(o2[p]):int(o2[p + 1])].tobytes(), lut=lut)
            out.append((o["score"], o["end_i"], o["end_j"], o["start_i"], o["start_j"], o["ops"]))
    _ORACLE[key] = out
    return out


def run(engine, so, lp, b, algo, scoring, lut):
    """One align_packed call: so = score-only fill (else tagged records), lp = SEQALIB_TB_LP
    (SEQALIB_TB_SO stays at its default: the quad kernel, not the one-lane walker)."""
    env = {"SEQALIB_SO": "1" if so else "0", "SEQALIB_TB_LP": lp}
    old = {k: os.environ.get(k) for k in list(env) + ["SEQALIB_TB_SO"]}
    os.environ.update(env)
    os.environ.pop("SEQALIB_TB_SO", None)
    try:
        res, ops = engine.align_packed(algo, sa.ScoringSystem(*scoring), *b[:4], lut=lut)
        plan, recs = engine.last_plan(), engine.last_plan_ex()[3]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res.copy(), ops.copy(), plan, recs


def check(engine, R, lp, algo, scoring, lut=None):
    b = batch(R)
    s1, o1, s2, o2, _ = b
    so = run(engine, True, lp, b, algo, scoring, lut)
    tg = run(engine, False, lp, b, algo, scoring, lut)
    assert so[2][1:] == (R, 1) and tg[2] == so[2], (so[2], tg[2])
    assert so[3] == sa.SA_RECORDS_SCORE_ONLY
    for f in FIELDS:
        bad = np.nonzero(so[0][f] != tg[0][f])[0]
        assert len(bad) == 0, (f, [(int(p), int(so[0][f][p]), int(tg[0][f][p])) for p in bad[:5]])
    assert (so[0]["flags"] == 0).all()
    exp = oracle(R, algo, scoring, lut)
    res, ops = so[0], so[1]
    for p in range(NPAIRS):
        off = int(o1[p] + o2[p]) + p
        k = int(res["nops"][p])
        assert ops[off:off + k].tobytes() == tg[1][off:off + k].tobytes(), f"op stream of pair {p} differs from the tagged path"
        got = (int(res["score"][p]), int(res["end_i"][p]), int(res["end_j"][p]), int(res["start_i"][p]),
               int(res["start_j"][p]), ops[off:off + k].tobytes())
        assert got == exp[p], (p, got[:5], exp[p][:5])
    return so


@pytest.mark.parametrize("lp", ["4", "8"])
@pytest.mark.parametrize("R", [32, 16])
def test_sw_walks(engine, R, lp):
    """Smith-Waterman: every pair equal to the tagged path and the oracle, and the batch holds the
    walks it was built for (asserted on the op streams: they are emitted from the end cell back)."""
    so = check(engine, R, lp, 0, SW)
    s1, o1, s2, o2, at = batch(R)
    res, ops = so[0], so[1]

    def walk(name):
        p = at[name]
        off = int(o1[p] + o2[p]) + p
        return p, ops[off:off + int(res["nops"][p])].tobytes()

    p, w = walk("identical")
    m = int(o1[p + 1] - o1[p])
    assert w == b"M" * m and (int(res["end_i"][p]), int(res["end_j"][p])) == (m, m)   # end cell in the last row and column
    p, w = walk("deleted_run")
    assert b"U" * 100 in w
    if R == 32:   # the run crosses the band boundary: the walk is above row 2,048 after it, below before
        k = w.index(b"U" * 100)
        i_before = int(res["end_i"][p]) - sum(c in b"MSXU" for c in w[:k])
        assert i_before > 2048 + 32 and i_before - 100 < 2048 - 32
        assert int(res["score"][at["above_f16_threshold"]]) == 2100
    p, w = walk("inserted_run_row300")
    assert b"L" * 128 in w                                       # >= 4 chunks of 32 columns
    p, w = walk("stop_mid_block")
    assert int(res["start_i"][p]) % R not in (0, R - 1) and int(res["start_i"][p]) > 0 and int(res["start_j"][p]) > 0
    p, w = walk("stop_row0")
    assert int(res["start_i"][p]) == 0 and int(res["start_j"][p]) > 0
    p, w = walk("stop_col0")
    assert int(res["start_j"][p]) == 0 and int(res["start_i"][p]) > 0


@pytest.mark.parametrize("lp", ["4", "8"])
@pytest.mark.parametrize("R", [32, 16])
def test_nw_walks(engine, R, lp):
    """Needleman-Wunsch on the same batches: the L run from row 20 (columns 21 .. 180: blocks without a
    left snapshot, and at R = 16 blocks that start left of column 0), walks that reach column 0 or
    row 0 far from (0, 0) and finish on the border."""
    so = check(engine, R, lp, 1, NW)
    s1, o1, s2, o2, at = batch(R)
    res, ops = so[0], so[1]

    def walk(name):
        p = at[name]
        off = int(o1[p] + o2[p]) + p
        return ops[off:off + int(res["nops"][p])].tobytes()

    assert b"U" * 100 in walk("deleted_run")
    w = walk("inserted_run_row20")
    assert b"L" * 128 in w and sum(c in b"MSXU" for c in w[w.index(b"L" * 128):]) <= 21
    assert b"L" * 128 in walk("inserted_run_row300")
    assert walk("border_col0").endswith(b"U" * 100)
    assert walk("border_row0").endswith(b"L" * 100)
    assert walk("border_col0_long").endswith(b"U" * 100)
    assert (res["start_i"] == 0).all() and (res["start_j"] == 0).all()


@pytest.mark.parametrize("lp", ["4", "8"])
@pytest.mark.parametrize("algo,scoring,lut", [(0, (-2, 2, -3), None), (0, (-2, 1, -1, False), None), (0, SW, AG_CT),
                                              (1, (-2, 2, -3), None), (1, (-2, 1, -1, False), None), (1, NW, AG_CT)],
                         ids=["sw-2,2,-3", "sw-no-mismatch", "sw-table", "nw-2,2,-3", "nw-no-mismatch", "nw-table"])
def test_other_scorings_and_match_table(engine, algo, scoring, lut, lp):
    """A non-default scoring of tests/test_gpu_so.py, !AllowMismatch, and a non-identity match table
    (A~G, C~T), on the R = 16 batch."""
    check(engine, 16, lp, algo, scoring, lut)
