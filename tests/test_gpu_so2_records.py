"""The two-pairs-per-wave fill (sa_fill_so2.hip) with its unit column table in LDS -- each lane reads
its column's table words {A, B} at every step, where they used to travel down the lanes by DPP -- and
the f16 cells' chunk maximum in one packed maximum3: every pair's result and op stream against the
16-bit integer cell (SEQALIB_SO2_F16=0) and against the full-matrix oracle.

The table holds the columns [32 c0 - 64, 32 c1) of a unit (chunks [c0, c1) of a band): 0 left of
column 0, the out-of-matrix word from a pair's n on.  The host gives the room when the widest unit
range of the launch is at most 1,024 columns (8 KiB); wider ranges, and SEQALIB_SO2_TAB=0, keep the
DPP path.  With max_n = 2,100 (the R = 16 batch) 3 and 8 segments per band take the table (23 and
9 chunks per unit) and 1 segment the DPP path; with max_n = 4,148 (R = 32) 8 segments take the
table; the `short` batch (n <= 800) takes it at every count, with 1 segment for unit ranges that
start at column 0 and hold a whole band.
Reference semantics: SASmithWaterman.h:89-117 (fill), :220-339 (traceback); SANeedlemanWunsch.h:69-86.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from test_gpu_so import FIELDS, NW, SW, THREADS, assert_same, run
from util import oracle_batch, pack_bytes

pytestmark = pytest.mark.gpu
BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def related(rng, a, rate=0.02, head=0):
    """A copy of a with `rate` substitutions, its first `head` symbols random."""
    b = a.copy()
    mut = rng.random(len(b)) < rate
    mut[:head] = True
    b[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
    return b


def ragged_couples(seed, band, top, npairs=201, big=0):
    """Pairs (2k, 2k + 1) share a wave; `band` rows per band (64 R).  Forced couples first: halves that
    differ in bands and in chunks per band, ramp-only columns (n < 64), n = 1 and 31 mod 32, m one
    over a band, 1 x 1; then random m, n in [1, top] (`big` of them near 2 `band` + 52: just over two
    bands), one pair in four a 2 % mutated copy.  An odd count: the last couple is a lone pair."""
    rng = np.random.default_rng(seed)
    forced = [(band + 1, 700), (300, 2 * band + 52), (2 * band + 52, 40), (band, band + 33), (1, 1), (band + 1, 1),
              (700, 63), (63, 700), (band + 1, 33), (513, 31 + 32 * 9), (band - 1, 65), (2 * band + 1, 95),
              (5, top), (top, 5), (band + 1, band + 1), (band, 64)]
    pairs = []
    for p in range(npairs):
        if p < len(forced):
            m, n = forced[p]
        elif p < len(forced) + big:
            m, n = 2 * band + 52 - int(rng.integers(0, 40)), 2 * band + 52 - int(rng.integers(0, 40))
        else:
            m, n = int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))
        a = ACGT[rng.integers(0, 4, m)]
        if p % 4 == 3 and p >= len(forced):
            b = related(rng, a)[:n]
        else:
            b = ACGT[rng.integers(0, 4, n)]
        pairs.append((a.tobytes(), b.tobytes()))
    assert npairs % 2 == 1
    return pack_bytes(pairs)


class Case:
    """A batch and, computed once, the full-matrix oracle's results and op streams of every pair."""

    def __init__(self, batch, algo=0, scoring=SW):
        self.batch, self.algo, self.scoring = batch, algo, scoring
        self.ores, self.oops = oracle_batch(algo, scoring, *batch, threads=THREADS)

    def check(self, got):
        """Every pair of an engine run against the oracle."""
        s1, o1, s2, o2 = self.batch
        res, ops, _ = got
        for f in FIELDS[:5]:
            bad = np.nonzero(res[f] != self.ores[f])[0]
            assert len(bad) == 0, (f, [(int(p), int(res[f][p]), int(self.ores[f][p])) for p in bad[:5]])
        bad = np.nonzero(res["nops"] != self.ores["nops"])[0]
        assert len(bad) == 0, ("nops", bad[:5].tolist())
        for p in range(len(o1) - 1):
            s, k = int(o1[p] + o2[p]) + p, int(res["nops"][p])
            assert ops[s:s + k].tobytes() == self.oops[s:s + k].tobytes(), f"op stream of pair {p}"


@pytest.fixture(scope="module")
def ragged16():
    return Case(ragged_couples(301, 1024, 2100))


@pytest.fixture(scope="module")
def ragged32():
    # (R = 32: 2,048 rows per band; most pairs stay below 2,100, a handful run to 4,148)
    return Case(ragged_couples(302, 2048, 2100, big=5))


@pytest.fixture(scope="module")
def short():
    return Case(ragged_couples(303, 256, 800, npairs=101))


def both_cells(engine, monkeypatch, case, R):
    """The batch on the default (4-op f16) cell and on the 16-bit cell: the same, and the oracle's."""
    o1, o2 = case.batch[1], case.batch[3]
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    a = run(engine, True, *case.batch, scoring=case.scoring, algo=case.algo)
    monkeypatch.setenv("SEQALIB_SO2_F16", "0")
    b = run(engine, True, *case.batch, scoring=case.scoring, algo=case.algo)
    monkeypatch.delenv("SEQALIB_SO2_F16")
    assert a[2][1] == R and b[2] == a[2]
    assert (a[0]["flags"] == 0).all()
    assert_same(a, b, o1, o2)
    case.check(a)
    return a


@pytest.fixture
def f16_on(engine):
    engine.test_hook(sa.SA_HOOK_F16, 0)
    yield
    engine.test_hook(sa.SA_HOOK_F16, 0)


@pytest.mark.parametrize("R", [16, 32])
def test_ragged_couples(engine, monkeypatch, f16_on, ragged16, ragged32, R):
    case = ragged16 if R == 16 else ragged32
    a = both_cells(engine, monkeypatch, case, R)
    assert a[2] == (sa.SA_KERNEL_T16_ENDCELL, R, 1)
    monkeypatch.setenv("SEQALIB_SO2_F16", "5")   # the 5-op f16 cell shares the table and the maximum3
    assert_same(a, run(engine, True, *case.batch), case.batch[1], case.batch[3])


@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("segs", ["1", "3", "8"])
def test_table_edges(engine, monkeypatch, f16_on, ragged16, ragged32, short, R, segs):
    """Unit column ranges that start at 0, mid-band and near the end."""
    monkeypatch.setenv("SEQALIB_SO_SEGS", segs)
    both_cells(engine, monkeypatch, ragged16 if R == 16 else ragged32, R)
    both_cells(engine, monkeypatch, short, R)


@pytest.mark.parametrize("R", [16, 32])
def test_no_table_fallback(engine, monkeypatch, f16_on, ragged16, ragged32, R):
    """SEQALIB_SO2_TAB=0: the column words by DPP, byte for byte the table's results."""
    case = ragged16 if R == 16 else ragged32
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    a = run(engine, True, *case.batch)
    monkeypatch.setenv("SEQALIB_SO2_TAB", "0")
    b = both_cells(engine, monkeypatch, case, R)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("R", [16, 32])
def test_nw(engine, monkeypatch, ragged16, ragged32, R):
    """The same ragged batch through fill_so2_kernel<SA_NW>: the table, the DPP path and one pair per
    wave agree, and match the oracle."""
    src = ragged16 if R == 16 else ragged32
    case = Case(src.batch, algo=1, scoring=NW)
    o1, o2 = case.batch[1], case.batch[3]
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    a = run(engine, True, *case.batch, scoring=NW, algo=1)
    assert a[2][1] == R and (a[0]["flags"] == 0).all()
    case.check(a)
    monkeypatch.setenv("SEQALIB_SO2_TAB", "0")
    assert_same(a, run(engine, True, *case.batch, scoring=NW, algo=1), o1, o2)
    monkeypatch.delenv("SEQALIB_SO2_TAB")
    monkeypatch.setenv("SEQALIB_SO2", "0")
    assert_same(a, run(engine, True, *case.batch, scoring=NW, algo=1), o1, o2)


def high_batch(seed, band, npairs=65):
    """Related pairs whose band >= 1 holds values in [1024, 2048): m = band + 950 .. band + 1,150 rows,
    the second sequence a 2 % mutated copy whose first band - 750 symbols are random, so the local
    path (1,700 .. 1,900 symbols, score ~ 0.94 of that) ends in band 1.  First, identical pairs of
    2,005 .. 2,500 symbols: above the f16 cell's retry threshold (2,000).  The rest random."""
    rng = np.random.default_rng(seed)
    over = [2005, 2047, 2048, 2100, 2500]
    pairs, rel = [], []
    for p in range(npairs):
        if p < len(over):
            a = ACGT[rng.integers(0, 4, over[p])]
            b = a
        elif p % 2 == 0:
            a = ACGT[rng.integers(0, 4, band + int(rng.integers(950, 1151)))]
            b = related(rng, a, head=band - 750)
            rel.append(p)
        else:
            a = ACGT[rng.integers(0, 4, int(rng.integers(1, band + 1100)))]
            b = ACGT[rng.integers(0, 4, int(rng.integers(1, band + 1100)))]
        pairs.append((a.tobytes(), b.tobytes()))
    return pack_bytes(pairs), over, rel


@pytest.mark.parametrize("R", [16, 32])
def test_high_scores(engine, monkeypatch, f16_on, R):
    batch, over, rel = high_batch(310 + R, 64 * R)
    case = Case(batch)
    a = both_cells(engine, monkeypatch, case, R)   # (flags 0: the pairs above 2,000 re-ran in int32)
    assert a[2] == (sa.SA_KERNEL_T16_ENDCELL, R, 1)
    sc = a[0]["score"]
    assert [int(x) for x in sc[:len(over)]] == over
    assert (sc[rel] >= 1400).all() and (sc[rel] < 2000).all(), sc[rel]
    assert (a[0]["end_i"][rel] > 64 * R).all()   # (the path's end, its largest values, in band 1)


@pytest.mark.parametrize("R", [16, 32])
def test_cell_switch(engine, monkeypatch, f16_on, ragged16, ragged32, short, R):
    """One context, the cell switched between launches (SA_HOOK_F16): f16, 16-bit, f16 again on
    another batch, 16-bit on it -- every launch is read as the cell it ran wrote it."""
    case = ragged16 if R == 16 else ragged32
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    a = run(engine, True, *case.batch)
    engine.test_hook(sa.SA_HOOK_F16, 1)
    b = run(engine, True, *case.batch)
    c = run(engine, True, *short.batch)
    engine.test_hook(sa.SA_HOOK_F16, 0)
    d = run(engine, True, *short.batch)
    e = run(engine, True, *case.batch)
    case.check(a)
    short.check(d)
    assert_same(a, b, case.batch[1], case.batch[3])
    assert_same(a, e, case.batch[1], case.batch[3])
    assert_same(c, d, short.batch[1], short.batch[3])
