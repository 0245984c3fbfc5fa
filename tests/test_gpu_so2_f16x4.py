"""The 4-op scaled-f16 cell of the two-pairs-per-wave Smith-Waterman fill (sa_fill_so2.hip X4: H / 2048
and F = max(H + Gap, 0) / 2048 per row) against the 5-op f16 cell (SEQALIB_SO2_F16=5), the 16-bit
integer cell (SEQALIB_SO2_F16=0) and the oracle.

Multi-band couples are the shape on which an earlier build of this cell got the high half (pair B)
of bands >= 1 wrong, by different amounts from run to run: ragged pairs of 1, 2 and 3 bands at
R = 16 (1 and 2 at R = 32), couples whose halves have different band counts, several column
segments, related pairs whose band >= 1 carries values in [1024, 2048), the same batch three times.
The threshold tests pin the flag / int32 re-run at scorings other than (-1, 1, -1).
Reference semantics: SASmithWaterman.h:89-117 (fill), :220-339 (traceback).
"""
import numpy as np
import pytest

import seqalib_amd as sa
from test_gpu_so import SW, assert_same, check_vs_oracle, identical_pairs_batch, run

pytestmark = pytest.mark.gpu
BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def pack(pairs):
    o1 = np.zeros(len(pairs) + 1, np.uint64)
    o2 = np.zeros(len(pairs) + 1, np.uint64)
    o1[1:] = np.cumsum([len(a) for a, _ in pairs])
    o2[1:] = np.cumsum([len(b) for _, b in pairs])
    s1 = np.frombuffer(b"".join(a for a, _ in pairs), np.uint8).copy()
    s2 = np.frombuffer(b"".join(b for _, b in pairs), np.uint8).copy()
    return s1, o1, s2, o2


def multiband_batch(seed=77, npairs=201):
    """Pairs (2k, 2k + 1) share a wave.  m, n in [600, 2300]: 1, 2 or 3 bands of 1,024 rows at
    R = 16.  First the forced couples (A | B rows): more bands in A, more in B, equal; then, one pair
    in three, a 2 % mutated copy of 1,500 .. 1,950 symbols (score ~ 0.96 length: the rows of its
    second band hold values in [1024, 2048)); the rest random.  An odd count: the last couple has
    one pair."""
    rng = np.random.default_rng(seed)
    forced = [m for couple in [(2300, 700), (700, 2300), (2300, 1500), (1100, 2200), (2049, 1024), (1024, 2049),
                               (1025, 1025), (2048, 2048), (600, 2300), (2300, 2300)] for m in couple]
    pairs, related = [], []
    for p in range(npairs):
        if p < len(forced):
            m, n = forced[p], int(rng.integers(600, 2301))
        else:
            m, n = int(rng.integers(600, 2301)), int(rng.integers(600, 2301))
        if p >= len(forced) and p % 3 == 0:
            m = int(rng.integers(1500, 1951))
            a = ACGT[rng.integers(0, 4, m)]
            b = a.copy()
            mut = rng.random(m) < 0.02
            b[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
            related.append(p)
        else:
            a = ACGT[rng.integers(0, 4, m)]
            b = ACGT[rng.integers(0, 4, n)]
        pairs.append((a.tobytes(), b.tobytes()))
    return pack(pairs), related


@pytest.fixture(scope="module")
def multiband():
    return multiband_batch()


@pytest.mark.parametrize("R", [16, 32])
def test_x4_multiband_couples(engine, monkeypatch, multiband, R):
    batch, related = multiband
    s1, o1, s2, o2 = batch
    engine.test_hook(sa.SA_HOOK_F16, 0)
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    try:
        runs = [run(engine, True, *batch) for _ in range(3)]   # the 4-op cell, three times
        monkeypatch.setenv("SEQALIB_SO2_F16", "5")
        f5 = run(engine, True, *batch)
        monkeypatch.setenv("SEQALIB_SO2_F16", "0")
        i16 = run(engine, True, *batch)
        monkeypatch.delenv("SEQALIB_SO2_F16")
        for r in runs + [f5, i16]:
            assert r[2] == (sa.SA_KERNEL_T16_ENDCELL, R, 1)
            assert (r[0]["flags"] == 0).all()
        sc = runs[0][0]["score"]
        # the related pairs are the ones whose later bands carry values in [1024, 2048)
        assert (sc[related] >= 1300).all() and (sc[related] < 1994).all(), sc[related]
        for r in runs[1:]:
            assert runs[0][0].tobytes() == r[0].tobytes() and runs[0][1].tobytes() == r[1].tobytes()
        assert_same(runs[0], i16, o1, o2)
        assert_same(runs[0], f5, o1, o2)
        idx = list(range(0, 20, 3)) + related[:4] + [len(o1) - 2]
        check_vs_oracle(0, SW, runs[0], batch, idx)
    finally:
        engine.test_hook(sa.SA_HOOK_F16, 0)


# identical pairs whose scores (match * length) straddle 2,000 (the retry threshold) and 2,048 (the
# end of the exact range), per scoring (gap, match, mismatch)
THRESHOLD = [
    ((-1, 1, -1), [1990, 1994, 1999, 2001, 2040, 2047, 2048, 2049, 2100]),
    ((-2, 2, -3), [990, 997, 999, 1000, 1001, 1020, 1023, 1024, 1025, 1050]),
    ((-8, 8, -8), [240, 248, 249, 250, 251, 255, 256, 257, 262]),
    ((-16, 4, -4), [470, 498, 499, 500, 501, 511, 512, 513, 525]),
]


@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("scoring,lengths", THRESHOLD)
def test_x4_threshold_scorings(engine, monkeypatch, scoring, lengths, R):
    """Exact against the 16-bit cell and the oracle, flags 0 after the in-call int32 re-run; the few
    flagged pairs of 1,100 leave the f16 cell on."""
    engine.test_hook(sa.SA_HOOK_F16, 0)
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    try:
        batch = identical_pairs_batch(17 + scoring[1], 1100, lengths, maxlen=900)
        s1, o1, s2, o2 = batch
        a = run(engine, True, *batch, scoring=scoring)
        monkeypatch.setenv("SEQALIB_SO2_F16", "0")
        b = run(engine, True, *batch, scoring=scoring)
        monkeypatch.delenv("SEQALIB_SO2_F16")
        assert a[2] == (sa.SA_KERNEL_T16_ENDCELL, R, 1) and b[2] == a[2]
        assert (a[0]["flags"] == 0).all()
        assert [int(x) for x in a[0]["score"][:len(lengths)]] == [scoring[1] * n for n in lengths]
        assert_same(a, b, o1, o2)
        check_vs_oracle(0, scoring, a, batch, list(range(len(lengths))) + [500, 1099])
        run(engine, True, *batch, scoring=scoring)
        assert engine.test_hook(sa.SA_HOOK_F16, 2) == 0
    finally:
        engine.test_hook(sa.SA_HOOK_F16, 0)


@pytest.mark.parametrize("R", [16, 32])
def test_x4_large_gap_every_pair_reruns(engine, monkeypatch, R):
    """Gap -400: (sampled maximum - 6 Gap) > 2,000 for every pair, so each takes the int32 re-run
    (exact results, flags 0) and the launch turns the f16 cell off for the context."""
    scoring = (-400, 8, -8)
    lengths = [100, 240, 250, 256, 257, 300, 700]
    engine.test_hook(sa.SA_HOOK_F16, 0)
    monkeypatch.setenv("SEQALIB_PLAN", f"{R},1")
    try:
        batch = identical_pairs_batch(23, 1100, lengths, maxlen=900)
        s1, o1, s2, o2 = batch
        a = run(engine, True, *batch, scoring=scoring)
        monkeypatch.setenv("SEQALIB_SO2_F16", "0")
        b = run(engine, True, *batch, scoring=scoring)
        monkeypatch.delenv("SEQALIB_SO2_F16")
        assert a[2] == (sa.SA_KERNEL_T16_ENDCELL, R, 1) and b[2] == a[2]
        assert (a[0]["flags"] == 0).all()
        assert [int(x) for x in a[0]["score"][:len(lengths)]] == [8 * n for n in lengths]
        assert_same(a, b, o1, o2)
        check_vs_oracle(0, scoring, a, batch, list(range(len(lengths))) + [500, 1099])
        assert engine.test_hook(sa.SA_HOOK_F16, 2) == 1
    finally:
        engine.test_hook(sa.SA_HOOK_F16, 0)
