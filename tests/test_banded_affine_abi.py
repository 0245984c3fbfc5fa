"""CPU: the banded affine entry points (sa_align_batch_banded_affine, sa_score_batch_banded_affine,
sa_banded_affine_plan_query, include/seqalib_hip.h) are exported, every status rule answers without a
context, and the host-only planner sizes a pair's 4-bit records linearly in (m + n) * B.  No GPU
compute is called here."""
import ctypes as C

import numpy as np
import pytest

import seqalib_amd as sa

SYMBOLS = ["sa_align_batch_banded_affine", "sa_score_batch_banded_affine", "sa_banded_affine_plan_query"]
ALGS = [sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH]
PLAN_CONSTANT = 4096     # as tests/test_banded_abi.py: word rounding and the steps before the first cell
MAX_DIAGONALS = 2048     # the limit the header states: 16 cells per lane and step, 64 lanes, two parities


def test_symbols_exported():
    L = sa.load_library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert sa.SA_RECORDS_BAND4 == 5
    assert L.sa_version() == 1   # the change only adds symbols


def _calls(L):
    def align(ctx, algo, sc, band, o1=None, o2=None, npairs=0):
        return L.sa_align_batch_banded_affine(ctx, algo, sc, None, o1, None, o2, npairs, None, band, None, None, 0)

    def score(ctx, algo, sc, band, o1=None, o2=None, npairs=0):
        return L.sa_score_batch_banded_affine(ctx, algo, sc, None, o1, None, o2, npairs, None, band, None)

    return align, score


def test_argument_checks_need_no_context():
    L = sa.load_library()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    nomis = sa.ScoringSystem(-3, -1, 2, -1, False)._c()
    for call in _calls(L):
        for algo in ALGS:
            assert call(None, algo, C.byref(aff), 4) == -1                 # only the context is missing
            assert call(None, algo, None, 4) == -1                         # NULL scoring
            assert call(None, algo, C.byref(sa.ScoringSystem(-3, 1, 1, -1)._c()), 4) == -5    # gap_extend > 0
            assert call(None, algo, C.byref(sa.ScoringSystem(3, 0, 1, -1)._c()), 4) == -1     # gap_open of any sign
            assert call(None, algo, C.byref(nomis), 0) == -5               # one diagonal, no mismatches
            assert call(None, algo, C.byref(nomis), 1) == -1
            assert call(None, algo, C.byref(aff), 2 ** 31) == -1           # B overflows 32 bits: SA_ERR_ARG
            assert call(None, algo, C.byref(aff), 2 ** 32 - 1) == -1
        for algo in (sa.SA_SW, sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_MYERS_MILLER):
            assert call(None, algo, C.byref(aff), 4) == -5
        for algo in (-1, 6, 9):
            assert call(None, algo, C.byref(aff), 4) == -1


def _offsets(m, n):
    return (np.array([0, m], dtype=np.uint64), np.array([0, n], dtype=np.uint64))


@pytest.mark.parametrize("algo", ALGS)
def test_pair_limits_need_no_context(algo):
    """The per-pair limits read the offsets only, so they too answer -5 where a valid pair answers -1."""
    L = sa.load_library()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()

    def status(sc, m, n, band):
        o1, o2 = _offsets(m, n)
        out = {call(None, algo, C.byref(sc), band, o1.ctypes.data, o2.ctypes.data, 1) for call in _calls(L)}
        assert len(out) == 1
        return out.pop()

    assert status(aff, 100, 100, 4) == -1
    # (m + n + 1) * max(|open| + |extend|, |match|, |mismatch|) + 10000 >= 2^29, at its edge: with
    # 1000 as the largest term the bound is m + n + 1 >= 536861 (536861000 alone is still below 2^29,
    # so this also pins the constant)
    assert 536861 * 1000 < 2 ** 29 <= 536861 * 1000 + 10000 and 536860 * 1000 + 10000 < 2 ** 29
    for sc in [sa.ScoringSystem(-3, -1, 1000, -1), sa.ScoringSystem(-3, -1, 1, -1000), sa.ScoringSystem(-600, -400, 1, -1),
               sa.ScoringSystem(1000, 0, 1, -1)]:
        assert status(sc._c(), 268430, 268430, 4) == -5, sc.args()
        assert status(sc._c(), 268430, 268429, 4) == -1, sc.args()
    off = sa.ScoringSystem(-3, -1, 1, -1000, False)._c()
    assert status(off, 268430, 268430, 4) == -1       # mismatch counted only when allowed
    assert status(aff, 2 ** 24, 100, 4) == -5         # a sequence of >= 2^24 symbols
    assert status(aff, 100, 2 ** 24, 4) == -5
    assert status(aff, 1024, 1024, 4096) == -5        # 2049 diagonals inside the matrix
    assert status(aff, 1024, 1023, 4096) == -1        # 2048
    assert status(aff, 100, 3000, 4) == -5            # 2909 diagonals
    assert (2 ** 21 + 10001) * 1021 >= 2 ** 31
    lg_big = status(aff, 2 ** 21 + 10000, 2 ** 21 + 11000, 10)  # (m + 1) * 1021 diagonals >= 2^31
    assert lg_big == (-5 if algo == sa.SA_LOCAL_GOTOH else -1)


@pytest.mark.parametrize("algo", ALGS)
def test_plan_is_linear_and_within_four_times_the_linear_plan(algo):
    for w in (0, 8, 64, 256, 500):
        for m, n in [(1000, 1000), (4096, 4096), (16384, 16384), (4096, 4000), (300, 1200)]:
            B = abs(n - m) + 2 * w + 1
            R, ppw, ws = sa.banded_affine_plan_query(algo, m, n, w)
            assert 2 * R * (64 // ppw) >= min(B, m + n + 1)
            assert ws <= 4 * max(B, 32) * (m + n + w + 2) // 4 + PLAN_CONSTANT, (w, m, n)
            assert ws <= 4 * sa.banded_plan_query(sa.SA_NW, m, n, w)[2] + PLAN_CONSTANT, (w, m, n)
    m = n = 16384
    full = sa.plan_query_ex(algo, sa.ScoringSystem(-3, -1, 1, -1), m, n, 100, nsym=20)[3]
    assert sa.banded_affine_plan_query(algo, m, n, 64)[2] * 16 <= full


@pytest.mark.parametrize("algo", ALGS)
def test_plan_query_limits(algo):
    L = sa.load_library()
    assert sa.banded_affine_plan_query(algo, 1024, 1023, 4096)[:2] == (16, 1)    # MAX_DIAGONALS exactly
    assert 1024 + 1023 + 1 == MAX_DIAGONALS
    for m, n, w in [(1024, 1024, 4096), (5000, 5000, 1024), (100, 2200, 20)]:
        assert L.sa_banded_affine_plan_query(algo, m, n, w, 1, None, None, None) == -5
        with pytest.raises(sa.SeqalibError):
            sa.banded_affine_plan_query(algo, m, n, w)
    assert L.sa_banded_affine_plan_query(algo, 100, 100, 2 ** 31, 1, None, None, None) == -1
    assert L.sa_banded_affine_plan_query(algo, 2 ** 24, 100, 4, 1, None, None, None) == -5
    for other in (sa.SA_SW, sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_MYERS_MILLER):
        assert L.sa_banded_affine_plan_query(other, 100, 100, 4, 1, None, None, None) == -5
    assert L.sa_banded_affine_plan_query(7, 100, 100, 4, 1, None, None, None) == -1
