"""CPU: the banded entry points (sa_align_batch_banded, sa_score_batch_banded, sa_banded_plan_query,
include/seqalib_hip.h) are exported, the host-only planner sizes a pair's records linearly in
(m + n) * B, and the argument checks that need no device answer.  No GPU compute is called here."""
import ctypes as C

import pytest

import seqalib_amd as sa

BANDED_SYMBOLS = ["sa_align_batch_banded", "sa_score_batch_banded", "sa_banded_plan_query"]
# sa_banded_plan_query: a variant's capacity is at least 32 diagonals of 2 bits per step, rounded up
# to whole 32-bit words per lane, plus the steps before the first cell -- far below this constant
PLAN_CONSTANT = 4096


def test_banded_symbols_exported():
    L = sa.load_library()
    missing = [s for s in BANDED_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert (sa.SA_KERNEL_BANDED, sa.SA_RECORDS_BAND2) == (4, 4)
    assert L.sa_version() == 1   # the change only adds symbols


def test_banded_plan_is_linear():
    m = n = 16384
    w = 64
    B = abs(n - m) + 2 * w + 1
    R, ppw, ws = sa.banded_plan_query(sa.SA_NW, m, n, w, 100)
    full = sa.plan_query_ex(sa.SA_NW, sa.ScoringSystem(-1, 1, -1), m, n, 100, nsym=20)[3]
    print(f"banded: R {R}, {ppw} pairs per wave, {ws} B/pair; full: {full} B/pair")
    assert ppw == 2 and 2 * R * (64 // ppw) >= B
    assert ws <= 4 * (m + n) * B // 4 + PLAN_CONSTANT
    assert ws * 16 <= full


@pytest.mark.parametrize("algo", [sa.SA_NW, sa.SA_SW, sa.SA_HIRSCHBERG])
def test_banded_plan_grows_with_the_band_not_the_matrix(algo):
    for w in (0, 8, 64, 256, 1000):
        B = 2 * w + 1
        for m in (1000, 4096, 16384):
            R, ppw, ws = sa.banded_plan_query(algo, m, m, w)
            assert 2 * R * (64 // ppw) >= B
            assert ws <= max(2 * B, 32) * (2 * m + w + 2) // 4 + PLAN_CONSTANT, (w, m)
    assert sa.banded_plan_query(algo, 700, 650, 4096)[0] == 16   # clipped to the matrix: 1351 diagonals
    with pytest.raises(sa.SeqalibError):
        sa.banded_plan_query(algo, 5000, 5000, 4096)              # > 4096 diagonals inside the matrix


def test_banded_argument_checks():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    nomis = sa.ScoringSystem(-1, 2)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()

    def align(ctx, algo, sc, band):
        return L.sa_align_batch_banded(ctx, algo, sc, None, None, None, None, 0, None, band, None, None, 0)

    def score(ctx, algo, sc, band):
        return L.sa_score_batch_banded(ctx, algo, sc, None, None, None, None, 0, None, band, None)

    for call in (align, score):
        assert call(None, sa.SA_NW, C.byref(lin), 4) == -1              # NULL context
        assert call(None, sa.SA_NW, None, 4) == -1                      # NULL scoring
        assert call(None, 9, C.byref(lin), 4) == -1
        for algo in (sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH, sa.SA_MYERS_MILLER):
            assert call(None, algo, C.byref(aff), 4) == -5              # SA_ERR_UNSUPPORTED
        assert call(None, sa.SA_NW, C.byref(nomis), 0) == -5            # one diagonal, no mismatches
        assert call(None, sa.SA_SW, C.byref(nomis), 1) == -1            # (fine: only the context is missing)
        assert call(None, sa.SA_NW, C.byref(lin), 2 ** 31) == -1        # B overflows 32 bits: SA_ERR_ARG
        assert call(None, sa.SA_NW, C.byref(lin), 2 ** 32 - 1) == -1
    assert L.sa_banded_plan_query(sa.SA_NW, 100, 100, 2 ** 31, 1, None, None, None) == -1
    assert L.sa_banded_plan_query(sa.SA_GLOBAL_GOTOH, 100, 100, 4, 1, None, None, None) == -5
    assert L.sa_banded_plan_query(sa.SA_NW, 2 ** 24, 100, 4, 1, None, None, None) == -5
