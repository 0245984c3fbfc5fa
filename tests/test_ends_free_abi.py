"""CPU: the ends-free banded entry points (sa_align_batch_banded_ends_free,
sa_score_batch_banded_ends_free, include/seqalib_hip.h) are exported and every status rule answers
without a context: the algorithm classes, free_ends, and the band, scoring and pair limits of the two
banded calls they build on, at their edges.  No GPU compute is called here."""
import ctypes as C

import numpy as np
import pytest

import seqalib_amd as sa

SYMBOLS = ["sa_align_batch_banded_ends_free", "sa_score_batch_banded_ends_free"]
LINEAR_ALGS = [sa.SA_NW, sa.SA_HIRSCHBERG]
ALGS = LINEAR_ALGS + [sa.SA_GLOBAL_GOTOH]
FIT = 12   # SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END


def test_symbols_exported():
    L = sa.load_library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert (sa.SA_FREE_SEQ1_BEGIN, sa.SA_FREE_SEQ1_END, sa.SA_FREE_SEQ2_BEGIN, sa.SA_FREE_SEQ2_END) == (1, 2, 4, 8)
    assert L.sa_version() == 1   # the change only adds symbols


def _calls(L):
    def align(ctx, algo, sc, band, fe, o1=None, o2=None, npairs=0):
        return L.sa_align_batch_banded_ends_free(ctx, algo, sc, None, o1, None, o2, npairs, None, band, fe, None, None, 0)

    def score(ctx, algo, sc, band, fe, o1=None, o2=None, npairs=0):
        return L.sa_score_batch_banded_ends_free(ctx, algo, sc, None, o1, None, o2, npairs, None, band, fe, None)

    return align, score


def test_argument_checks_need_no_context():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for call in _calls(L):
        for algo in ALGS:
            sc = aff if algo == sa.SA_GLOBAL_GOTOH else lin
            nomis = (sa.ScoringSystem(-3, -1, 2, -1, False) if algo == sa.SA_GLOBAL_GOTOH else sa.ScoringSystem(-1, 2))._c()
            for fe in range(16):
                assert call(None, algo, C.byref(sc), 4, fe) == -1          # only the context is missing
            assert call(None, algo, C.byref(sc), 4, 16) == -1              # free_ends outside SA_FREE_*
            assert call(None, algo, C.byref(sc), 4, 2 ** 32 - 1) == -1
            assert call(None, algo, None, 4, FIT) == -1                    # NULL scoring
            assert call(None, algo, C.byref(nomis), 0, FIT) == -5          # one diagonal, no mismatches
            assert call(None, algo, C.byref(nomis), 1, FIT) == -1
            assert call(None, algo, C.byref(sc), 2 ** 31, FIT) == -1       # B overflows 32 bits: SA_ERR_ARG
            assert call(None, algo, C.byref(sc), 2 ** 32 - 1, FIT) == -1
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(sa.ScoringSystem(-3, 1, 1, -1)._c()), 4, FIT) == -5   # gap_extend > 0
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(sa.ScoringSystem(3, 0, 1, -1)._c()), 4, FIT) == -1    # gap_open of any sign
        for algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH, sa.SA_MYERS_MILLER):
            assert call(None, algo, C.byref(aff), 4, FIT) == -5
            assert call(None, algo, C.byref(aff), 4, 0) == -5
        for algo in (-1, 6, 9):
            assert call(None, algo, C.byref(aff), 4, FIT) == -1
        # a free_ends that is out of range is a bad argument whatever the algorithm's class
        assert call(None, sa.SA_SW, C.byref(lin), 4, 16) == -1


def _offsets(m, n):
    return (np.array([0, m], dtype=np.uint64), np.array([0, n], dtype=np.uint64))


def _status(L, algo, sc, m, n, band, fe=FIT):
    o1, o2 = _offsets(m, n)
    out = {call(None, algo, C.byref(sc), band, fe, o1.ctypes.data, o2.ctypes.data, 1) for call in _calls(L)}
    assert len(out) == 1
    return out.pop()


@pytest.mark.parametrize("algo", LINEAR_ALGS)
def test_linear_pair_limits_need_no_context(algo):
    """The limits of sa_align_batch_banded with SA_NW, read from the offsets alone: -5 where a valid pair
    answers -1."""
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    assert _status(L, algo, lin, 100, 100, 4) == -1
    # (m + n + 1) * max(|gap|, |match|, |mismatch|) >= 2^29 at its edge: 2^29 = 1024 * 524288
    for sc in [sa.ScoringSystem(-1, 1024, -1), sa.ScoringSystem(-1, 1, -1024), sa.ScoringSystem(-1024, 1, -1),
               sa.ScoringSystem(1024, 1, -1)]:
        assert _status(L, algo, sc._c(), 262144, 262143, 4) == -5, sc.args()
        assert _status(L, algo, sc._c(), 262143, 262143, 4) == -1, sc.args()
    off = sa.ScoringSystem(-1, 1, -1024, False)._c()
    assert _status(L, algo, off, 262144, 262143, 4) == -1     # mismatch counted only when allowed
    assert _status(L, algo, lin, 2 ** 24, 100, 4) == -5       # a sequence of >= 2^24 symbols
    assert _status(L, algo, lin, 100, 2 ** 24, 4) == -5
    assert _status(L, algo, lin, 2048, 2048, 8192) == -5      # 4097 diagonals inside the matrix
    assert _status(L, algo, lin, 2048, 2047, 8192) == -1      # 4096
    assert _status(L, algo, lin, 150, 5000, 16) == -5         # a fit whose window is too long: 4883 diagonals
    assert _status(L, algo, lin, 150, 4000, 16) == -1         # 3883
    # no (m + 1) * diagonals < 2^31 limit: the end-cell search orders candidates by position
    assert (2 ** 21 + 10001) * 1021 >= 2 ** 31
    for fe in (0, FIT, 15):
        assert _status(L, algo, lin, 2 ** 21 + 10000, 2 ** 21 + 11000, 10, fe) == -1


def test_affine_pair_limits_need_no_context():
    """The limits of sa_align_batch_banded_affine with SA_GLOBAL_GOTOH."""
    L = sa.load_library()
    algo = sa.SA_GLOBAL_GOTOH
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    assert _status(L, algo, aff, 100, 100, 4) == -1
    # (m + n + 1) * max(|open| + |extend|, |match|, |mismatch|) + 10000 >= 2^29 at its edge (as
    # tests/test_banded_affine_abi.py)
    assert 536861 * 1000 < 2 ** 29 <= 536861 * 1000 + 10000 and 536860 * 1000 + 10000 < 2 ** 29
    for sc in [sa.ScoringSystem(-3, -1, 1000, -1), sa.ScoringSystem(-3, -1, 1, -1000), sa.ScoringSystem(-600, -400, 1, -1),
               sa.ScoringSystem(1000, 0, 1, -1)]:
        assert _status(L, algo, sc._c(), 268430, 268430, 4) == -5, sc.args()
        assert _status(L, algo, sc._c(), 268430, 268429, 4) == -1, sc.args()
    off = sa.ScoringSystem(-3, -1, 1, -1000, False)._c()
    assert _status(L, algo, off, 268430, 268430, 4) == -1     # mismatch counted only when allowed
    assert _status(L, algo, aff, 2 ** 24, 100, 4) == -5       # a sequence of >= 2^24 symbols
    assert _status(L, algo, aff, 100, 2 ** 24, 4) == -5
    assert _status(L, algo, aff, 1024, 1024, 4096) == -5      # 2049 diagonals inside the matrix
    assert _status(L, algo, aff, 1024, 1023, 4096) == -1      # 2048
    assert _status(L, algo, aff, 100, 3000, 4) == -5          # 2909 diagonals
    assert (2 ** 21 + 10001) * 1021 >= 2 ** 31
    for fe in (0, FIT, 15):
        assert _status(L, algo, aff, 2 ** 21 + 10000, 2 ** 21 + 11000, 10, fe) == -1


def test_python_doors_raise_where_there_is_no_ends_free_form():
    pairs = [(b"ACGT", b"ACGT")]
    for cls in (sa.SmithWatermanSA, sa.LocalGotohSA, sa.MyersMillerSA):
        for door in ("getEndsFreeAlignments", "getEndsFreeScores", "getEndsFreeEndCells"):
            with pytest.raises(sa.SeqalibError):
                getattr(cls(), door)(pairs, 4, FIT)
    m = sa.SubstitutionMatrix(b"ACGT", np.eye(4, dtype=np.int16))
    for cls in (sa.NeedlemanWunschSA, sa.GlobalGotohSA):
        with pytest.raises(sa.SeqalibError):
            cls(matrix=m).getEndsFreeAlignments(pairs, 4, FIT)
        with pytest.raises(sa.SeqalibError):
            cls(matrix=m).getEndsFreeScores(pairs, 4, FIT)
