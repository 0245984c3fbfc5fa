"""CPU: the banded matrix entry points (sa_align_batch_banded_matrix, sa_score_batch_banded_matrix,
include/seqalib_hip.h) are exported and bound, and every status rule that needs no device answers
with a NULL context, each with a message in sa_last_error(NULL).  No GPU compute is called here."""
import ctypes as C

import numpy as np
import pytest

import seqalib_amd as sa

SYMBOLS = ["sa_align_batch_banded_matrix", "sa_score_batch_banded_matrix"]
LINEAR = [sa.SA_SW, sa.SA_NW]
AFFINE = [sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH]
ARG, UNSUPPORTED = -1, -5
TABLE = np.zeros((256, 256), dtype=np.int16)
TABLE[:] = -1
np.fill_diagonal(TABLE, 2)


def test_symbols_exported_and_bound():
    L = sa.load_library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert len(L.sa_align_batch_banded_matrix.argtypes) == 14
    assert len(L.sa_score_batch_banded_matrix.argtypes) == 12
    assert L.sa_align_batch_banded_matrix.restype is C.c_int and L.sa_score_batch_banded_matrix.restype is C.c_int
    assert L.sa_version() == 1   # the change only adds symbols
    for name in ("align_banded_matrix_packed", "score_banded_matrix_packed", "align_banded_matrix", "score_banded_matrix"):
        assert callable(getattr(sa.Engine, name))
    for cls in (sa.SmithWatermanSA, sa.NeedlemanWunschSA, sa.LocalGotohSA, sa.GlobalGotohSA):
        for name in ("getBandedMatrixAlignments", "getBandedMatrixAlignment", "getBandedMatrixScores"):
            assert callable(getattr(cls, name)), (cls, name)
        assert hasattr(cls, "getBandedMatrixEndCells") == (cls in (sa.SmithWatermanSA, sa.LocalGotohSA))
    for cls in (sa.HirschbergSA, sa.MyersMillerSA):
        assert not any(hasattr(cls, n) for n in ("getBandedMatrixAlignments", "getBandedMatrixScores", "getBandedMatrixEndCells"))


def _status(L, algo, sc, band, pairs=(), table=TABLE, null_table=False):
    """The status both calls give with a NULL context (they must agree), after checking that a failure
    left a message."""
    s1 = np.frombuffer(b"".join(a for a, _ in pairs), dtype=np.uint8)
    s2 = np.frombuffer(b"".join(b for _, b in pairs), dtype=np.uint8)
    o1 = np.cumsum([0] + [len(a) for a, _ in pairs]).astype(np.uint64)
    o2 = np.cumsum([0] + [len(b) for _, b in pairs]).astype(np.uint64)
    n = len(pairs)
    res = np.zeros(max(n, 1), dtype=sa.RESULT_DTYPE)
    cap = int(o1[-1] + o2[-1]) + n + 1
    ops = np.zeros(cap, dtype=np.uint8)
    scp = None if sc is None else C.byref(sc)
    tab = None if null_table else table.ctypes.data
    p1 = s1.ctypes.data if len(s1) else None
    p2 = s2.ctypes.data if len(s2) else None
    out = set()
    for rc in (L.sa_align_batch_banded_matrix(None, algo, scp, p1, o1.ctypes.data, p2, o2.ctypes.data, n, tab, None, band,
                                              res.ctypes.data, ops.ctypes.data, cap),
               L.sa_score_batch_banded_matrix(None, algo, scp, p1, o1.ctypes.data, p2, o2.ctypes.data, n, tab, None, band,
                                              res.ctypes.data)):
        assert rc != 0
        assert L.sa_last_error(None), (algo, band)
        out.add(rc)
    assert len(out) == 1, out
    return out.pop()


def _lengths(L, algo, sc, band, m, n, table=TABLE):
    """_status for one pair of m x n copies of the symbol 'A' (the limits read lengths and the table)."""
    return _status(L, algo, sc, band, [(b"A" * m, b"A" * n)], table)


def test_argument_checks_need_no_context():
    L = sa.load_library()
    lin = sa.ScoringSystem(-2, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    pair = [(b"ACGT", b"ACT")]
    for algo in LINEAR + AFFINE:
        sc = lin if algo in LINEAR else aff
        assert _status(L, algo, sc, 4, pair) == ARG                       # only the context is missing
        assert _status(L, algo, sc, 4) == ARG                             # (npairs = 0 as well)
        assert _status(L, algo, None, 4, pair) == ARG                     # NULL scoring
        assert _status(L, algo, sc, 4, pair, null_table=True) == ARG      # NULL submat
        assert _status(L, algo, sc, 2 ** 31, pair) == ARG                 # B overflows 32 bits
        assert _status(L, algo, sc, 2 ** 32 - 1, pair) == ARG
        assert _status(L, algo, sc, 2 ** 31 - 1, pair) == ARG             # (valid: the whole matrix)
    for algo in (-1, 6, 9):
        assert _status(L, algo, lin, 4, pair) == ARG
    for algo in (sa.SA_HIRSCHBERG, sa.SA_MYERS_MILLER):
        assert _status(L, algo, lin, 4, pair) == UNSUPPORTED
        assert _status(L, algo, aff, 4, pair) == UNSUPPORTED


def test_band_zero_is_valid_for_every_scoring():
    """allow_mismatch is ignored (mismatches are always allowed), so band = 0 passes every check that
    the banded calls without a table make: only the context is missing."""
    L = sa.load_library()
    pair = [(b"ACGT", b"ACT")]
    for algo in LINEAR:
        assert _status(L, algo, sa.ScoringSystem(-1, 2)._c(), 0, pair) == ARG
    for algo in AFFINE:
        assert _status(L, algo, sa.ScoringSystem(-3, -1, 2, -1, False)._c(), 0, pair) == ARG
    # (the same scorings are rejected by the calls without a table)
    assert L.sa_score_batch_banded(None, sa.SA_NW, C.byref(sa.ScoringSystem(-1, 2)._c()), None, None, None, None, 0, None, 0,
                                   None) == UNSUPPORTED


def test_gap_extend_sign():
    L = sa.load_library()
    pair = [(b"ACGT", b"ACT")]
    for algo in AFFINE:
        assert _status(L, algo, sa.ScoringSystem(-3, 1, 1, -1)._c(), 4, pair) == UNSUPPORTED   # gap_extend = 1
        assert _status(L, algo, sa.ScoringSystem(-3, 0, 1, -1)._c(), 4, pair) == ARG
        assert _status(L, algo, sa.ScoringSystem(3, -1, 1, -1)._c(), 4, pair) == ARG           # gap_open of any sign
    for algo in LINEAR:   # the linear algorithms do not read gap_extend
        assert _status(L, algo, sa.ScoringSystem(-3, 1, 1, -1)._c(), 4, pair) == ARG


@pytest.mark.parametrize("algo", LINEAR + AFFINE)
def test_symbol_count(algo):
    L = sa.load_library()
    sc = (sa.ScoringSystem(-2, 1, -1) if algo in LINEAR else sa.ScoringSystem(-3, -1, 1, -1))._c()
    a64 = bytes(range(100, 164))
    assert _status(L, algo, sc, 4, [(a64[:40], a64[30:])]) == ARG                  # 64: passes, no context
    assert _status(L, algo, sc, 4, [(a64[:40], a64[30:] + b"\x00")]) == UNSUPPORTED   # 65, both sides together
    assert _status(L, algo, sc, 4, [(a64, b""), (b"", b"\xff")]) == UNSUPPORTED


@pytest.mark.parametrize("algo", LINEAR + AFFINE)
def test_score_bound_reads_the_table(algo):
    """(m + n + 1) * max |S| against 2^29, max |S| over the symbol pairs of the batch only."""
    L = sa.load_library()
    lin = algo in LINEAR
    sc = (sa.ScoringSystem(-2, 1, -1) if lin else sa.ScoringSystem(-3, -1, 1, -1))._c()
    big = TABLE.copy()
    big[ord("A"), ord("A")] = 32767
    # 2^29 = 16384 * 32768: m + n + 1 = 16385 is over, 16384 is not (16384 * 32767 + 10000 < 2^29 too)
    assert 16385 * 32767 >= 2 ** 29 > 16384 * 32767 + 10000
    assert _lengths(L, algo, sc, 4, 8192, 8192, big) == UNSUPPORTED
    assert _lengths(L, algo, sc, 4, 8192, 8191, big) == ARG
    # the affine bound adds 10000 (the border constant): with 1000 as the largest entry, m + n + 1 = 536861
    # is over for the affine algorithms and not for the linear ones, whose edge is 536871
    k = TABLE.copy()
    k[ord("A"), ord("A")] = 1000
    assert 536861 * 1000 < 2 ** 29 <= 536861 * 1000 + 10000 and 536860 * 1000 + 10000 < 2 ** 29 <= 536871 * 1000
    assert _lengths(L, algo, sc, 4, 268430, 268430, k) == (ARG if lin else UNSUPPORTED)
    assert _lengths(L, algo, sc, 4, 268430, 268429, k) == ARG
    assert _lengths(L, algo, sc, 4, 268435, 268435, k) == UNSUPPORTED
    assert _lengths(L, algo, sc, 4, 268435, 268434, k) == (ARG if lin else UNSUPPORTED)
    neg = TABLE.copy()
    neg[ord("A"), ord("A")] = -32768
    assert _lengths(L, algo, sc, 4, 8192, 8192, neg) == UNSUPPORTED
    unused = TABLE.copy()
    unused[ord("C"), ord("D")] = 32767          # a symbol pair the batch does not use
    assert _lengths(L, algo, sc, 4, 8192, 8192, unused) == ARG
    # the gap terms: linear |gap|, affine |gap_open| + |gap_extend| (stricter than the matrix call's max)
    if lin:
        g = sa.ScoringSystem(-1000, 1, -1)._c()
        assert _lengths(L, algo, g, 4, 268436, 268435) == UNSUPPORTED     # 536872 * 1000 >= 2^29
        assert _lengths(L, algo, g, 4, 268435, 268434) == ARG
    else:
        g = sa.ScoringSystem(-600, -400, 1, -1)._c()
        assert _lengths(L, algo, g, 4, 268430, 268430) == UNSUPPORTED     # 536861 * 1000 + 10000 >= 2^29
        assert _lengths(L, algo, g, 4, 268430, 268429) == ARG


@pytest.mark.parametrize("algo", LINEAR + AFFINE)
def test_pair_limits(algo):
    L = sa.load_library()
    lin = algo in LINEAR
    sc = (sa.ScoringSystem(-2, 1, -1) if lin else sa.ScoringSystem(-3, -1, 1, -1))._c()
    assert _lengths(L, algo, sc, 4, 2 ** 24, 100) == UNSUPPORTED        # a sequence of >= 2^24 symbols
    assert _lengths(L, algo, sc, 4, 100, 2 ** 24) == UNSUPPORTED
    if lin:
        assert _lengths(L, algo, sc, 4096, 2048, 2048) == UNSUPPORTED   # 4097 diagonals inside the matrix
        assert _lengths(L, algo, sc, 4096, 2048, 2047) == ARG           # 4096
        assert _lengths(L, algo, sc, 4, 100, 5000) == UNSUPPORTED       # 4909
    else:
        assert _lengths(L, algo, sc, 4096, 1024, 1024) == UNSUPPORTED   # 2049
        assert _lengths(L, algo, sc, 4096, 1024, 1023) == ARG           # 2048
        assert _lengths(L, algo, sc, 4, 100, 3000) == UNSUPPORTED       # 2909
    # local algorithms: (m + 1) * B' >= 2^31 with B' = 1021
    assert (2 ** 21 + 10001) * 1021 >= 2 ** 31
    local = algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH)
    assert _lengths(L, algo, sc, 10, 2 ** 21 + 10000, 2 ** 21 + 11000) == (UNSUPPORTED if local else ARG)


def test_bad_offsets():
    L = sa.load_library()
    sc = sa.ScoringSystem(-2, 1, -1)._c()
    res = np.zeros(2, dtype=sa.RESULT_DTYPE)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)
    for o1, o2 in [([1, 4], [0, 4]),          # offsets must start at 0
                   ([0, 4, 2], [0, 2, 4])]:   # and must not decrease
        a = np.array(o1, dtype=np.uint64)
        b = np.array(o2, dtype=np.uint64)
        rc = L.sa_score_batch_banded_matrix(None, sa.SA_NW, C.byref(sc), s.ctypes.data, a.ctypes.data, s.ctypes.data,
                                            b.ctypes.data, len(o1) - 1, TABLE.ctypes.data, None, 4, res.ctypes.data)
        assert rc == ARG and L.sa_last_error(None)
    rc = L.sa_score_batch_banded_matrix(None, sa.SA_NW, C.byref(sc), None, None, None, None, 0, TABLE.ctypes.data, None, 4, None)
    assert rc == ARG and L.sa_last_error(None)   # NULL offsets


def test_python_doors_without_a_device():
    """The new methods raise without a matrix before anything reaches the engine."""
    for cls, args in [(sa.SmithWatermanSA, (-1, 1, -1)), (sa.NeedlemanWunschSA, (-1, 1, -1)),
                      (sa.LocalGotohSA, (-3, -1, 1, -1)), (sa.GlobalGotohSA, (-3, -1, 1, -1))]:
        al = cls(sa.ScoringSystem(*args))
        with pytest.raises(sa.SeqalibError):
            al.getBandedMatrixAlignments([("AC", "AC")], 2)
        with pytest.raises(sa.SeqalibError):
            al.getBandedMatrixScores([("AC", "AC")], 2)
