"""CPU: the banded extension entry points (sa_align_batch_banded_extend, sa_score_batch_banded_extend,
sa_banded_extend_plan_query, include/seqalib_hip.h) are exported and every status rule answers without a
context: the algorithm classes, xdrop, the band, the scoring rules, the per-pair limits with SW's key
limit, the diagonal caps, calls that break two rules at once, and the geometry the plan query reports.
SA_ERR_CAPACITY and SA_ERR_NOMEM need a context: tests/test_gpu_banded_extend.py reaches them
(test_capacity_and_workspace_statuses).  No GPU compute is called here."""
import ctypes as C

import numpy as np
import pytest

import seqalib_amd as sa
from extend_model import extend_band

SYMBOLS = ["sa_align_batch_banded_extend", "sa_score_batch_banded_extend", "sa_banded_extend_plan_query"]
ALGS = [sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH]
OTHERS = [sa.SA_SW, sa.SA_LOCAL_GOTOH, sa.SA_MYERS_MILLER]
OK, ARG, UNSUPPORTED = 0, -1, -5
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals


def test_symbols_and_constants():
    L = sa.load_library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert L.sa_version() == 1   # the change only adds symbols
    assert (sa.SA_XDROP_OFF, sa.SA_XDROP_PERIOD, sa.SA_FLAG_DROPPED) == (-1, 16, 32)
    header = open(sa.library_path().rsplit("/seqalib_amd/", 1)[0] + "/include/seqalib_hip.h").read()
    assert "#define SA_XDROP_OFF (-1)" in header and "#define SA_XDROP_PERIOD 16" in header and "SA_FLAG_DROPPED = 32" in header


def _calls(L):
    def align(ctx, algo, sc, band, xdrop, o1=None, o2=None, npairs=0):
        return L.sa_align_batch_banded_extend(ctx, algo, sc, None, o1, None, o2, npairs, None, band, xdrop, None, None, 0)

    def score(ctx, algo, sc, band, xdrop, o1=None, o2=None, npairs=0):
        return L.sa_score_batch_banded_extend(ctx, algo, sc, None, o1, None, o2, npairs, None, band, xdrop, None)

    return align, score


def _plan(L, algo, m, n, w):
    R, ppw, ws = C.c_int(-1), C.c_int(-1), C.c_uint64(0)
    rc = L.sa_banded_extend_plan_query(algo, m, n, w, C.byref(R), C.byref(ppw), C.byref(ws))
    return rc, R.value, ppw.value, ws.value


def test_argument_checks_need_no_context():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    up = sa.ScoringSystem(-3, 1, 1, -1)._c()   # gap_extend > 0
    for call in _calls(L):
        for algo in ALGS:
            sc = aff if algo == sa.SA_GLOBAL_GOTOH else lin
            nomis = (sa.ScoringSystem(-3, -1, 2, -1, False) if algo == sa.SA_GLOBAL_GOTOH else sa.ScoringSystem(-1, 2))._c()
            for xdrop in (sa.SA_XDROP_OFF, 0, 1, 30, 2 ** 31 - 1):
                assert call(None, algo, C.byref(sc), 4, xdrop) == ARG             # only the context is missing
                assert b"ctx" in L.sa_last_error(None)
            for xdrop in (-2, -17, -(2 ** 31)):
                assert call(None, algo, C.byref(sc), 4, xdrop) == ARG             # xdrop < -1
                assert b"xdrop" in L.sa_last_error(None)
            assert call(None, algo, None, 4, 10) == ARG                           # NULL scoring
            assert call(None, algo, C.byref(nomis), 0, 10) == UNSUPPORTED         # one diagonal, no mismatches
            assert call(None, algo, C.byref(nomis), 1, 10) == ARG
            assert b"ctx" in L.sa_last_error(None)
            assert call(None, algo, C.byref(sc), 2 ** 31, 10) == ARG              # band >= 2^31
            assert b"band" in L.sa_last_error(None)
            assert call(None, algo, C.byref(sc), 2 ** 32 - 1, 10) == ARG
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(up), 4, 10) == UNSUPPORTED
        for algo in OTHERS:
            assert call(None, algo, C.byref(aff), 4, 10) == UNSUPPORTED
        for algo in (-1, 6, 9):
            assert call(None, algo, C.byref(aff), 4, 10) == ARG
    for algo in OTHERS:
        assert _plan(L, algo, 10, 10, 4)[0] == UNSUPPORTED
    assert _plan(L, 7, 10, 10, 4)[0] == ARG
    assert _plan(L, sa.SA_NW, 10, 10, 2 ** 31)[0] == ARG
    assert _plan(L, sa.SA_NW, 2 ** 24, 10, 4)[0] == UNSUPPORTED
    assert _plan(L, sa.SA_NW, 10, 2 ** 24, 4)[0] == UNSUPPORTED
    assert _plan(L, sa.SA_NW, 2 ** 40, 10, 4)[0] == UNSUPPORTED


def test_two_broken_rules_at_once():
    """An SA_ERR_ARG rule wins over an SA_ERR_UNSUPPORTED one, whatever their order in the argument list."""
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    up = sa.ScoringSystem(-3, 1, 1, -1)._c()
    nomis = sa.ScoringSystem(-3, 1, 2, -1, False)._c()   # gap_extend > 0 and no mismatches
    big = np.array([0, 2 ** 24], dtype=np.uint64)
    small = np.array([0, 10], dtype=np.uint64)
    for call in _calls(L):
        for algo in OTHERS:
            assert call(None, algo, C.byref(lin), 4, -2) == ARG                   # an unsupported class and a bad xdrop
            assert call(None, algo, C.byref(lin), 2 ** 31, 10) == ARG             # ... and a band that overflows
        assert call(None, 9, C.byref(lin), 4, -2) == ARG
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(up), 2 ** 31, 10) == ARG    # gap_extend > 0 and the band
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(up), 4, -5) == ARG          # gap_extend > 0 and xdrop
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(nomis), 0, 10) == UNSUPPORTED   # two unsupported rules
        assert call(None, sa.SA_SW, C.byref(nomis), 0, 10) == UNSUPPORTED
        # a pair past 2^24 symbols whose band is past the cap as well; with a bad xdrop on top
        assert call(None, sa.SA_NW, C.byref(lin), 5000, 10, big.ctypes.data, big.ctypes.data, 1) == UNSUPPORTED
        assert call(None, sa.SA_NW, C.byref(lin), 5000, -2, big.ctypes.data, big.ctypes.data, 1) == ARG
        # decreasing offsets are an argument error before that pair's limits
        down = np.array([0, 10, 5], dtype=np.uint64)
        both = np.array([0, 5, 5 + 2 ** 24], dtype=np.uint64)
        assert call(None, sa.SA_NW, C.byref(lin), 4, 10, down.ctypes.data, both.ctypes.data, 2) == ARG
        assert call(None, sa.SA_NW, C.byref(lin), 4, 10, small.ctypes.data, small.ctypes.data, 1) == ARG   # (valid: the context)
        assert b"ctx" in L.sa_last_error(None)


def _status(L, algo, sc, m, n, band, xdrop=10):
    o1, o2 = np.array([0, m], dtype=np.uint64), np.array([0, n], dtype=np.uint64)
    out = {call(None, algo, C.byref(sc), band, xdrop, o1.ctypes.data, o2.ctypes.data, 1) for call in _calls(L)}
    assert len(out) == 1
    return out.pop()


def test_pair_limits():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for algo in ALGS:
        sc = aff if algo == sa.SA_GLOBAL_GOTOH else lin
        assert _status(L, algo, sc, 2 ** 24 - 1, 100, 4) == ARG            # only the context is missing
        assert _status(L, algo, sc, 2 ** 24, 100, 4) == UNSUPPORTED
        assert _status(L, algo, sc, 100, 2 ** 24, 4) == UNSUPPORTED
        # SW's key limit: (m + 1) * B' < 2^31
        assert _status(L, algo, sc, 2 ** 21, 2 ** 21, 600) == UNSUPPORTED  # 2^21 * 1201
        assert b"2^31" in L.sa_last_error(None)
        assert _plan(L, algo, 2 ** 21, 2 ** 21, 600)[0] == UNSUPPORTED
        assert _status(L, algo, sc, 2 ** 20, 2 ** 21, 600) == ARG          # 2^20 * 1201 < 2^31
        assert _status(L, algo, sc, 2 ** 21, 100, 600) == ARG              # B' = 701: the clipped band counts
    # the 2^29 score bounds
    assert _status(L, sa.SA_NW, sa.ScoringSystem(-1, 2 ** 20, -1)._c(), 300, 300, 4) == UNSUPPORTED     # 601 * 2^20
    assert _status(L, sa.SA_NW, sa.ScoringSystem(-1, 2 ** 20, -1)._c(), 200, 200, 4) == ARG             # 401 * 2^20
    assert _status(L, sa.SA_NW, sa.ScoringSystem(-(2 ** 20), 1, -1)._c(), 300, 300, 4) == UNSUPPORTED
    assert _status(L, sa.SA_NW, sa.ScoringSystem(-1, 1, -(2 ** 20), False)._c(), 300, 300, 4) == ARG     # a mismatch term that is not read
    assert _status(L, sa.SA_GLOBAL_GOTOH, sa.ScoringSystem(-(2 ** 19), -(2 ** 19), 1, -1)._c(), 300, 300, 4) == UNSUPPORTED
    assert _status(L, sa.SA_GLOBAL_GOTOH, sa.ScoringSystem(-3, -1, 2 ** 20, -1)._c(), 256, 256, 4) == UNSUPPORTED   # 513 * 2^20 + 10000
    assert _status(L, sa.SA_GLOBAL_GOTOH, sa.ScoringSystem(-3, -1, 2 ** 20, -1)._c(), 250, 250, 4) == ARG


def test_diagonal_caps():
    """4096 (NW) / 2048 (GlobalGotoh) diagonals inside the matrix, a shape just inside and just past each."""
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for algo in (sa.SA_NW, sa.SA_HIRSCHBERG):
        assert _status(L, algo, lin, 9000, 9000, 2047) == ARG           # 4095 diagonals
        assert _status(L, algo, lin, 9000, 9000, 2048) == UNSUPPORTED   # 4097
        assert _plan(L, algo, 100, 9000, 3995)[:3] == (OK, 32, 1)       # lo' = -100, hi' = 3995: 4096
        assert _plan(L, algo, 100, 9000, 3996)[0] == UNSUPPORTED
        assert _plan(L, algo, 9000, 100, 3996)[0] == UNSUPPORTED        # lo' = -3996, hi' = 100
        assert _plan(L, algo, 100, 100, 2 ** 31 - 1)[:3] == (OK, 4, 2)  # the whole 100 x 100 matrix: 201 diagonals
    assert _status(L, sa.SA_GLOBAL_GOTOH, aff, 9000, 9000, 1023) == ARG
    assert _status(L, sa.SA_GLOBAL_GOTOH, aff, 9000, 9000, 1024) == UNSUPPORTED
    assert _plan(L, sa.SA_GLOBAL_GOTOH, 100, 9000, 1947)[:3] == (OK, 16, 1)
    assert _plan(L, sa.SA_GLOBAL_GOTOH, 100, 9000, 1948)[0] == UNSUPPORTED


def _expected_plan(affine, m, n, w):
    """(R, pairs per wave, record bytes) from the header's formulas."""
    lo, hi, tend = extend_band(m, n, w)
    beff = hi - lo + 1
    steps = tend - ((-lo) & ~1) + 1
    for R, Ln in VARIANTS[:7] if affine else VARIANTS:
        if beff <= 2 * R * Ln:
            if affine:
                words = -(-steps // (8 // R)) * Ln if R <= 8 else steps * (R // 8) * Ln
            else:
                words = -(-steps // (16 // R)) * Ln if R <= 16 else steps * 2 * Ln
            return R, 64 // Ln, 4 * words


@pytest.mark.parametrize("algo", [sa.SA_NW, sa.SA_GLOBAL_GOTOH])
def test_geometry(algo):
    """Every shape is accepted (there is no legality rule), and B', the variant and the record bytes come from
    the header's formulas; the seeded plan query at diag = 0 with both ends free reports the same records."""
    L = sa.load_library()
    affine = algo == sa.SA_GLOBAL_GOTOH
    sc = (sa.ScoringSystem(-3, -1, 1, -1) if affine else sa.ScoringSystem(-1, 1, -1))._c()
    shapes = [(m, n, w) for m in range(7) for n in range(7) for w in range(4)]
    shapes += [(150, 2000, 16), (2000, 150, 16), (2000, 2000, 16), (40, 40, 8), (5000, 5000, 1023), (0, 0, 0), (0, 77, 5), (77, 0, 5),
               (300, 20, 100), (20, 300, 100)]
    for m, n, w in shapes:
        assert _status(L, algo, sc, m, n, w) == ARG, (m, n, w)   # only the context is missing
        assert _plan(L, algo, m, n, w) == (OK,) + _expected_plan(affine, m, n, w), (m, n, w)
        R, ppw, ws = C.c_int(), C.c_int(), C.c_uint64()
        assert L.sa_banded_seeded_plan_query(algo, m, n, 0, w, 10, C.byref(R), C.byref(ppw), C.byref(ws)) == OK
        assert (R.value, ppw.value, ws.value) == _plan(L, algo, m, n, w)[1:]
    assert _plan(L, algo, 2000, 2000, 16)[1:3] == (2, 4)


def test_python_doors_raise_where_there_is_no_extension_form():
    pairs = [(b"ACGT", b"ACGT")]
    doors = ("getExtensionAlignments", "getExtensionScores", "getExtensionEndCells", "getExtensionDropped")
    for cls in (sa.SmithWatermanSA, sa.LocalGotohSA, sa.MyersMillerSA):
        for door in doors:
            with pytest.raises(sa.SeqalibError):
                getattr(cls(), door)(pairs, 4, 10)
        with pytest.raises(sa.SeqalibError):
            cls().getExtensionAlignment(b"ACGT", b"ACGT", 4, 10)
    m = sa.SubstitutionMatrix(b"ACGT", np.eye(4, dtype=np.int16))
    for cls in (sa.NeedlemanWunschSA, sa.HirschbergSA, sa.GlobalGotohSA):
        for door in doors:
            with pytest.raises(sa.SeqalibError, match="matrix"):
                getattr(cls(matrix=m), door)(pairs, 4, 10)
    with pytest.raises(sa.SeqalibError):
        sa.banded_extend_plan_query(sa.SA_SW, 10, 10, 4)
    with pytest.raises(sa.SeqalibError):
        sa.banded_extend_plan_query(sa.SA_NW, 9000, 9000, 2048)
    assert sa.banded_extend_plan_query(sa.SA_NW, 2000, 2000, 16)[:2] == (2, 4)
    assert sa.banded_extend_plan_query(sa.SA_GLOBAL_GOTOH, 150, 10 ** 6, 16)[:2] == (2, 4)
