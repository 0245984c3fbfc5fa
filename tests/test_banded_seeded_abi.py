"""CPU: the seeded banded entry points (sa_align_batch_banded_seeded, sa_score_batch_banded_seeded,
sa_banded_seeded_plan_query, include/seqalib_hip.h) are exported and every status rule answers without a
context: the algorithm classes, free_ends, diag, the legality rule (a legal begin and a legal end in the
band), the diagonal caps, and the geometry the plan query reports.  No GPU compute is called here."""
import ctypes as C

import numpy as np
import pytest

import seqalib_amd as sa
from seeded_model import seeded_band, seeded_legal, seeded_steps

SYMBOLS = ["sa_align_batch_banded_seeded", "sa_score_batch_banded_seeded", "sa_banded_seeded_plan_query"]
ALGS = [sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH]
FIT = 12   # SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END
OK, ARG, UNSUPPORTED = 0, -1, -5
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals


def test_symbols_exported():
    L = sa.load_library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert L.sa_version() == 1   # the change only adds symbols


def _calls(L):
    def align(ctx, algo, sc, diag, band, fe, o1=None, o2=None, npairs=0):
        return L.sa_align_batch_banded_seeded(ctx, algo, sc, None, o1, None, o2, npairs, None, diag, band, fe, None, None, 0)

    def score(ctx, algo, sc, diag, band, fe, o1=None, o2=None, npairs=0):
        return L.sa_score_batch_banded_seeded(ctx, algo, sc, None, o1, None, o2, npairs, None, diag, band, fe, None)

    return align, score


def _plan(L, algo, m, n, k, w, fe):
    R, ppw, ws = C.c_int(-1), C.c_int(-1), C.c_uint64(0)
    rc = L.sa_banded_seeded_plan_query(algo, m, n, k, w, fe, C.byref(R), C.byref(ppw), C.byref(ws))
    return rc, R.value, ppw.value, ws.value


def test_argument_checks_need_no_context():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for call in _calls(L):
        for algo in ALGS:
            sc = aff if algo == sa.SA_GLOBAL_GOTOH else lin
            nomis = (sa.ScoringSystem(-3, -1, 2, -1, False) if algo == sa.SA_GLOBAL_GOTOH else sa.ScoringSystem(-1, 2))._c()
            for fe in range(16):
                assert call(None, algo, C.byref(sc), None, 4, fe) == ARG          # only the context is missing
            assert call(None, algo, C.byref(sc), None, 4, 16) == ARG              # free_ends outside SA_FREE_*
            assert call(None, algo, C.byref(sc), None, 4, 2 ** 32 - 1) == ARG
            assert call(None, algo, None, None, 4, FIT) == ARG                    # NULL scoring
            assert call(None, algo, C.byref(nomis), None, 0, FIT) == UNSUPPORTED  # one diagonal, no mismatches
            assert call(None, algo, C.byref(nomis), None, 1, FIT) == ARG
            assert call(None, algo, C.byref(sc), None, 2 ** 31, FIT) == ARG       # band >= 2^31
            assert call(None, algo, C.byref(sc), None, 2 ** 32 - 1, FIT) == ARG
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(sa.ScoringSystem(-3, 1, 1, -1)._c()), None, 4, FIT) == UNSUPPORTED   # gap_extend > 0
        for algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH, sa.SA_MYERS_MILLER):
            assert call(None, algo, C.byref(aff), None, 4, FIT) == UNSUPPORTED
        for algo in (-1, 6, 9):
            assert call(None, algo, C.byref(aff), None, 4, FIT) == ARG
        assert call(None, sa.SA_SW, C.byref(lin), None, 4, 16) == ARG   # a bad free_ends whatever the algorithm's class
    for algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH, sa.SA_MYERS_MILLER):
        assert _plan(L, algo, 10, 10, 0, 4, FIT)[0] == UNSUPPORTED
    assert _plan(L, 7, 10, 10, 0, 4, FIT)[0] == ARG
    assert _plan(L, sa.SA_NW, 10, 10, 0, 4, 16)[0] == ARG
    assert _plan(L, sa.SA_NW, 10, 10, 0, 2 ** 31, FIT)[0] == ARG
    assert _plan(L, sa.SA_NW, 2 ** 24, 10, 0, 4, FIT)[0] == UNSUPPORTED
    assert _plan(L, sa.SA_NW, 10, 2 ** 24, 0, 4, FIT)[0] == UNSUPPORTED


def _status(L, algo, sc, m, n, k, band, fe=FIT):
    o1, o2 = np.array([0, m], dtype=np.uint64), np.array([0, n], dtype=np.uint64)
    d = np.array([k], dtype=np.int32)
    out = {call(None, algo, C.byref(sc), d.ctypes.data, band, fe, o1.ctypes.data, o2.ctypes.data, 1) for call in _calls(L)}
    assert len(out) == 1
    return out.pop()


def test_diag_checks_name_the_pair():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    o1, o2 = np.array([0, 5, 10], dtype=np.uint64), np.array([0, 5, 25], dtype=np.uint64)   # 5 x 5 (legal at k = 0 whatever the flags), 5 x 20
    for call in _calls(L):
        assert call(None, sa.SA_NW, C.byref(lin), None, 4, FIT, o1.ctypes.data, o2.ctypes.data, 2) == ARG   # NULL diag
        assert b"diag" in L.sa_last_error(None)
        for bad in (-6, 21):   # the seed diagonal does not cross pair 1's 5 x 20 matrix
            d = np.array([0, bad], dtype=np.int32)
            assert call(None, sa.SA_NW, C.byref(lin), d.ctypes.data, 4, FIT, o1.ctypes.data, o2.ctypes.data, 2) == ARG
            assert b"pair 1" in L.sa_last_error(None)
        for good in (-5, 20):   # the corner diagonals: legal with every end free
            d = np.array([0, good], dtype=np.int32)
            assert call(None, sa.SA_NW, C.byref(lin), d.ctypes.data, 4, 15, o1.ctypes.data, o2.ctypes.data, 2) == ARG
            assert b"ctx" in L.sa_last_error(None)
        # pair 1 seeded at 10 with w = 2 and no free end: neither (0, 0) nor (m, n) is in its band
        d = np.array([0, 10], dtype=np.int32)
        assert call(None, sa.SA_NW, C.byref(lin), d.ctypes.data, 2, 0, o1.ctypes.data, o2.ctypes.data, 2) == UNSUPPORTED
        msg = L.sa_last_error(None)
        assert b"pair 1" in msg and b"begin" in msg and b"end" in msg
        assert call(None, sa.SA_NW, C.byref(lin), d.ctypes.data, 2, sa.SA_FREE_SEQ2_BEGIN, o1.ctypes.data, o2.ctypes.data, 2) == UNSUPPORTED
        msg = L.sa_last_error(None)
        assert b"pair 1" in msg and b"end" in msg and b"begin" not in msg
        assert call(None, sa.SA_NW, C.byref(lin), d.ctypes.data, 2, sa.SA_FREE_SEQ2_END, o1.ctypes.data, o2.ctypes.data, 2) == UNSUPPORTED
        msg = L.sa_last_error(None)
        assert b"pair 1" in msg and b"begin" in msg and b"legal end" not in msg


def _expected_plan(affine, m, n, k, w):
    """(R, pairs per wave, record bytes) from the header's formulas, or None past the diagonal cap."""
    lo, hi = seeded_band(m, n, k, w)
    beff = hi - lo + 1
    tb, tend = seeded_steps(m, n, k, w)
    steps = tend - tb + 1
    for R, Ln in VARIANTS[:7] if affine else VARIANTS:
        if beff <= 2 * R * Ln:
            if affine:
                words = -(-steps // (8 // R)) * Ln if R <= 8 else steps * (R // 8) * Ln
            else:
                words = -(-steps // (16 // R)) * Ln if R <= 16 else steps * 2 * Ln
            return R, 64 // Ln, 4 * words
    return None


@pytest.mark.parametrize("algo", [sa.SA_NW, sa.SA_GLOBAL_GOTOH])
def test_legality_and_geometry_exhaustively(algo):
    """m, n <= 6, k in [-m - 1, n + 1], w <= 3, every free_ends: the score call's status is the legality
    rule restated in Python (tests/seeded_model.py), the plan query agrees, and B', the variant and the
    record bytes come from the formulas for tb / tend."""
    L = sa.load_library()
    affine = algo == sa.SA_GLOBAL_GOTOH
    sc = (sa.ScoringSystem(-3, -1, 1, -1) if affine else sa.ScoringSystem(-1, 1, -1))._c()
    score = _calls(L)[1]
    checked = 0
    for m in range(7):
        for n in range(7):
            o1, o2 = np.array([0, m], dtype=np.uint64), np.array([0, n], dtype=np.uint64)
            for k in range(-m - 1, n + 2):
                d = np.array([k], dtype=np.int32)
                for w in range(4):
                    for fe in range(16):
                        rc = score(None, algo, C.byref(sc), d.ctypes.data, w, fe, o1.ctypes.data, o2.ctypes.data, 1)
                        plan = _plan(L, algo, m, n, k, w, fe)
                        if not -m <= k <= n:
                            assert rc == ARG and plan[0] == ARG, (m, n, k, w, fe)
                            continue
                        if seeded_legal(m, n, k, w, fe) != (True, True):
                            assert rc == UNSUPPORTED and plan[0] == UNSUPPORTED, (m, n, k, w, fe)
                            continue
                        assert rc == ARG, (m, n, k, w, fe)   # only the context is missing
                        assert plan == (OK,) + _expected_plan(affine, m, n, k, w), (m, n, k, w, fe)
                        checked += 1
    assert checked > 5000


def test_diagonal_caps():
    """4096 (NW) / 2048 (GlobalGotoh) diagonals inside the matrix, a shape just inside and just past each;
    the cap is on the clipped band, so a seed near a corner admits a wider w."""
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for algo in (sa.SA_NW, sa.SA_HIRSCHBERG):
        assert _status(L, algo, lin, 100, 9000, 4000, 2047) == ARG           # 4095 diagonals
        assert _status(L, algo, lin, 100, 9000, 4000, 2048) == UNSUPPORTED   # 4097
    assert _plan(L, sa.SA_NW, 100, 9000, 0, 3995, FIT)[0] == OK              # lo' = -100, hi' = 3995: 4096
    assert _plan(L, sa.SA_NW, 100, 9000, 0, 3996, FIT)[0] == UNSUPPORTED     # 4097
    assert _plan(L, sa.SA_NW, 100, 9000, 4000, 2047, FIT)[1] == 32
    assert _status(L, sa.SA_GLOBAL_GOTOH, aff, 100, 9000, 4000, 1023) == ARG          # 2047
    assert _status(L, sa.SA_GLOBAL_GOTOH, aff, 100, 9000, 4000, 1024) == UNSUPPORTED  # 2049
    assert _plan(L, sa.SA_GLOBAL_GOTOH, 100, 9000, 0, 1947, FIT)[0] == OK             # lo' = -100, hi' = 1947: 2048
    assert _plan(L, sa.SA_GLOBAL_GOTOH, 100, 9000, 0, 1948, FIT)[0] == UNSUPPORTED
    assert _plan(L, sa.SA_GLOBAL_GOTOH, 100, 9000, 4000, 1023, FIT)[1] == 16


def test_a_read_against_a_contig():
    """m = 150, n = 10^6, k = 5 * 10^5, w = 16: accepted, 33 diagonals, four pairs per wave, and record
    bytes that do not depend on n (2m + 2w + 1 steps)."""
    L = sa.load_library()
    seen = set()
    for n in (10 ** 6, 10 ** 6 + 12345, 2 ** 24 - 1, 520000):
        for algo in (sa.SA_NW, sa.SA_GLOBAL_GOTOH):
            rc, R, ppw, ws = _plan(L, algo, 150, n, 500000, 16, FIT)
            assert (rc, R, ppw) == (OK, 2, 4), (n, algo)
            assert ws == _expected_plan(algo == sa.SA_GLOBAL_GOTOH, 150, n, 500000, 16)[2]
            seen.add((algo, ws))
        assert _status(L, sa.SA_NW, sa.ScoringSystem(-1, 1, -1)._c(), 150, n, 500000, 16) == ARG
    assert len(seen) == 2
    assert seeded_steps(150, 10 ** 6, 500000, 16) == (0, 2 * 150 + 2 * 16)
    # the corridor band refuses the same pair
    o1, o2 = np.array([0, 150], dtype=np.uint64), np.array([0, 10 ** 6], dtype=np.uint64)
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    assert L.sa_score_batch_banded_ends_free(None, sa.SA_NW, C.byref(lin), None, o1.ctypes.data, None, o2.ctypes.data, 1,
                                             None, 16, FIT, None) == UNSUPPORTED


def test_python_doors_raise_where_there_is_no_seeded_form():
    pairs = [(b"ACGT", b"ACGT")]
    for cls in (sa.SmithWatermanSA, sa.LocalGotohSA, sa.MyersMillerSA):
        for door in ("getSeededAlignments", "getSeededScores", "getSeededEndCells"):
            with pytest.raises(sa.SeqalibError):
                getattr(cls(), door)(pairs, [0], 4, FIT)
    m = sa.SubstitutionMatrix(b"ACGT", np.eye(4, dtype=np.int16))
    for cls in (sa.NeedlemanWunschSA, sa.GlobalGotohSA):
        with pytest.raises(sa.SeqalibError):
            cls(matrix=m).getSeededAlignments(pairs, [0], 4, FIT)
        with pytest.raises(sa.SeqalibError):
            cls(matrix=m).getSeededScores(pairs, [0], 4, FIT)
    for cls in (sa.NeedlemanWunschSA, sa.HirschbergSA, sa.GlobalGotohSA):
        for diags in ([], [0, 0]):   # the wrong length raises before the C call (no context is made)
            with pytest.raises(sa.SeqalibError, match="seed diagonals"):
                cls().getSeededAlignments(pairs, diags, 4, FIT)
            with pytest.raises(sa.SeqalibError, match="seed diagonals"):
                cls().getSeededScores(pairs, diags, 4, FIT)
    with pytest.raises(sa.SeqalibError):
        sa.banded_seeded_plan_query(sa.SA_NW, 5, 20, 10, 2, 0)
    assert sa.banded_seeded_plan_query(sa.SA_NW, 150, 10 ** 6, 500000, 16, FIT)[:2] == (2, 4)
