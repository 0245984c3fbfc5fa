"""CPU: the device-resident seeded banded entry points (sa_align_batch_banded_seeded_device,
sa_score_batch_banded_seeded_device, sa_banded_seeded_device_plan_query, include/seqalib_hip.h) are exported,
every host-side status rule answers without a context -- the algorithm classes, free_ends, band, NULL pointers,
and the three refusals made from the bound shape alone, with both sides of the 4096 / 2048 caps -- and the plan
query returns the bound restated here.  No pointer is dereferenced before the context is looked at, so the
"device" pointers are plain non-NULL numbers.  No GPU is touched."""
import ctypes as C

import pytest

import seqalib_amd as sa

SYMBOLS = ["sa_align_batch_banded_seeded_device", "sa_score_batch_banded_seeded_device", "sa_banded_seeded_device_plan_query"]
ALGS = [sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH]
FIT = 12   # SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END
OK, ARG, UNSUPPORTED = 0, -1, -5
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals
P = 4096   # a non-NULL pointer that is never read


def test_symbols_exported():
    L = sa.load_library()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert L.sa_version() == 1   # the change only adds symbols
    assert sa.SA_FLAG_BAD_BAND == 64


def _calls(L):
    """Both calls with one signature; `null` names the pointer arguments to pass as NULL."""
    def ptrs(null):
        names = ("seq1", "start1", "len1", "seq2", "start2", "len2", "diag", "res", "ops", "ops_off")
        return {k: (None if k in null else P) for k in names}

    def align(ctx, algo, sc, band, fe, npairs=1, max_m=40, max_n=40, null=()):
        p = ptrs(null)
        return L.sa_align_batch_banded_seeded_device(ctx, algo, sc, p["seq1"], 100, p["start1"], p["len1"], p["seq2"], 100,
                                                     p["start2"], p["len2"], npairs, max_m, max_n, None, p["diag"], band, fe,
                                                     p["res"], p["ops"], p["ops_off"], 1000, None)

    def score(ctx, algo, sc, band, fe, npairs=1, max_m=40, max_n=40, null=()):
        p = ptrs(null)
        return L.sa_score_batch_banded_seeded_device(ctx, algo, sc, p["seq1"], 100, p["start1"], p["len1"], p["seq2"], 100,
                                                     p["start2"], p["len2"], npairs, max_m, max_n, None, p["diag"], band, fe,
                                                     p["res"], None)

    return align, score


def _plan(L, algo, max_m, max_n, band):
    R, rec, plan = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
    rc = L.sa_banded_seeded_device_plan_query(algo, max_m, max_n, band, C.byref(R), C.byref(rec), C.byref(plan))
    return rc, R.value, rec.value, plan.value


def test_argument_checks_need_no_context():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for call in _calls(L):
        for algo in ALGS:
            sc = aff if algo == sa.SA_GLOBAL_GOTOH else lin
            nomis = (sa.ScoringSystem(-3, -1, 2, -1, False) if algo == sa.SA_GLOBAL_GOTOH else sa.ScoringSystem(-1, 2))._c()
            for fe in range(16):
                assert call(None, algo, C.byref(sc), 4, fe) == ARG          # only the context is missing
                assert b"ctx" in L.sa_last_error(None)
            assert call(None, algo, C.byref(sc), 4, FIT, npairs=0) == ARG   # ... also with no pair
            assert call(None, algo, C.byref(sc), 4, 16) == ARG              # free_ends outside SA_FREE_*
            assert b"free_ends" in L.sa_last_error(None)
            assert call(None, algo, C.byref(sc), 4, 2 ** 32 - 1) == ARG
            assert call(None, algo, None, 4, FIT) == ARG                    # NULL scoring
            assert b"scoring" in L.sa_last_error(None)
            assert call(None, algo, C.byref(nomis), 0, FIT) == UNSUPPORTED  # one diagonal, no mismatches
            assert call(None, algo, C.byref(nomis), 1, FIT) == ARG
            assert call(None, algo, C.byref(sc), 2 ** 31, FIT) == ARG       # band >= 2^31
            assert b"band" in L.sa_last_error(None)
            assert call(None, algo, C.byref(sc), 2 ** 32 - 1, FIT) == ARG
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(sa.ScoringSystem(-3, 1, 1, -1)._c()), 4, FIT) == UNSUPPORTED   # gap_extend > 0
        for algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH, sa.SA_MYERS_MILLER):
            assert call(None, algo, C.byref(aff), 4, FIT) == UNSUPPORTED
        for algo in (-1, 6, 9):
            assert call(None, algo, C.byref(aff), 4, FIT) == ARG
        assert call(None, sa.SA_SW, C.byref(lin), 4, 16) == ARG   # a bad free_ends whatever the algorithm's class
    for algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH, sa.SA_MYERS_MILLER):
        assert _plan(L, algo, 10, 10, 4)[0] == UNSUPPORTED
    assert _plan(L, 7, 10, 10, 4)[0] == ARG
    assert _plan(L, sa.SA_NW, 10, 10, 2 ** 31)[0] == ARG


def test_null_pointers():
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    align, score = _calls(L)
    for name in ("start1", "len1", "start2", "len2", "diag", "res", "seq1", "seq2"):
        for call in (align, score):
            assert call(None, sa.SA_NW, C.byref(lin), 4, FIT, null=(name,)) == ARG, name
            assert b"NULL" in L.sa_last_error(None), name
    for name in ("ops", "ops_off"):
        assert align(None, sa.SA_NW, C.byref(lin), 4, FIT, null=(name,)) == ARG, name
        assert b"NULL" in L.sa_last_error(None), name
    # no pair: no pointer is needed, only the context is missing
    everything = ("seq1", "start1", "len1", "seq2", "start2", "len2", "diag", "res", "ops", "ops_off")
    for call in (align, score):
        assert call(None, sa.SA_NW, C.byref(lin), 4, FIT, npairs=0, null=everything) == ARG
        assert b"ctx" in L.sa_last_error(None)


def test_bound_shape_refusals():
    """From (max_m, max_n, band, scoring) alone: a length bound >= 2^24, the 2^29 score bound, and the band of
    min(2w + 1, max_m + max_n + 1) diagonals against 4096 (NW) / 2048 (GlobalGotoh), both sides of each."""
    L = sa.load_library()
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    for call in _calls(L):
        for algo in ALGS:
            sc = aff if algo == sa.SA_GLOBAL_GOTOH else lin
            assert call(None, algo, C.byref(sc), 4, FIT, max_m=2 ** 24 - 1, max_n=2 ** 24 - 1) == ARG
            assert call(None, algo, C.byref(sc), 4, FIT, max_m=2 ** 24) == UNSUPPORTED
            assert b"2^24" in L.sa_last_error(None)
            assert call(None, algo, C.byref(sc), 4, FIT, max_n=2 ** 24) == UNSUPPORTED
            assert call(None, algo, C.byref(sc), 4, FIT, max_m=2 ** 32 - 1) == UNSUPPORTED
        # the score bound: (max_m + max_n + 1) * big (+ 10000) < 2^29
        big = sa.ScoringSystem(-1, 1024, -1)._c()          # big = 1024: max_m + max_n + 1 < 2^19
        assert call(None, sa.SA_NW, C.byref(big), 4, FIT, max_m=2 ** 18, max_n=2 ** 18 - 2) == ARG
        assert call(None, sa.SA_NW, C.byref(big), 4, FIT, max_m=2 ** 18, max_n=2 ** 18 - 1) == UNSUPPORTED
        assert b"2^29" in L.sa_last_error(None)
        abig = sa.ScoringSystem(-1000, -24, 1, -1)._c()    # big = 1024, and the borders' 10000: max_m + max_n + 1 <= 2^19 - 10
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(abig), 4, FIT, max_m=2 ** 18, max_n=2 ** 18 - 11) == ARG
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(abig), 4, FIT, max_m=2 ** 18, max_n=2 ** 18 - 10) == UNSUPPORTED
        # the diagonal caps
        for algo in (sa.SA_NW, sa.SA_HIRSCHBERG):
            assert call(None, algo, C.byref(lin), 2047, FIT, max_m=5000, max_n=5000) == ARG            # 4095
            assert call(None, algo, C.byref(lin), 2048, FIT, max_m=5000, max_n=5000) == UNSUPPORTED    # 4097
            assert b"4096" in L.sa_last_error(None)
            assert call(None, algo, C.byref(lin), 2 ** 31 - 1, FIT, max_m=2000, max_n=2095) == ARG     # the matrix clips: 4096
            assert call(None, algo, C.byref(lin), 2 ** 31 - 1, FIT, max_m=2000, max_n=2096) == UNSUPPORTED
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(aff), 1023, FIT, max_m=5000, max_n=5000) == ARG           # 2047
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(aff), 1024, FIT, max_m=5000, max_n=5000) == UNSUPPORTED   # 2049
        assert b"2048" in L.sa_last_error(None)
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(aff), 5000, FIT, max_m=1000, max_n=1047) == ARG           # 2048
        assert call(None, sa.SA_GLOBAL_GOTOH, C.byref(aff), 5000, FIT, max_m=1000, max_n=1048) == UNSUPPORTED
    # stricter than the host call: a 100 x 9000 pair seeded at 0 fits 4096 diagonals at w = 3995 there, not here
    assert sa.banded_seeded_plan_query(sa.SA_NW, 100, 9000, 0, 3995, FIT)[0] == 32
    assert _plan(L, sa.SA_NW, 100, 9000, 3995)[0] == UNSUPPORTED


def _expected_bound(affine, M, N, w):
    """(R of the bound's variant, record bytes) from the header's formulas, or None past the diagonal cap."""
    beff = min(2 * w + 1, M + N + 1)
    steps = min(M + N, 2 * M + 2 * w, 2 * N + 2 * w) + 2
    for R, Ln in VARIANTS[:7] if affine else VARIANTS:
        if beff <= 2 * R * Ln:
            if affine:
                words = -(-steps // (8 // R)) * Ln if R <= 8 else steps * (R // 8) * Ln
            else:
                words = -(-steps // (16 // R)) * Ln if R <= 16 else steps * 2 * Ln
            return R, 4 * words
    return None


@pytest.mark.parametrize("algo", ALGS)
def test_plan_query_returns_the_bound(algo):
    L = sa.load_library()
    affine = algo == sa.SA_GLOBAL_GOTOH
    shapes = [(0, 0), (1, 0), (0, 7), (12, 12), (40, 40), (150, 1000), (150, 100000), (2000, 2000), (3000, 17), (2 ** 24 - 1, 2 ** 24 - 1)]
    widths = [0, 1, 3, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 2 ** 31 - 1]
    taken = 0
    for M, N in shapes:
        for w in widths:
            exp = _expected_bound(affine, M, N, w)
            got = _plan(L, algo, M, N, w)
            if exp is None:
                assert got[0] == UNSUPPORTED, (M, N, w)
                continue
            assert got == (OK, exp[0], exp[1], 68), (M, N, w)
            taken += 1
    assert taken > 100
    assert sa.banded_seeded_device_plan_query(sa.SA_NW, 2000, 2000, 16) == (2, 32064, 68)
    with pytest.raises(sa.SeqalibError):
        sa.banded_seeded_device_plan_query(sa.SA_SW, 10, 10, 4)
