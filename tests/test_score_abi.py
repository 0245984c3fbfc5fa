"""CPU: the score-only entry points (sa_score_batch*, include/seqalib_hip.h) are exported, and the
host-only planner of a score call, sa_score_plan_query, provisions no direction records for the
int32 kernel family.  No GPU compute is called here."""
import ctypes as C

import pytest

import seqalib_amd as sa

SCORE_SYMBOLS = ["sa_score_batch", "sa_score_batch_bits", "sa_score_batch_device", "sa_multi_score_batch",
                 "sa_score_plan_query"]

# the class defaults (SASmithWaterman.h:352, the others (-1, 2, -1)); affine ones as the golden corpus
DEFAULTS = {sa.SA_SW: sa.ScoringSystem(-1, 1, -1), sa.SA_NW: sa.ScoringSystem(-1, 2, -1),
            sa.SA_LOCAL_GOTOH: sa.ScoringSystem(-3, -1, 1, -1), sa.SA_GLOBAL_GOTOH: sa.ScoringSystem(-3, -1, 1, -1)}


def test_score_symbols_exported():
    L = sa.load_library()
    missing = [s for s in SCORE_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert sa.SA_RECORDS_NONE == 3
    assert L.sa_version() == 1   # the change only adds symbols


@pytest.mark.parametrize("algo", [sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH])
def test_score_plan_has_no_records(algo):
    """20 letters, 4096 x 4096, 1,000 pairs: the align plan holds >= 4 MiB of records per pair, the
    score plan row buffers of tens of KiB."""
    sc = DEFAULTS[algo]
    k_a, R_a, W_a, ws_align = sa.plan_query_ex(algo, sc, 4096, 4096, 1000, nsym=20)
    k_s, R_s, W_s, ws_score = sa.score_plan_query(algo, sc, 4096, 4096, 1000, nsym=20)
    print(f"algo {algo}: align ({k_a}, {R_a}, {W_a}) {ws_align} B/pair, score ({k_s}, {R_s}, {W_s}) {ws_score} B/pair")
    assert k_s == sa.SA_KERNEL_INT32
    assert ws_align >= 4 << 20
    assert ws_score < ws_align
    assert ws_score * 16 < ws_align
    assert ws_score <= 64 << 10


@pytest.mark.parametrize("algo", [sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH])
@pytest.mark.parametrize("shape", [(4096, 4096, 10000), (1024, 1024, 10000), (4096, 4096, 1), (300, 300, 1100)])
def test_score_plan_dna_keeps_kernel_family(algo, shape):
    m, n, npairs = shape
    sc = DEFAULTS[algo]
    assert sa.score_plan_query(algo, sc, m, n, npairs, nsym=4)[:3] == sa.plan_query_ex(algo, sc, m, n, npairs, nsym=4)[:3]


def test_score_plan_hirschberg_is_nw():
    sc = sa.ScoringSystem(-1, 2, -1)
    assert sa.score_plan_query(sa.SA_HIRSCHBERG, sc, 2048, 2048, 100, nsym=20) == \
        sa.score_plan_query(sa.SA_NW, sc, 2048, 2048, 100, nsym=20)


def test_score_myers_miller_unsupported():
    L = sa.load_library()
    sc = sa.ScoringSystem(-3, -1, 1, -1)._c()
    ws = C.c_uint64()
    rc = L.sa_score_plan_query(sa.SA_MYERS_MILLER, C.byref(sc), 100, 100, 10, 4, None, None, None, C.byref(ws))
    assert rc == -5   # SA_ERR_UNSUPPORTED
    assert b"MYERS_MILLER" in L.sa_last_error(None)
    with pytest.raises(sa.SeqalibError):
        sa.score_plan_query(sa.SA_MYERS_MILLER, sa.ScoringSystem(-3, -1, 1, -1), 100, 100, 10)


def test_score_plan_argument_checks():
    L = sa.load_library()
    sc = sa.ScoringSystem(-1, 1, -1)._c()
    assert L.sa_score_plan_query(7, C.byref(sc), 10, 10, 1, 4, None, None, None, None) == -1
    assert L.sa_score_plan_query(0, None, 10, 10, 1, 4, None, None, None, None) == -1
    assert L.sa_score_batch(None, 0, C.byref(sc), None, None, None, None, 0, None, None) == -1
    assert L.sa_score_batch_bits(None, 0, C.byref(sc), None, None, 0, None, None, None) == -1
    assert L.sa_score_batch_device(None, 0, C.byref(sc), None, None, None, None, 0, 0, 0, None, None, None) == -1
    assert L.sa_multi_score_batch(None, 0, C.byref(sc), None, None, None, None, 0, None, None) == -1
