"""CPU: the matrix entry points (sa_align_batch_matrix, sa_score_batch_matrix, sa_matrix_plan_query,
include/seqalib_hip.h) are exported, their argument and limit checks answer without a device (a NULL
context), and the host-only planner reports the int32 plan.  No GPU compute is called here."""
import ctypes as C

import numpy as np
import pytest

import seqalib_amd as sa

ERR_ARG, ERR_UNSUPPORTED = -1, -5
MATRIX_SYMBOLS = ["sa_align_batch_matrix", "sa_score_batch_matrix", "sa_matrix_plan_query"]


def test_matrix_symbols_exported():
    L = sa.load_library()
    missing = [s for s in MATRIX_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert L.sa_version() == 1   # the change only adds symbols


def call(kind, ctx, algo, sc, pairs, submat):
    """sa_align_batch_matrix / sa_score_batch_matrix on host buffers with context `ctx` (None: NULL)."""
    L = sa.load_library()
    s1, o1, s2, o2 = sa.pack_pairs(pairs)
    n = len(pairs)
    res = np.zeros(max(n, 1), dtype=sa.RESULT_DTYPE)
    cap = int(o1[-1] + o2[-1]) + n + 1
    ops = np.zeros(cap, dtype=np.uint8)
    tab = None if submat is None else np.ascontiguousarray(submat, dtype=np.int16).reshape(65536)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    scp = None if sc is None else C.byref(sc)
    if kind == "align":
        return L.sa_align_batch_matrix(ctx, algo, scp, p(s1), p(o1), p(s2), p(o2), n, p(tab), None, p(res), p(ops), cap)
    return L.sa_score_batch_matrix(ctx, algo, scp, p(s1), p(o1), p(s2), p(o2), n, p(tab), None, p(res))


@pytest.mark.parametrize("kind", ["align", "score"])
def test_matrix_argument_checks(kind):
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    aff = sa.ScoringSystem(-3, -1, 1, -1)._c()
    tab = np.ones((256, 256), dtype=np.int16)
    pairs = [(b"ACGT", b"AGT"), (b"", b"T")]
    for algo in (sa.SA_SW, sa.SA_NW):
        assert call(kind, None, algo, lin, pairs, tab) == ERR_ARG           # valid: only the context is missing
    for algo in (sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH):
        assert call(kind, None, algo, aff, pairs, tab) == ERR_ARG
    for algo in (sa.SA_HIRSCHBERG, sa.SA_MYERS_MILLER):
        assert call(kind, None, algo, aff, pairs, tab) == ERR_UNSUPPORTED
    assert b"SA_SW" in sa.load_library().sa_last_error(None)
    assert call(kind, None, 9, lin, pairs, tab) == ERR_ARG
    assert call(kind, None, sa.SA_NW, None, pairs, tab) == ERR_ARG          # NULL scoring
    assert call(kind, None, sa.SA_NW, lin, pairs, None) == ERR_ARG          # NULL submat
    assert call(kind, None, sa.SA_NW, lin, [], tab) == ERR_ARG              # an empty batch: still the context


@pytest.mark.parametrize("kind", ["align", "score"])
def test_matrix_symbol_limit(kind):
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    tab = np.zeros((256, 256), dtype=np.int16)
    s64 = bytes(range(100, 164))
    assert call(kind, None, sa.SA_SW, lin, [(s64[:40], s64[30:])], tab) == ERR_ARG          # 64 symbols, both sides together
    assert call(kind, None, sa.SA_SW, lin, [(s64[:40], s64[30:] + b"\x00")], tab) == ERR_UNSUPPORTED   # 65
    assert b"64" in sa.load_library().sa_last_error(None)
    assert call(kind, None, sa.SA_SW, lin, [(s64, b""), (b"", b"\xff")], tab) == ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", ["align", "score"])
def test_matrix_score_bound_edge(kind):
    """(m + n + 1) * max(|gap terms|, max |S| over the batch's symbols) >= 2^29 is refused, one less is
    taken -- by the gap term, by a table entry, and by an affine term; entries of absent symbols do
    not count."""
    tab = np.zeros((256, 256), dtype=np.int16)
    tab[ord("A"), ord("C")] = -16384               # |S| = 2^14: m + n + 1 = 2^15 is the edge
    tab[ord("Z"), ord("Z")] = 32767                # never read: Z is not in the batch
    lin = sa.ScoringSystem(-1, 1, -1)._c()
    a = b"A" * 16384
    assert call(kind, None, sa.SA_NW, lin, [(a, b"C" * 16383)], tab) == ERR_UNSUPPORTED
    assert b"2^29" in sa.load_library().sa_last_error(None)
    assert call(kind, None, sa.SA_NW, lin, [(a, b"C" * 16382)], tab) == ERR_ARG
    big_gap = sa.ScoringSystem(-(2 ** 20), 1, -1)._c()   # m + n + 1 = 512 is the edge
    assert call(kind, None, sa.SA_SW, big_gap, [(b"A" * 256, b"A" * 255)], tab) == ERR_UNSUPPORTED
    assert call(kind, None, sa.SA_SW, big_gap, [(b"A" * 255, b"A" * 255)], tab) == ERR_ARG
    big_ext = sa.ScoringSystem(-3, 2 ** 20, 1, -1)._c()
    assert call(kind, None, sa.SA_GLOBAL_GOTOH, big_ext, [(b"A" * 256, b"A" * 255)], tab) == ERR_UNSUPPORTED
    assert call(kind, None, sa.SA_GLOBAL_GOTOH, big_ext, [(b"A" * 255, b"A" * 255)], tab) == ERR_ARG
    # match / mismatch are ignored: a huge match does not count
    huge = sa.ScoringSystem(-1, 2 ** 30, -(2 ** 30))._c()
    assert call(kind, None, sa.SA_SW, huge, [(b"A" * 255, b"A" * 255)], tab) == ERR_ARG


SHAPES = [(4096, 4096, 1000), (4096, 4096, 2000), (300, 5000, 4000), (100, 100, 3), (9000, 300, 3), (513, 700, 40),
          (4096, 4096, 1), (20000, 20000, 8), (70, 50000, 1)]


@pytest.mark.parametrize("algo", [sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH])
def test_matrix_plan_is_the_int32_plan(algo, monkeypatch):
    """The matrix call runs the int32 kernel alone on the int32 planner's plan: what sa_plan_query_ex
    reports for a 20-letter batch when no 16-bit variant is enqueued beside it (SEQALIB_T16=0; with one,
    sa_plan_query_ex adds that variant's workspace), and -- kernel and rows per lane -- what
    sa_score_plan_query reports (whose record-free fill may cap the waves)."""
    sc = sa.ScoringSystem(-3, -1, 1, -1) if algo >= 2 else sa.ScoringSystem(-1, 1, -1)
    monkeypatch.setenv("SEQALIB_T16", "0")
    for m, n, npairs in SHAPES:
        got = sa.matrix_plan_query(algo, sc, m, n, npairs, 20)
        assert got == sa.plan_query_ex(algo, sc, m, n, npairs, 20), (m, n, npairs)
        assert got[0] == sa.SA_KERNEL_INT32
        score = sa.score_plan_query(algo, sc, m, n, npairs, 20)
        assert got[:2] == score[:2] and score[2] <= got[2] and score[3] <= got[3], (m, n, npairs)
    monkeypatch.delenv("SEQALIB_T16")
    for m, n, npairs in SHAPES:   # the scoring's match / mismatch and the environment do not matter
        assert sa.matrix_plan_query(algo, sc, m, n, npairs, 64) == sa.matrix_plan_query(algo, sc, m, n, npairs, 1)
    L = sa.load_library()
    c = sc._c()
    assert L.sa_matrix_plan_query(algo, C.byref(c), 100, 100, 1, 65, None, None, None, None) == ERR_UNSUPPORTED
    assert L.sa_matrix_plan_query(algo, C.byref(c), 2 ** 24, 100, 1, 20, None, None, None, None) == ERR_UNSUPPORTED
    assert L.sa_matrix_plan_query(algo, None, 100, 100, 1, 20, None, None, None, None) == ERR_ARG
    assert L.sa_matrix_plan_query(sa.SA_HIRSCHBERG, C.byref(c), 100, 100, 1, 20, None, None, None, None) == ERR_UNSUPPORTED
