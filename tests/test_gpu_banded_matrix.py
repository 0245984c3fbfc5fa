"""Banded substitution-matrix alignment (sa_align_batch_banded_matrix, sa_score_batch_banded_matrix)
on the GPU, for SW, NW, LocalGotoh and GlobalGotoh.

Whole-matrix bands are checked against sa_align_batch_matrix, field for field and op for op; narrow
bands against tests/banded_matrix_model.py, the plain-dict model that tests/test_banded_matrix_model.py
pins.  Every comparison is exact.  Shapes are those of test_gpu_banded.py (ragged_pairs, narrow_cases,
mixed_pairs), with the sequences redrawn over the alphabet under test.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from banded_matrix_model import banded_matrix_model
from test_gpu_banded import AA, FIELDS, NARROW_W, mixed_pairs, narrow_cases, pair_ops, ragged_pairs, related, seq
from util import pack_bytes

pytestmark = pytest.mark.gpu

ALGS = [sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH]
LINEAR_VARIANTS = [(1, 4), (2, 4), (4, 4), (4, 2), (4, 1), (8, 1), (16, 1), (32, 1)]   # (cells per lane, pairs per wave)
AFFINE_VARIANTS = LINEAR_VARIANTS[:7]


def affine(algo):
    return algo >= sa.SA_LOCAL_GOTOH


def scoring(algo, k=0):
    """The k-th ScoringSystem arguments of the algorithm (match / mismatch are set to values a wrong
    read of them would show: the calls ignore them)."""
    return [(-3, -1, 1000, -1000), (-5, -2, 77, 55)][k] if affine(algo) else [(-2, 1000, -1000), (-4, 77, 55)][k]


def gaps(algo, args):
    return (args[0], args[1]) if affine(algo) else args[0]


def plan_query(algo, m, n, w):
    return (sa.banded_affine_plan_query if affine(algo) else sa.banded_plan_query)(algo, m, n, w)


def random_table(seed, lo=-8, hi=8):
    """An asymmetric 256 x 256 int16 table."""
    t = np.random.default_rng(seed).integers(lo, hi + 1, (256, 256)).astype(np.int16)
    assert (t != t.T).any()
    return t


def alphabet(k):
    """k byte values; from 20 symbols on they include 0x00 and 0xFF."""
    if k <= 3:
        return np.frombuffer(b"QAZ"[:k], dtype=np.uint8)
    if k == 20:
        return AA
    return np.array([0, 255] + list(range(60, 60 + k - 2)), dtype=np.uint8)


def redraw(pairs, alph, seed):
    """Related pairs of the same lengths over another alphabet."""
    rng = np.random.default_rng(seed)
    out = []
    for a, b in pairs:
        x = seq(rng, alph, len(a))
        out.append((x, related(rng, alph, x, len(b))))
    return out


def run_align(engine, algo, args, pairs, tab, w, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_banded_matrix_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, tab, w, lut)
    return res, ops, o1, o2


def run_score(engine, algo, args, pairs, tab, w, lut=None):
    return engine.score_banded_matrix_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), tab, w, lut)


def check_score_contract(score, res):
    for f in ("score", "end_i", "end_j"):
        assert np.array_equal(score[f], res[f]), f
    assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all()
    assert (score["flags"] == 0).all() and (score["reserved"] == 0).all()


_MODEL = {}


def model(algo, args, tab_key, rows, a, b, w, lut=None):
    """banded_matrix_model, computed once per input (tab_key names the table `rows`)."""
    if lut is not None:
        return banded_matrix_model(algo, gaps(algo, args), rows, a, b, w, lut)
    key = (algo, gaps(algo, args), tab_key, a, b, w)
    if key not in _MODEL:
        _MODEL[key] = banded_matrix_model(algo, gaps(algo, args), rows, a, b, w)
    return _MODEL[key]


def check_model(engine, algo, args, pairs, tab, tab_key, w, lut=None):
    """The align and the score call against the model, exactly; returns the models."""
    res, ops, o1, o2 = run_align(engine, algo, args, pairs, tab, w, lut)
    score = run_score(engine, algo, args, pairs, tab, w, lut)
    rows = np.asarray(tab).tolist()
    lrows = None if lut is None else np.asarray(lut).reshape(256, 256).tolist()
    out = []
    for p, (a, b) in enumerate(pairs):
        want = model(algo, args, tab_key, rows, a, b, w, lrows)
        out.append(want)
        r = res[p]
        got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
               pair_ops(res, ops, o1, o2, p))
        assert got == want, (algo, args, w, p, len(a), len(b))
        assert int(r["flags"]) == 0 and int(r["reserved"]) == 0
        assert b"X" not in got[5]
    check_score_contract(score, res)
    return out


def compare_with_matrix_call(engine, algo, args, pairs, tab, w, lut=None):
    """A whole-matrix band: every sa_result field and every op is sa_align_batch_matrix's."""
    s1, o1, s2, o2 = pack_bytes(pairs)
    sc = sa.ScoringSystem(*args)
    full, fops = engine.align_matrix_packed(algo, sc, s1, o1, s2, o2, tab, lut)
    assert (full["flags"] == 0).all()   # (the scorings used here set no flag in the matrix call)
    band, bops = engine.align_banded_matrix_packed(algo, sc, s1, o1, s2, o2, tab, w, lut)
    plan = engine.last_plan_ex()
    for f in FIELDS:
        assert np.array_equal(full[f], band[f]), (algo, args, f)
    for p in range(len(pairs)):
        assert pair_ops(band, bops, o1, o2, p) == pair_ops(full, fops, o1, o2, p), (algo, args, p)
    check_score_contract(engine.score_banded_matrix_packed(algo, sc, s1, o1, s2, o2, tab, w, lut), band)
    return plan


# ------------------------------------------------ 1. whole-matrix band = the full matrix path
@pytest.fixture(scope="module")
def ragged():
    # lengths <= 700: at most 1401 diagonals inside the matrix, within the affine fills' 2048
    return ragged_pairs(12, AA)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("merge", ["1", "0"])
def test_whole_matrix_band_equals_matrix_call(engine, monkeypatch, ragged, algo, merge):
    """merge = 0: every pair runs the narrowest variant that holds its clipped band."""
    monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
    tab = random_table(101)
    for k in (0, 1):
        plan = compare_with_matrix_call(engine, algo, scoring(algo, k), ragged, tab, 4096)
        assert (plan[0], plan[2], plan[3]) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_BAND4 if affine(algo) else sa.SA_RECORDS_BAND2)


# ------------------------------------------------------- 2. narrow bands against the model
NARROW_K = [1, 2, 3, 20, 63, 64]


@pytest.fixture(scope="module")
def narrow():
    """{w: (k, pairs)}: the shapes of narrow_cases() at every width, over alphabets of 1, 2, 3, 20, 63
    and 64 symbols in turn (odd K: dense int16 table rows that straddle 32-bit words)."""
    base = narrow_cases()
    out = {}
    for x, w in enumerate(NARROW_W):
        k = NARROW_K[x % len(NARROW_K)]
        out[w] = (k, redraw(base[w], alphabet(k), 300 + w))
    assert {k for k, _ in out.values()} == set(NARROW_K)
    assert out[3][0] == 20 and len(out[3][1]) >= 70   # the record-word boundary sweep, m + n = 65 .. 134
    return out


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("w", NARROW_W)
def test_narrow_band_matches_model(engine, narrow, algo, w):
    k, pairs = narrow[w]
    used = set(b"".join(a + b for a, b in pairs))
    assert len(used) <= k and (k < 63 or {0, 255} <= used)
    tab = random_table(102)
    check_model(engine, algo, scoring(algo, w % 2), pairs, tab, 102, w)
    assert engine.last_timings()[1] == 0   # (the score call ran last)
    kernel, _, waves, records = engine.last_plan_ex()
    assert (kernel, waves, records) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_NONE)
    run_align(engine, algo, scoring(algo), pairs[:3], tab, w)
    kernel, _, waves, records = engine.last_plan_ex()
    assert (kernel, waves, records) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_BAND4 if affine(algo) else sa.SA_RECORDS_BAND2)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("k", [1, 3, 63, 64])
def test_narrow_band_alphabet_sizes_at_the_word_boundary_sweep(engine, narrow, algo, k):
    """The m + n = 65 .. 134 sweep at w = 3 over the alphabets it did not get above."""
    pairs = redraw(narrow[3][1][-70:], alphabet(k), 400 + k)
    check_model(engine, algo, scoring(algo), pairs, random_table(103), 103, 3)


@pytest.mark.parametrize("algo", ALGS)
def test_all_negative_table(engine, narrow, algo):
    """No diagonal move gains: a local alignment is empty (score 0, no ops, start = end)."""
    tab = random_table(104, -8, -1)
    for w in (0, 3, 16):
        pairs = narrow[w][1][:15]
        models = check_model(engine, algo, scoring(algo), pairs, tab, 104, w)
        if algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH):
            for (a, b), (score, ei, ej, si, sj, ops) in zip(pairs, models):
                if a and b:
                    assert (score, ops, (si, sj)) == (0, b"", (ei, ej))


@pytest.mark.parametrize("algo", ALGS)
def test_extreme_table_entries(engine, algo):
    """Entries of +-32767 on pairs short enough for the score bound ((m + n + 1) * 32767 + 10000 < 2^29
    up to m + n = 16082; these have m + n <= 200)."""
    rng = np.random.default_rng(105)
    tab = rng.choice(np.array([-32767, 32767, -3, 5], dtype=np.int16), (256, 256))
    pairs = redraw([(b"x" * m, b"x" * n) for m, n in [(1, 1), (7, 9), (33, 31), (64, 64), (100, 97), (90, 110)]], AA, 106)
    for w in (0, 2, 16):
        check_model(engine, algo, scoring(algo), pairs, tab, 105, w)
    compare_with_matrix_call(engine, algo, scoring(algo), pairs, tab, 4096)


# ------------------------------------------- 3. every variant is reached, and reached unmerged
def variant_shapes(algo):
    """{variant: three (m, n)} whose whole-matrix band (m + n + 1 diagonals) needs exactly that variant;
    the widest ones are the smallest shapes that reach them."""
    shapes = {(1, 4): [(15, 16), (9, 3), (1, 20)], (2, 4): [(30, 33), (17, 16), (40, 2)],
              (4, 4): [(60, 67), (33, 32), (100, 9)], (4, 2): [(120, 135), (65, 64), (3, 200)],
              (4, 1): [(250, 261), (129, 128), (300, 100)], (8, 1): [(500, 523), (257, 256), (513, 300)],
              (16, 1): [(520, 600), (513, 515), (700, 690)]}
    if not affine(algo):
        shapes[(32, 1)] = [(1500, 1490), (1100, 1300), (1027, 1029)]
    return shapes


@pytest.mark.parametrize("algo", ALGS)
def test_every_variant_unmerged(engine, monkeypatch, algo):
    monkeypatch.setenv("SEQALIB_BAND_MERGE", "0")
    shapes = variant_shapes(algo)
    assert list(shapes) == (AFFINE_VARIANTS if affine(algo) else LINEAR_VARIANTS)
    tab = random_table(107)
    for x, (variant, mn) in enumerate(shapes.items()):
        assert {plan_query(algo, m, n, 4096)[:2] for m, n in mn} == {variant}
        pairs = redraw([(b"x" * m, b"x" * n) for m, n in mn], AA, 500 + x)
        plan = compare_with_matrix_call(engine, algo, scoring(algo, x % 2), pairs, tab, 4096)
        assert plan[1] == variant[0], (variant, plan)
        assert engine.last_timings()[2] == 1


# ------------------------------------------------------------- 4. mixed bands in one call
@pytest.fixture(scope="module")
def mixed():
    return redraw(mixed_pairs(), AA, 108)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("merge", ["0", "1"])
def test_mixed_bands_in_one_call(engine, monkeypatch, mixed, algo, merge):
    monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
    shapes = {plan_query(algo, len(a), len(b), 2)[:2] for a, b in mixed}
    assert len(shapes) >= 4, shapes
    check_model(engine, algo, scoring(algo), mixed, random_table(109), 109, 2)


@pytest.mark.parametrize("algo", ALGS)
def test_one_call_split_into_several_launches(engine, mixed, algo):
    """A workspace limit of exactly the largest pair's own records (the plan query's bytes): the call
    runs in several launches and its results are exact."""
    limit = max(plan_query(algo, len(a), len(b), 2)[2] for a, b in mixed)
    tab = random_table(109)
    run_align(engine, algo, scoring(algo), mixed, tab, 2)
    unlimited = engine.last_timings()[2]
    try:
        engine.set_workspace_limit(limit)
        check_model(engine, algo, scoring(algo), mixed, tab, 109, 2)
        run_align(engine, algo, scoring(algo), mixed, tab, 2)
        assert engine.last_timings()[2] > unlimited
    finally:
        engine.set_workspace_limit(0)


# ----------------------------------------------------------------------------- 5. labels
@pytest.mark.parametrize("algo", ALGS)
def test_match_lut_changes_labels_only(engine, narrow, algo):
    lut = (np.arange(256)[:, None] % 10 == np.arange(256)[None, :] % 10).astype(np.uint8)
    tab = random_table(110)
    pairs = narrow[15][1]
    assert narrow[15][0] == 63   # many symbols: classes that differ from equality
    for w in (15, 4096):
        plain, pops, o1, o2 = run_align(engine, algo, scoring(algo), pairs, tab, w)
        named, nops, _, _ = run_align(engine, algo, scoring(algo), pairs, tab, w, lut)
        for f in FIELDS:
            assert np.array_equal(plain[f], named[f]), (w, f)
        changed = 0
        for p in range(len(pairs)):
            x, y = pair_ops(plain, pops, o1, o2, p), pair_ops(named, nops, o1, o2, p)
            assert x.replace(b"M", b"S") == y.replace(b"M", b"S"), (w, p)
            changed += x != y
        assert changed
    check_model(engine, algo, scoring(algo), pairs, tab, 110, 15, lut)
    compare_with_matrix_call(engine, algo, scoring(algo), pairs, tab, 4096, lut)


# ---------------------------------------------------------------------- 6. degenerate batches
@pytest.mark.parametrize("algo", ALGS)
def test_degenerate_batches(engine, algo):
    tab = random_table(111)
    args = scoring(algo)
    # the call without a table, with the same gap terms
    plain = (engine.align_banded_affine_packed if affine(algo) else engine.align_banded_packed)
    plain_sc = sa.ScoringSystem(*((args[0], args[1], 1, -1) if affine(algo) else (args[0], 1, -1)))
    for pairs in ([(b"", b"")] * 3,                                  # no symbol at all: K = 0
                  [(b"", b"ACD"), (b"ACDE", b""), (b"", b"")],       # one side empty
                  [(b"", b"ACD"), (b"ACDE", b"AC"), (b"A", b"")]):
        for w in (0, 2, 4096):
            check_model(engine, algo, args, pairs, tab, 111, w)
            if all(not a or not b for a, b in pairs):   # empty inputs: what the calls without a table give
                res, ops, o1, o2 = run_align(engine, algo, args, pairs, tab, w)
                want, wops = plain(algo, plain_sc, *pack_bytes(pairs), w)
                for f in FIELDS:
                    assert np.array_equal(res[f], want[f]), (pairs, w, f)
                for p in range(len(pairs)):
                    assert pair_ops(res, ops, o1, o2, p) == pair_ops(want, wops, o1, o2, p)
    res, ops, _, _ = run_align(engine, algo, args, [], tab, 2)       # npairs = 0
    assert len(res) == 0
    assert len(run_score(engine, algo, args, [], tab, 2)) == 0
    a64 = bytes(range(100, 164))
    ok = [(a64[:40] * 2, a64[30:] * 2), (a64[::-1], a64)]
    check_model(engine, algo, args, ok, tab, 111, 5)                 # 64 symbols
    for bad in ([(a64[:40], a64[30:] + b"\x00")], [(a64, b""), (b"", b"\xff")]):   # 65, both sides together
        with pytest.raises(sa.SeqalibError):
            run_align(engine, algo, args, bad, tab, 5)
        with pytest.raises(sa.SeqalibError):
            run_score(engine, algo, args, bad, tab, 5)


def test_argument_checks_on_the_engine(engine):
    tab = random_table(112)
    pair = [(b"ACDE", b"ACE")]
    for algo in (sa.SA_HIRSCHBERG, sa.SA_MYERS_MILLER):
        with pytest.raises(sa.SeqalibError):
            run_align(engine, algo, (-3, -1, 1, -1), pair, tab, 2)
    for algo in (sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH):
        with pytest.raises(sa.SeqalibError):
            run_align(engine, algo, (-3, 1, 1, -1), pair, tab, 2)    # gap_extend > 0
        check_model(engine, algo, (-3, -1, 2, -1, False), pair, tab, 112, 0)   # band 0, allow_mismatch = 0: valid
    for algo in (sa.SA_SW, sa.SA_NW):
        check_model(engine, algo, (-1, 2), pair, tab, 112, 0)
    with pytest.raises(sa.SeqalibError):
        run_align(engine, sa.SA_NW, (-2, 1, -1), [(b"A" * 100, b"A" * 5000)], tab, 4)   # 4909 diagonals


# --------------------------------------------------------------------- 7. Python classes
def test_python_classes(engine):
    rng = np.random.default_rng(3)
    pairs = []
    for m, n in [(40, 44), (100, 91), (7, 0), (150, 150)]:
        a = seq(rng, AA, m)
        pairs.append((a.decode(), related(rng, AA, a, n).decode()))
    tab = random_table(113)
    rows = tab.tolist()
    for cls, algo in [(sa.SmithWatermanSA, sa.SA_SW), (sa.NeedlemanWunschSA, sa.SA_NW),
                      (sa.LocalGotohSA, sa.SA_LOCAL_GOTOH), (sa.GlobalGotohSA, sa.SA_GLOBAL_GOTOH)]:
        args = scoring(algo)
        al = cls(sa.ScoringSystem(*args), matrix=tab)
        got = al.getBandedMatrixAlignments(pairs, 4)
        scores = al.getBandedMatrixScores(pairs, 4)
        models = [banded_matrix_model(algo, gaps(algo, args), rows, a.encode(), b.encode(), 4) for a, b in pairs]
        for (a, b), g, s, (sc, ei, ej, si, sj, ops) in zip(pairs, got, scores, models):
            want = sa.expand_ops(algo, a, b, sa.PairResult(sc, ei, ej, si, sj, 0, ops))
            assert g.rows() == want.rows()
            assert s == sc
        assert al.getScore() == models[-1][0]
        assert al.getBandedMatrixAlignment(*pairs[0], 4).rows() == got[0].rows()
        if algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH):
            assert al.getBandedMatrixEndCells(pairs, 4) == [x[1:3] for x in models]
        else:
            assert not hasattr(al, "getBandedMatrixEndCells")
        with pytest.raises(sa.SeqalibError):    # the old doors keep answering as they did
            al.getAlignments(pairs, band=4)
        with pytest.raises(sa.SeqalibError):
            al.getScores(pairs, band=4)
        if affine(algo):
            with pytest.raises(sa.SeqalibError):
                al.getBandedAlignments(pairs, 4)
            with pytest.raises(sa.SeqalibError):
                al.getBandedScores(pairs, 4)
        without = cls(sa.ScoringSystem(*args))
        with pytest.raises(sa.SeqalibError):
            without.getBandedMatrixAlignments(pairs, 4)
        with pytest.raises(sa.SeqalibError):
            without.getBandedMatrixScores(pairs, 4)
    for cls in (sa.HirschbergSA, sa.MyersMillerSA):
        assert not hasattr(cls, "getBandedMatrixAlignments") and not hasattr(cls, "getBandedMatrixScores")
