"""Substitution-matrix scoring (sa_align_batch_matrix, sa_score_batch_matrix) on the GPU.

A degenerate table (S = match on the diagonal, mismatch elsewhere) must reproduce sa_align_batch field
for field; real tables are checked against tests/submat_model.py, the plain-Python model that
tests/test_submat_model.py pins against the oracle.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from submat_model import model_align
from test_gpu_banded import AA, ACGT, FIELDS, pair_ops, ragged_pairs, related, seq
from util import named_lut, pack_bytes, scoring_fields

pytestmark = pytest.mark.gpu

ALGS = [sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH]
LIN = [(-1, 1, -1), (-2, 2, -3)]
AFF = [(-3, -1, 1, -1), (-5, -2, 4, -3)]
HACK_SIZES = {(314, 288), (60, 57), (61, 58)}


def scorings(algo):
    return AFF if algo >= sa.SA_LOCAL_GOTOH else LIN


def gaps_of(algo, args):
    g, _, _, go, ge, _ = scoring_fields(args)
    return (go, ge) if algo >= sa.SA_LOCAL_GOTOH else g


def degenerate_table(args, lut=None):
    _, ma, mi, _, _, _ = scoring_fields(args)
    eq = np.eye(256, dtype=bool) if lut is None else (np.asarray(lut).reshape(256, 256) != 0)
    return np.where(eq, ma, mi).astype(np.int16)


def run_matrix(engine, algo, args, pairs, tab, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_matrix_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, tab, lut)
    return res, ops, o1, o2


def check_score_contract(score, res):
    for f in ("score", "end_i", "end_j"):
        assert np.array_equal(score[f], res[f]), f
    assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all()
    assert (score["reserved"] == 0).all() and (score["flags"] == 0).all()


def check_model(engine, algo, args, pairs, tab, lut=None, models=None):
    """Align and score calls against the model; returns the models (one dict per pair)."""
    res, ops, o1, o2 = run_matrix(engine, algo, args, pairs, tab, lut)
    score = engine.score_matrix_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), tab, lut)
    rows = np.asarray(tab).reshape(256, 256).tolist()
    out = []
    for p, (a, b) in enumerate(pairs):
        want = models[p] if models else model_align(algo, gaps_of(algo, args), rows, a, b, lut)
        out.append(want)
        r = res[p]
        where = (algo, args, p, len(a), len(b))
        assert (int(r["score"]), int(r["end_i"]), int(r["end_j"])) == (want["score"], want["end_i"], want["end_j"]), where
        assert (int(score["score"][p]), int(score["end_i"][p]), int(score["end_j"][p])) == \
            (want["score"], want["end_i"], want["end_j"]), where
        if want["diverged"]:   # the reference's walk does not terminate: LocalGotoh flags it
            assert algo == sa.SA_LOCAL_GOTOH and int(r["flags"]) == sa.SA_FLAG_DIVERGED, where
            continue
        assert (int(r["start_i"]), int(r["start_j"]), pair_ops(res, ops, o1, o2, p)) == \
            (want["start_i"], want["start_j"], want["ops"]), where
        assert int(r["flags"]) == 0 and int(r["reserved"]) == 0, where
        assert b"X" not in want["ops"]
    assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all()
    assert (score["reserved"] == 0).all() and (score["flags"] == 0).all()
    return out


# --------------------------------------------------- 1. a degenerate table = sa_align_batch
@pytest.fixture(scope="module")
def ragged():
    return {"dna": ragged_pairs(11, ACGT), "aa": ragged_pairs(12, AA)}


def drop_hack_sizes(algo, pairs):
    if algo != sa.SA_LOCAL_GOTOH:
        return pairs
    kept = [(a, b) for a, b in pairs if (len(a), len(b)) not in HACK_SIZES]
    assert len(pairs) - len(kept) <= len(pairs) // 20
    return kept


def compare_with_align_batch(engine, algo, args, pairs, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    sc = sa.ScoringSystem(*args)
    full, fops = engine.align_packed(algo, sc, s1, o1, s2, o2, lut)
    assert engine.last_plan_ex()[0] == sa.SA_KERNEL_INT32
    plan = engine.last_plan_ex()
    mat, mops = engine.align_matrix_packed(algo, sc, s1, o1, s2, o2, degenerate_table(args, lut), lut)
    assert engine.last_plan_ex() == plan == (sa.SA_KERNEL_INT32, plan[1], plan[2], sa.SA_RECORDS_FLAGS)
    for f in FIELDS:
        assert np.array_equal(full[f], mat[f]), (algo, args, f)
    for p in range(len(pairs)):
        assert pair_ops(mat, mops, o1, o2, p) == pair_ops(full, fops, o1, o2, p), (algo, args, p)
    score = engine.score_matrix_packed(algo, sc, s1, o1, s2, o2, degenerate_table(args, lut), lut)
    assert engine.last_plan_ex()[3] == sa.SA_RECORDS_NONE
    for f in ("score", "end_i", "end_j"):
        assert np.array_equal(score[f], mat[f]), (algo, args, f)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("alphabet", ["dna", "aa"])
def test_degenerate_table_equals_align_batch(engine, monkeypatch, ragged, algo, alphabet):
    monkeypatch.setenv("SEQALIB_T16", "0")
    monkeypatch.setenv("SEQALIB_TINY", "0")
    pairs = drop_hack_sizes(algo, ragged[alphabet])
    for args in scorings(algo):
        compare_with_align_batch(engine, algo, args, pairs)


@pytest.mark.parametrize("algo", ALGS)
def test_degenerate_table_named_lut(engine, monkeypatch, algo):
    """named_lut("nwild") as the label LUT and as the score rule."""
    monkeypatch.setenv("SEQALIB_T16", "0")
    monkeypatch.setenv("SEQALIB_TINY", "0")
    pairs = drop_hack_sizes(algo, ragged_pairs(13, np.frombuffer(b"ACGTN", dtype=np.uint8), extra=10)[::2])
    compare_with_align_batch(engine, algo, scorings(algo)[1], pairs, named_lut("nwild"))


@pytest.mark.parametrize("algo", ALGS)
def test_degenerate_table_many_pairs(engine, monkeypatch, algo):
    """1030 pairs: the many-pairs plan (one wave per pair, R = 8 here) and a launch of more than one
    workgroup of the one-lane-per-pair walk."""
    monkeypatch.setenv("SEQALIB_T16", "0")
    rng = np.random.default_rng(70 + algo)
    pairs = []
    for k in range(1030):
        a = seq(rng, AA, 100 + k % 300)
        pairs.append((a, related(rng, AA, a, 90 + k % 250) if k % 2 else seq(rng, AA, 80 + k % 200)))
    pairs = drop_hack_sizes(algo, pairs)
    compare_with_align_batch(engine, algo, scorings(algo)[0], pairs)
    assert engine.last_plan_ex()[1:3] == (8, 1)


# ------------------------------------------------------- 2. real tables against the model
def table_over(alphabet, values):
    t = np.zeros((256, 256), dtype=np.int16)
    t[np.ix_(alphabet, alphabet)] = values
    return t


def real_tables():
    rng = np.random.default_rng(2025)
    k = len(AA)
    asym = rng.integers(-8, 13, (k, k))
    # positive off-diagonal entries: 'S' ops with positive terms
    pos = np.where(np.eye(k, dtype=bool), 5, rng.integers(-6, 4, (k, k)))
    neg = rng.integers(-9, 0, (k, k))
    return {"asym": table_over(AA, asym), "posoff": table_over(AA, pos), "neg": table_over(AA, neg)}


def model_pairs(seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for L in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        a = seq(rng, AA, L)
        pairs.append((a, related(rng, AA, a, 37)))
        b = seq(rng, AA, 29)
        pairs.append((b, related(rng, AA, b, L)))
    a = seq(rng, AA, 257)
    pairs.append((a, related(rng, AA, a, 257)))
    a = seq(rng, AA, 513)
    pairs.append((a, related(rng, AA, a, 300)))
    pairs.append((seq(rng, AA, 65), seq(rng, AA, 64)))
    return pairs


@pytest.fixture(scope="module")
def tables():
    return real_tables()


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("name", ["asym", "posoff", "neg"])
def test_real_tables_match_model(engine, tables, algo, name):
    tab = tables[name]
    args = scorings(algo)[0]
    models = check_model(engine, algo, args, model_pairs(31), tab)
    if name == "posoff":
        assert any(b"S" in w["ops"] for w in models)
    if name == "neg" and algo == sa.SA_SW:   # every cell is 0: the last cell of the matrix, an empty path
        assert all((w["score"], w["ops"]) == (0, b"") for w in models if w["end_i"])
    if name == "neg" and algo == sa.SA_LOCAL_GOTOH:
        assert all(w["score"] == 0 for w in models)


@pytest.mark.parametrize("algo", ALGS)
def test_unstaged_seq2_matches_model(engine, tables, algo):
    """A 3 x 50,000 pair: Seq2 is longer than the LDS stage, so the whole launch reads it from memory."""
    rng = np.random.default_rng(77)
    pairs = [(seq(rng, AA, 3), seq(rng, AA, 50000)), (seq(rng, AA, 70), seq(rng, AA, 90))]
    check_model(engine, algo, scorings(algo)[0], pairs, tables["asym"])


@pytest.mark.parametrize("k", [1, 2, 64])
def test_alphabet_sizes_match_model(engine, k):
    """K = 1, 2, 64 distinct symbols, the symbol bytes 0 and 255 among them."""
    rng = np.random.default_rng(900 + k)
    alphabet = np.array(([0] if k == 1 else [0, 255] + list(range(60, 60 + k - 2))), dtype=np.uint8)
    tab = table_over(alphabet, rng.integers(-8, 13, (k, k)))
    lut = np.zeros((256, 256), dtype=np.uint8)   # a label rule of its own: a ~ b when a = b mod 3
    for a in range(256):
        lut[a, a % 3::3] = 1
    pairs = [(seq(rng, alphabet, m), seq(rng, alphabet, n)) for m, n in
             [(0, 0), (1, 1), (0, 9), (9, 0), (64, 65), (130, 97), (97, 130), (257, 40)]]
    if k == 64:   # every symbol occurs
        pairs.append((alphabet.tobytes(), alphabet[::-1].tobytes()))
    for algo in ALGS:
        check_model(engine, algo, scorings(algo)[k % 2], pairs, tab, lut if k != 1 else None)


# ------------------------------------------------------------------------ 3. forced plans
def plan_pairs():
    rng = np.random.default_rng(5)
    pairs = []
    for m, n in [(1030, 120), (520, 300), (120, 1030), (257, 64), (64, 257), (0, 5), (5, 0), (1, 1)]:
        a = seq(rng, AA, m)
        pairs.append((a, related(rng, AA, a, n)))
    return pairs


@pytest.fixture(scope="module")
def plan_reference(tables):
    """The model's results for plan_pairs(), all four algorithms (computed once)."""
    rows = tables["asym"].tolist()
    pairs = plan_pairs()
    return {algo: [model_align(algo, gaps_of(algo, scorings(algo)[0]), rows, a, b) for a, b in pairs] for algo in ALGS}


PLANS = ["1,0", "2,0", "4,0", "8,0", "4,1", "8,1", "16,1", "4,4", "8,3", "16,16"]
SETTINGS = [("SEQALIB_PLAN", p) for p in PLANS] + [("SEQALIB_TB", "wave"), ("SEQALIB_TB", "lane"), ("SEQALIB_TB", "seg"),
                                                     ("SEQALIB_SPLIT", "0"), ("SEQALIB_TINY", "0"), ("SEQALIB_TINY", "1"),
                                                     ("SEQALIB_T16", "1"), ("SEQALIB_STAGE_SEQ2", "0")]


@pytest.mark.parametrize("setting", [None] + SETTINGS, ids=lambda s: "default" if s is None else "=".join(s))
def test_forced_plans_do_not_change_results(engine, monkeypatch, tables, plan_reference, setting):
    """Whatever the switches say -- honoured (SEQALIB_PLAN, SEQALIB_SPLIT, SEQALIB_STAGE_SEQ2) or ignored
    (SEQALIB_TB, SEQALIB_TINY, SEQALIB_T16) -- a matrix call returns the model's results."""
    if setting:
        monkeypatch.setenv(*setting)
    pairs = plan_pairs()
    for algo in ALGS:
        check_model(engine, algo, scorings(algo)[0], pairs, tables["asym"], models=plan_reference[algo])
        kernel, R, W, records = engine.last_plan_ex()   # (the score call ran last)
        assert (kernel, records) == (sa.SA_KERNEL_INT32, sa.SA_RECORDS_NONE)
        if setting and setting[0] == "SEQALIB_PLAN":
            r, w = map(int, setting[1].split(","))
            assert R == r and (W == 0) == (w == 0)
        if setting == ("SEQALIB_SPLIT", "0"):
            assert W > 0


# ------------------------------------------------------------------------- 4. keyed bound
@pytest.mark.parametrize("algo", [sa.SA_SW, sa.SA_LOCAL_GOTOH])
@pytest.mark.parametrize("s", [1000, 600])
def test_local_scores_around_the_key_bound(engine, algo, s):
    """100 identical symbols: 100 * 1000 = 100,000 does not fit a 16-bit (score, column) key, 60,000
    does.  scoring.match (1) must not be what the bound is computed from."""
    tab = np.full((256, 256), -3, dtype=np.int16)
    tab[ord("K"), ord("K")] = s
    tab[ord("Q"), ord("Q")] = 2   # a used symbol with a smaller entry
    pairs = [(b"K" * 100, b"K" * 100), (b"Q" + b"K" * 100, b"K" * 100 + b"QQ")]
    models = check_model(engine, algo, scorings(algo)[0], pairs, tab)
    assert models[0]["score"] == 100 * s and (models[0]["end_i"], models[0]["end_j"]) == (100, 100)


# -------------------------------------------------------------------------- 5. score call
@pytest.mark.parametrize("algo", ALGS)
def test_score_call_contract(engine, tables, algo):
    pairs = model_pairs(41)[::3] + plan_pairs()[:2]
    args = scorings(algo)[1]
    res, _, _, _ = run_matrix(engine, algo, args, pairs, tables["asym"])
    assert engine.last_plan_ex()[3] == sa.SA_RECORDS_FLAGS
    assert engine.last_timings()[1] > 0
    score = engine.score_matrix_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), tables["asym"])
    check_score_contract(score, res)
    kernel, _, _, records = engine.last_plan_ex()
    assert (kernel, records) == (sa.SA_KERNEL_INT32, sa.SA_RECORDS_NONE)
    assert engine.last_timings()[1] == 0


def test_score_call_fits_where_records_do_not(engine):
    rng = np.random.default_rng(6)
    pairs = []
    for _ in range(2):
        a = seq(rng, AA, 16384)
        pairs.append((a, related(rng, AA, a, 16000)))
    args = (-1, 1, -1)
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(pairs)
    tab = degenerate_table(args)
    limit = 8 << 20
    assert sa.score_plan_query(sa.SA_SW, sc, 16384, 16000, 2, 20)[3] <= limit < sa.matrix_plan_query(sa.SA_SW, sc, 16384, 16000, 2, 20)[3]
    engine.set_workspace_limit(limit)
    try:
        for algo in (sa.SA_SW, sa.SA_NW):
            with pytest.raises(sa.SeqalibError, match="memory"):
                engine.align_matrix_packed(algo, sc, s1, o1, s2, o2, tab)
            score = engine.score_matrix_packed(algo, sc, s1, o1, s2, o2, tab)
            full = engine.score_packed(algo, sc, s1, o1, s2, o2)
            for f in FIELDS:
                assert np.array_equal(score[f], full[f]), (algo, f)
    finally:
        engine.set_workspace_limit(0)


# ---------------------------------------------------------------------- 6. Python classes
def test_python_classes(engine, tables):
    rng = np.random.default_rng(3)
    pairs = []
    for m, n in [(40, 44), (100, 91), (7, 0), (150, 150)]:
        a = seq(rng, AA, m)
        pairs.append((a.decode(), related(rng, AA, a, n).decode()))
    k = len(AA)
    matrix = sa.SubstitutionMatrix(AA.tobytes(), tables["asym"][np.ix_(AA, AA)], default=-4)
    assert matrix.score("A", "C") == int(tables["asym"][ord("A"), ord("C")]) and matrix.score("A", "B") == -4
    assert np.array_equal(matrix.table[np.ix_(AA, AA)], tables["asym"][np.ix_(AA, AA)]) and k == 20
    rows = matrix.table.tolist()
    for cls, args in [(sa.SmithWatermanSA, (-1, 1, -1)), (sa.NeedlemanWunschSA, (-2, 2, -3)),
                      (sa.LocalGotohSA, (-3, -1, 1, -1)), (sa.GlobalGotohSA, (-5, -2, 4, -3))]:
        al = cls(sa.ScoringSystem(*args), matrix=matrix)
        got = al.getAlignments(pairs)
        scores = al.getScores(pairs)
        for (a, b), g, s in zip(pairs, got, scores):
            w = model_align(cls.ALGO, gaps_of(cls.ALGO, args), rows, a.encode(), b.encode())
            want = sa.expand_ops(cls.ALGO, a, b, sa.PairResult(w["score"], w["end_i"], w["end_j"], w["start_i"],
                                                               w["start_j"], 0, w["ops"]))
            assert g.rows() == want.rows()
            assert s == w["score"]
        assert al.getAlignment(*pairs[0]).rows() == got[0].rows()
        if cls.ALGO in (sa.SA_SW, sa.SA_LOCAL_GOTOH):
            cells = al.getEndCells(pairs)
            assert cells == [tuple(model_align(cls.ALGO, gaps_of(cls.ALGO, args), rows, a.encode(), b.encode())[f]
                                   for f in ("end_i", "end_j")) for a, b in pairs]
        with pytest.raises(sa.SeqalibError):
            al.getAlignments(pairs, band=4)
        with pytest.raises(sa.SeqalibError):
            al.getScores(pairs, band=4)
    for cls in (sa.HirschbergSA, sa.MyersMillerSA):
        with pytest.raises(sa.SeqalibError):
            cls(sa.ScoringSystem(-3, -1, 1, -1), matrix=matrix)
    with pytest.raises(sa.SeqalibError):
        sa.SubstitutionMatrix("AA", [[1, 2], [3, 4]])
    with pytest.raises(sa.SeqalibError):
        sa.SubstitutionMatrix("AC", [[1, 2, 3]])
    d = sa.SubstitutionMatrix("AC", {("A", "A"): 3, ("A", "C"): -2}, default=-7)
    assert (d.score("A", "A"), d.score("A", "C"), d.score("C", "A")) == (3, -2, -7)
