"""Ends-free banded NW / GlobalGotoh (sa_align_batch_banded_ends_free, sa_score_batch_banded_ends_free)
on the GPU.

free_ends = 0 is compared bit for bit with the banded global calls; every flag set is compared with
tests/ends_free_model.py, a plain-dict restatement of the header's contract that
tests/test_ends_free_model.py pins on the CPU.  The input builders are those of test_gpu_banded.py.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from banded_affine_model import affine_rescore
from ends_free_model import ends_free_model
from test_gpu_banded import ACGT, FIELDS, mixed_pairs, pair_ops, ragged_pairs, related, seq
from util import linear_rescore, named_lut, pack_bytes, scoring_fields

pytestmark = pytest.mark.gpu

NW, HB, GG = sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH
# the last of each list lies outside gap < 0 < match
SCORINGS = {NW: [(-1, 1, -1), (-1, 2), (1, -1, -2)],
            GG: [(-3, -1, 1, -1), (-3, -1, 2, -1, False), (2, -1, -1, -2)]}
FIT = sa.SA_FREE_SEQ2_BEGIN | sa.SA_FREE_SEQ2_END
OVERLAP = sa.SA_FREE_SEQ1_BEGIN | sa.SA_FREE_SEQ2_END
PURINE = named_lut("purine")
EDGES = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]


def run_align(engine, algo, args, pairs, w, fe, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_banded_ends_free_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, w, fe, lut)
    return res, ops, o1, o2


def run_score(engine, algo, args, pairs, w, fe, lut=None):
    return engine.score_banded_ends_free_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), w, fe, lut)


_MODEL = {}


def model(algo, args, a, b, w, fe, lut=None):
    """ends_free_model, computed once per input (several tests share pairs)."""
    if lut is not None:
        return ends_free_model(algo, args, a, b, w, fe, lut)
    key = (algo, args, a, b, w, fe)
    if key not in _MODEL:
        _MODEL[key] = ends_free_model(algo, args, a, b, w, fe)
    return _MODEL[key]


def check_model(engine, algo, args, pairs, w, fe, lut=None):
    """Align and score call against the model: every field and op exact, the score contract kept."""
    res, ops, o1, o2 = run_align(engine, algo, args, pairs, w, fe, lut)
    score = run_score(engine, algo, args, pairs, w, fe, lut)
    for p, (a, b) in enumerate(pairs):
        want = model(algo, args, a, b, w, fe, lut)
        r = res[p]
        got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
               pair_ops(res, ops, o1, o2, p))
        assert got == want, (algo, args, w, fe, p, len(a), len(b))
        assert int(r["flags"]) == 0 and int(r["reserved"]) == 0
        s = score[p]
        assert (int(s["score"]), int(s["end_i"]), int(s["end_j"])) == want[:3], (algo, args, w, fe, p, len(a), len(b))
        assert (int(s["start_i"]), int(s["start_j"]), int(s["nops"]), int(s["flags"]), int(s["reserved"])) == (-1, -1, 0, 0, 0)
    return res, ops


# ------------------------------------------- 1. free_ends = 0 is the banded global call, bit for bit
@pytest.fixture(scope="module")
def ragged():
    pairs = ragged_pairs(21, ACGT)
    lengths = {len(a) for a, _ in pairs} | {len(b) for _, b in pairs}
    assert set(EDGES) <= lengths and 80 <= len(pairs) <= 120
    return pairs


@pytest.mark.parametrize("algo", [NW, HB, GG])
@pytest.mark.parametrize("lut", [None, "purine"])
def test_no_free_end_is_the_banded_global_call(engine, ragged, algo, lut):
    s1, o1, s2, o2 = pack_bytes(ragged)
    table = PURINE if lut else None
    base = engine.align_banded_affine_packed if algo == GG else engine.align_banded_packed
    for args in SCORINGS[GG if algo == GG else NW]:
        sc = sa.ScoringSystem(*args)
        for w in (4096, 9):   # the whole matrix (at most 1401 diagonals), and a band that clips most pairs
            want, wops = base(algo, sc, s1, o1, s2, o2, w, table)
            got, gops = engine.align_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, w, 0, table)
            for f in FIELDS:
                assert np.array_equal(want[f], got[f]), (args, w, f)
            for p in range(len(ragged)):
                assert pair_ops(got, gops, o1, o2, p) == pair_ops(want, wops, o1, o2, p), (args, w, p)
            score = engine.score_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, w, 0, table)
            for f in ("score", "end_i", "end_j"):
                assert np.array_equal(score[f], want[f]), (args, w, f)


# ------------------------------------------------------- 2. every flag set against the model
@pytest.fixture(scope="module")
def small():
    """Pairs <= 300 long: empty and one-symbol sequences, |n - m| above and below every w used."""
    rng = np.random.default_rng(31)
    pairs = []
    for m, n in [(0, 0), (0, 5), (5, 0), (1, 1), (1, 30), (30, 1), (1, 0), (37, 37), (40, 90), (90, 40), (64, 65),
                 (129, 120), (300, 290), (60, 300), (33, 31)]:
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, n)))
    # a read inside a window, and two overlapping reads
    win = seq(rng, ACGT, 120)
    pairs.append((win[50:90], win))
    pairs.append((win, win[70:] + seq(rng, ACGT, 30)))
    return pairs


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("fe", range(16))
def test_every_flag_set_matches_the_model(engine, small, algo, fe):
    for k, w in enumerate((0, 1, 5, 40)):
        args = SCORINGS[algo][(fe + k) % 3]
        if w == 0 and not scoring_fields(args)[5]:
            args = SCORINGS[algo][0]   # one diagonal needs allow_mismatch
        check_model(engine, algo, args, small, w, fe, PURINE if (fe + k) % 5 == 0 else None)


def test_hirschberg_means_nw(engine, small):
    for fe in (0, FIT, 15):
        a, aops = run_align(engine, HB, (-1, 1, -1), small, 5, fe)[:2]
        b, bops = run_align(engine, NW, (-1, 1, -1), small, 5, fe)[:2]
        assert a.tobytes() == b.tobytes() and aops.tobytes() == bops.tobytes()


# one pair per fill variant: the clipped band has just more diagonals than the variant below holds
VARIANT_PAIRS = [(33, 2, 40, 56, 8), (65, 4, 50, 70, 22), (129, 4, 70, 100, 49), (257, 4, 130, 170, 108),
                 (513, 8, 260, 300, 236)]   # (diagonals, cells per lane, m, n, w)


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("diagonals,cells,m,n,w", VARIANT_PAIRS)
def test_every_variant_matches_the_model(engine, algo, diagonals, cells, m, n, w):
    assert abs(n - m) + 2 * w + 1 == diagonals and w <= min(m, n)   # none clipped
    query = sa.banded_affine_plan_query if algo == GG else sa.banded_plan_query
    assert query(algo, m, n, w)[0] == cells
    rng = np.random.default_rng(diagonals)
    a = seq(rng, ACGT, m)
    pairs = [(a, related(rng, ACGT, a, n))]
    if diagonals <= 129:   # (the model's time: the wider pairs run one way round and three flag sets)
        pairs.append((related(rng, ACGT, a, n), a))
    for fe in range(16) if diagonals <= 129 else (15, 6, 9):
        check_model(engine, algo, SCORINGS[algo][0], pairs, w, fe)
        assert engine.last_plan_ex()[1] == cells


@pytest.mark.parametrize("algo,cells,m,n,w", [(NW, 16, 200, 1100, 100), (GG, 16, 200, 1100, 100), (NW, 32, 300, 2100, 150)])
def test_widest_variants_match_the_model(engine, algo, cells, m, n, w):
    """A read in a long window: 1101 and (linear only) 2101 diagonals, 16 and 32 cells per lane and step."""
    rng = np.random.default_rng(n)
    window = seq(rng, ACGT, n)
    pairs = [(related(rng, ACGT, window[n // 3:n // 3 + m], m), window)]
    query = sa.banded_affine_plan_query if algo == GG else sa.banded_plan_query
    assert query(algo, m, n, w)[0] == cells
    check_model(engine, algo, SCORINGS[algo][0], pairs, w, 15)
    assert engine.last_plan_ex()[1] == cells


def rescore(algo, args, res, ops, o1, o2):
    if algo == NW:
        return linear_rescore(args, res, ops, o1, o2)
    return np.array([affine_rescore(args, pair_ops(res, ops, o1, o2, p)) for p in range(len(res))], dtype=np.int64)


@pytest.fixture(scope="module")
def related3000():
    pairs = []
    for p in range(8):
        a = sa.synth_dna(7000 + p, 3000)
        pairs.append((a, sa.synth_mutate(a, 7100 + p)))
    return pairs


@pytest.mark.parametrize("algo,w", [(NW, 16), (NW, 600), (NW, 1100), (GG, 16), (GG, 600)])
def test_properties_at_3000(engine, related3000, algo, w):
    """Pairs long enough for steps without border cells at every width up to 32 cells per lane and step
    (beyond what the model computes in a test's time): free_ends = 0 is the banded call bit for bit; with
    free ends the ops add up to the score and to (end - start), and freeing ends never lowers the score."""
    args = SCORINGS[algo][0]
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(related3000)
    base = engine.align_banded_affine_packed if algo == GG else engine.align_banded_packed
    want, wops = base(algo, sc, s1, o1, s2, o2, w)
    got, gops = engine.align_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, w, 0)
    assert want.tobytes() == got.tobytes() and wops.tobytes() == gops.tobytes()
    m, n = np.diff(o1).astype(np.int64), np.diff(o2).astype(np.int64)
    for fe in (15, FIT, sa.SA_FREE_SEQ1_END):
        res, ops = engine.align_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, w, fe)
        assert (res["score"] >= want["score"]).all(), fe
        assert np.array_equal(rescore(algo, args, res, ops, o1, o2), res["score"].astype(np.int64)), fe
        for p in range(len(m)):
            x = pair_ops(res, ops, o1, o2, p)
            assert sum(c in b"MSU" for c in x) == res["end_i"][p] - res["start_i"][p], (fe, p)
            assert sum(c in b"MSL" for c in x) == res["end_j"][p] - res["start_j"][p], (fe, p)
        assert ((res["end_i"] == m) | (res["end_j"] == n)).all() and ((res["start_i"] == 0) | (res["start_j"] == 0)).all()
        score = engine.score_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, w, fe)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], res[f]), (fe, f)


# --------------------------------------------------------------------- 3. planted alignments
def edited(rng, s):
    """s with one substitution, one insertion and one deletion, away from its ends."""
    b = bytearray(s)
    k = len(b) // 4
    b[k] = ACGT[(list(ACGT).index(b[k]) + 1) % 4]
    b.insert(2 * k, int(ACGT[rng.integers(0, 4)]))
    del b[3 * k]
    return bytes(b)


@pytest.mark.parametrize("algo,args", [(NW, (-2, 2, -3)), (GG, (-3, -1, 2, -3))])
def test_planted_fit(engine, algo, args):
    """A 100-symbol read with three edits inside a 400-symbol window, at several offsets: the fit finds
    the planted interval within the edit count and beats the global alignment of the pair."""
    rng = np.random.default_rng(17)
    pairs, offsets = [], []
    for off in (0, 3, 150, 297, 300):
        window = seq(rng, ACGT, 400)
        pairs.append((edited(rng, window[off:off + 100]), window))
        offsets.append(off)
    base = engine.align_banded_affine_packed if algo == GG else engine.align_banded_packed
    glob = base(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), 8)[0]
    res, _ = check_model(engine, algo, args, pairs, 8, FIT)
    for p, off in enumerate(offsets):
        r = res[p]
        assert (int(r["start_i"]), int(r["end_i"])) == (0, len(pairs[p][0]))
        assert abs(int(r["start_j"]) - off) <= 3 and abs(int(r["end_j"]) - (off + 100)) <= 3, (p, r)
        assert int(r["score"]) > int(glob["score"][p])


@pytest.mark.parametrize("algo,args", [(NW, (-2, 2, -3)), (GG, (-3, -1, 2, -3))])
def test_planted_overlap(engine, algo, args):
    """The last 140 symbols of Seq1 are, with three edits, the first symbols of Seq2, which goes on for 30
    more: w = 40 holds the start diagonal with 10 to spare."""
    rng = np.random.default_rng(18)
    pairs = []
    for _ in range(4):
        s1 = seq(rng, ACGT, 400)
        pairs.append((s1, edited(rng, s1[260:]) + seq(rng, ACGT, 30)))
    base = engine.align_banded_affine_packed if algo == GG else engine.align_banded_packed
    glob = base(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), 40)[0]
    res, _ = check_model(engine, algo, args, pairs, 40, OVERLAP)
    for p, (a, b) in enumerate(pairs):
        r = res[p]
        assert (int(r["start_j"]), int(r["end_i"])) == (0, 400)
        assert abs(int(r["start_i"]) - 260) <= 3 and abs(int(r["end_j"]) - (len(b) - 30)) <= 3, (p, r)
        assert int(r["score"]) > int(glob["score"][p])


# ------------------------------------------------------------- 4. reporting, launches, merging
@pytest.mark.parametrize("algo,records", [(NW, sa.SA_RECORDS_BAND2), (GG, sa.SA_RECORDS_BAND4)])
def test_plan_and_timings(engine, small, algo, records):
    run_align(engine, algo, SCORINGS[algo][0], small, 5, FIT)
    kernel, _, waves, rec = engine.last_plan_ex()
    assert (kernel, waves, rec) == (sa.SA_KERNEL_BANDED, 1, records)
    run_score(engine, algo, SCORINGS[algo][0], small, 5, FIT)
    kernel, _, waves, rec = engine.last_plan_ex()
    assert (kernel, waves, rec) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_NONE)
    assert engine.last_timings()[1] == 0


@pytest.mark.parametrize("algo", [NW, GG])
def test_workspace_limit_splits_the_launch(engine, algo):
    rng = np.random.default_rng(51)
    pairs = []
    for k in range(12):
        read = seq(rng, ACGT, 150)
        pairs.append((read, seq(rng, ACGT, 20 * k) + related(rng, ACGT, read, 150) + seq(rng, ACGT, 300 - 20 * k)))
    query = sa.banded_affine_plan_query if algo == GG else sa.banded_plan_query
    plans = {query(algo, len(a), len(b), 6) for a, b in pairs}
    assert len(plans) == 1   # one variant, equal records
    want, wops = check_model(engine, algo, SCORINGS[algo][0], pairs, 6, FIT)
    launches = engine.last_timings()[2]
    try:
        engine.set_workspace_limit(3 * plans.pop()[2])
        got, gops = check_model(engine, algo, SCORINGS[algo][0], pairs, 6, FIT)
        run_align(engine, algo, SCORINGS[algo][0], pairs, 6, FIT)
        assert engine.last_timings()[2] == 4 > launches
    finally:
        engine.set_workspace_limit(0)
    assert want.tobytes() == got.tobytes() and wops.tobytes() == gops.tobytes()


@pytest.mark.parametrize("algo", [NW, GG])
def test_mixed_variants_in_one_call(engine, monkeypatch, algo):
    pairs = mixed_pairs()
    query = sa.banded_affine_plan_query if algo == GG else sa.banded_plan_query
    assert len({query(algo, len(a), len(b), 2)[:2] for a, b in pairs}) >= 4
    out = {}
    for merge in ("0", "1"):
        monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
        res, ops = check_model(engine, algo, SCORINGS[algo][0], pairs, 2, 15)
        run_align(engine, algo, SCORINGS[algo][0], pairs, 2, 15)
        out[merge] = (res.tobytes(), ops.tobytes(), engine.last_timings()[2])
    assert out["0"][:2] == out["1"][:2] and out["1"][2] < out["0"][2]


# ---------------------------------------------------------------------- 5. Python classes
def test_python_classes(engine):
    rng = np.random.default_rng(3)
    win = seq(rng, ACGT, 90)
    pairs = [(win[30:60].decode(), win.decode()), (win.decode(), (win[50:] + seq(rng, ACGT, 6)).decode()), ("ACGT", ""),
             ("", "AC")]
    for cls, algo, args in [(sa.NeedlemanWunschSA, NW, (-2, 2, -3)), (sa.HirschbergSA, HB, (-2, 2, -3)),
                            (sa.GlobalGotohSA, GG, (-3, -1, 2, -3))]:
        al = cls(sa.ScoringSystem(*args))
        for fe in (FIT, OVERLAP, 0, 15):
            got = al.getEndsFreeAlignments(pairs, 8, fe)
            models = [ends_free_model(algo, args, a.encode(), b.encode(), 8, fe) for a, b in pairs]
            assert al.getScore() == models[-1][0]
            for (a, b), g, (sc, ei, ej, si, sj, ops) in zip(pairs, got, models):
                want = sa.expand_ops(sa.SA_SW, a, b, sa.PairResult(sc, ei, ej, si, sj, 0, ops))   # forceGlobal over (start, end)
                assert g.rows() == want.rows()
                assert len(g.rows()[0].replace("-", "")) == len(a) and len(g.rows()[2].replace("-", "")) == len(b)
            assert al.getEndsFreeScores(pairs, 8, fe) == [x[0] for x in models]
            assert al.getEndsFreeEndCells(pairs, 8, fe) == [x[1:3] for x in models]
            assert al.getEndsFreeAlignment(*pairs[0], 8, fe).rows() == got[0].rows()
