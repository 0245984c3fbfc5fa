"""Banded LocalGotoh / GlobalGotoh (sa_align_batch_banded_affine, sa_score_batch_banded_affine) on
the GPU.

Narrow bands are checked against tests/banded_affine_model.py, a plain-dict restatement of the banded
affine semantics of include/seqalib_hip.h.  Whole-matrix bands are checked against sa_align_batch and
the oracle; none of their pairs has a size the reference's LocalGotoh size hack fires on, because the
banded calls are the raw path.  The input builders are those of test_gpu_banded.py.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from banded_affine_model import affine_rescore, banded_affine_model
from test_gpu_banded import (AA, ACGT, FIELDS, NARROW_W, mixed_pairs, narrow_cases, pair_ops, ragged_pairs, related, seq)
from util import LG_HACK_SIZES, named_lut, oracle_batch, pack_bytes

pytestmark = pytest.mark.gpu

ALGS = [sa.SA_GLOBAL_GOTOH, sa.SA_LOCAL_GOTOH]
SCORINGS = [(-3, -1, 1, -1), (-2, -2, 2, -3), (-3, -1, 2, -1, False)]
# (cells per lane, pairs per wave) of the affine fills: three values per cell fit one wave's registers
# up to 16 cells per lane and step, i.e. 2048 diagonals inside the matrix
VARIANTS = [(1, 4), (2, 4), (4, 4), (4, 2), (4, 1), (8, 1), (16, 1)]
MAX_DIAGONALS = 2048


def run_align(engine, algo, args, pairs, w, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_banded_affine_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, w, lut)
    return res, ops, o1, o2


_MODEL = {}


def model(algo, args, a, b, w, lut=None):
    """banded_affine_model, computed once per input (several tests share pairs)."""
    if lut is not None:
        return banded_affine_model(algo, args, a, b, w, lut)
    key = (algo, args, a, b, w)
    if key not in _MODEL:
        _MODEL[key] = banded_affine_model(algo, args, a, b, w)
    return _MODEL[key]


def check_model(engine, algo, args, pairs, w, lut=None):
    res, ops, o1, o2 = run_align(engine, algo, args, pairs, w, lut)
    score = engine.score_banded_affine_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), w, lut)
    for p, (a, b) in enumerate(pairs):
        want = model(algo, args, a, b, w, lut)
        r = res[p]
        got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
               pair_ops(res, ops, o1, o2, p))
        assert got == want, (algo, args, w, p, len(a), len(b))
        assert int(r["flags"]) == 0 and int(r["reserved"]) == 0
        s = score[p]
        assert (int(s["score"]), int(s["end_i"]), int(s["end_j"])) == want[:3], (algo, args, w, p, len(a), len(b))
        assert (int(s["start_i"]), int(s["start_j"]), int(s["nops"]), int(s["flags"]), int(s["reserved"])) == (-1, -1, 0, 0, 0)


# --------------------------------------------------------- 1. whole-matrix band = the full path
@pytest.fixture(scope="module")
def ragged():
    # EDGE_LENGTHS stops at 700, so the clipped whole-matrix band has at most 1401 diagonals: inside
    # the 2048 the affine fills hold, and no length had to be capped
    out = {}
    for name, seed, alphabet in [("dna", 11, ACGT), ("aa", 12, AA)]:
        pairs = [(a, b) for a, b in ragged_pairs(seed, alphabet) if (len(a), len(b)) not in LG_HACK_SIZES]
        assert len(pairs) >= 80 and not any((len(a), len(b)) in LG_HACK_SIZES for a, b in pairs)
        assert max(len(a) + len(b) + 1 for a, b in pairs) <= MAX_DIAGONALS
        out[name] = pairs
    return out


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("alphabet", ["dna", "aa"])
@pytest.mark.parametrize("merge", ["1", "0"])
def test_whole_matrix_band_equals_full_path(engine, monkeypatch, ragged, algo, alphabet, merge):
    monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
    pairs = ragged[alphabet]
    s1, o1, s2, o2 = pack_bytes(pairs)
    for args in SCORINGS:
        sc = sa.ScoringSystem(*args)
        full, fops = engine.align_packed(algo, sc, s1, o1, s2, o2)
        band, bops = engine.align_banded_affine_packed(algo, sc, s1, o1, s2, o2, 4096)
        ora, oops = oracle_batch(algo, args, s1, o1, s2, o2)
        for f in FIELDS:
            assert np.array_equal(full[f], band[f]), (args, f)
        for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops"):
            assert np.array_equal(ora[f], band[f].astype(np.int64)), (args, f)
        for p in range(len(pairs)):
            b = pair_ops(band, bops, o1, o2, p)
            assert b == pair_ops(full, fops, o1, o2, p), (args, p)
            assert b == pair_ops(ora, oops, o1, o2, p), (args, p)
        score = engine.score_banded_affine_packed(algo, sc, s1, o1, s2, o2, 4096)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], band[f]), (args, f)
        assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all()
        assert (score["flags"] == 0).all() and (score["reserved"] == 0).all()


# ------------------------------------------------------ 2. narrow bands against the model
@pytest.fixture(scope="module")
def narrow():
    # narrow_cases() holds, at w = 3, every m + n from 65 to 134.  Such a pair has 7 diagonals, so it
    # runs one cell per lane and step with 8 steps per 32-bit word of 4-bit records, and m + n + 2
    # steps are kept: the word count grows at m + n = 71, 79, ..., 127 -- all inside the sweep.
    return narrow_cases()


def test_rescore_helper_agrees_with_the_model(narrow):
    for w in (1, 3, 16, 64):
        for algo in ALGS:
            for a, b in narrow[w]:
                want = model(algo, (-3, -1, 1, -1), a, b, w)
                assert affine_rescore((-3, -1, 1, -1), want[5]) == want[0], (algo, w, len(a), len(b))


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("w", NARROW_W)
def test_narrow_band_matches_model(engine, narrow, algo, w):
    check_model(engine, algo, (-3, -1, 1, -1) if w % 2 else (-2, -2, 2, -3), narrow[w], w)
    assert engine.last_timings()[1] == 0   # (the score call ran last)
    kernel, _, waves, records = engine.last_plan_ex()
    assert (kernel, waves, records) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_NONE)
    run_align(engine, algo, (-3, -1, 1, -1), narrow[w][:3], w)
    kernel, _, waves, records = engine.last_plan_ex()
    assert (kernel, waves, records) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_BAND4)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("w", [1, 3, 16])
def test_narrow_band_no_mismatch(engine, narrow, algo, w):
    check_model(engine, algo, (-3, -1, 2, -1, False), narrow[w], w)


@pytest.mark.parametrize("algo", ALGS)
def test_narrow_band_named_lut(engine, narrow, algo):
    check_model(engine, algo, (-2, -2, 2, -3), narrow[15], 15, named_lut("purine"))


# ------------------------------------------------------------ 3. mixed variants in one call
def expected_launches(shapes, merge):
    """As test_gpu_banded.expected_launches, over the affine variant list."""
    used = [v in shapes for v in VARIANTS]
    took_in = False
    for v in range(len(VARIANTS) - 1):
        fixed, took_in = took_in, False
        if merge and not fixed and used[v] and used[v + 1]:
            used[v] = False
            took_in = True
    return sum(used)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("merge", ["0", "1"])
def test_mixed_bands_in_one_call(engine, monkeypatch, algo, merge):
    monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
    pairs = mixed_pairs()
    shapes = {sa.banded_affine_plan_query(algo, len(a), len(b), 2)[:2] for a, b in pairs}
    assert len(shapes) >= 4, shapes
    check_model(engine, algo, (-3, -1, 1, -1), pairs, 2)
    run_align(engine, algo, (-3, -1, 1, -1), pairs, 2)
    assert engine.last_timings()[2] == expected_launches(shapes, merge == "1")


# ------------------------------------------------------------------- 4. workspace limit
@pytest.mark.parametrize("algo", ALGS)
def test_merge_respects_the_workspace_limit(engine, algo):
    """A long narrow pair beside a short wide one, and two pairs of neighbouring variants, under a
    workspace limit of exactly the largest pair's own records (sa_banded_affine_plan_query)."""
    rng = np.random.default_rng(9)
    w = 8
    a = seq(rng, ACGT, 4096)
    narrow = (a, related(rng, ACGT, a, 4096))           # 17 diagonals
    b = seq(rng, ACGT, 100)
    wide = (b, related(rng, ACGT, b, 2000))             # 1917 diagonals
    c = seq(rng, ACGT, 2000)
    near = (c, related(rng, ACGT, c, 2030))             # 47 diagonals: the variant next to narrow's
    plans = {k: sa.banded_affine_plan_query(algo, len(x), len(y), w) for k, (x, y) in
             dict(narrow=narrow, wide=wide, near=near).items()}
    assert plans["narrow"][0] == 1 and plans["near"][0] == 2 and plans["wide"][0] == 16
    assert plans["narrow"][2] * 4 < plans["wide"][2]
    try:
        for pairs, limit, launches in [([narrow, wide], plans["wide"][2], 2),
                                       ([narrow, near], max(plans["narrow"][2], plans["near"][2]), 2),
                                       ([narrow, near], 2 * plans["narrow"][2] + plans["near"][2], 1)]:
            engine.set_workspace_limit(limit)
            check_model(engine, algo, (-3, -1, 1, -1), pairs, w)
            run_align(engine, algo, (-3, -1, 1, -1), pairs, w)
            assert engine.last_timings()[2] == launches, (limit, launches)
    finally:
        engine.set_workspace_limit(0)


# --------------------------------------------------------------------- 5. widest variant
@pytest.mark.parametrize("algo", ALGS)
def test_widest_variant(engine, algo):
    """More than 1024 diagonals inside the matrix: 16 cells per lane and step, the widest affine fill."""
    rng = np.random.default_rng(41)
    pairs = []
    for m, n in [(1020, 1010), (520, 600), (513, 515)]:
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, n)))
    assert {sa.banded_affine_plan_query(algo, len(a), len(b), 4096)[0] for a, b in pairs} == {16}
    with pytest.raises(sa.SeqalibError):
        sa.banded_affine_plan_query(algo, 1024, 1024, 4096)   # 2049 diagonals
    s1, o1, s2, o2 = pack_bytes(pairs)
    for args in [(-3, -1, 1, -1), (-3, -1, 2, -1, False)]:
        sc = sa.ScoringSystem(*args)
        full, fops = engine.align_packed(algo, sc, s1, o1, s2, o2)
        band, bops = engine.align_banded_affine_packed(algo, sc, s1, o1, s2, o2, 4096)
        assert engine.last_plan_ex()[1] == 16
        for f in FIELDS:
            assert np.array_equal(full[f], band[f]), (args, f)
        for p in range(len(pairs)):
            assert pair_ops(band, bops, o1, o2, p) == pair_ops(full, fops, o1, o2, p), (args, p)
        score = engine.score_banded_affine_packed(algo, sc, s1, o1, s2, o2, 4096)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], band[f]), (args, f)


def test_argument_checks_on_the_engine(engine):
    for algo in ALGS:
        with pytest.raises(sa.SeqalibError):
            run_align(engine, algo, (-3, -1, 2, -1, False), [(b"ACGT", b"ACGT")], 0)
        with pytest.raises(sa.SeqalibError):
            run_align(engine, algo, (-3, 1, 1, -1), [(b"ACGT", b"ACGT")], 2)
    with pytest.raises(sa.SeqalibError):
        run_align(engine, sa.SA_NW, (-3, -1, 1, -1), [(b"ACGT", b"ACGT")], 2)


# ------------------------------------------------------------------ 6. properties at size
@pytest.fixture(scope="module")
def related4096():
    pairs = []
    for p in range(64):
        a = sa.synth_dna(5000 + p, 4096)
        pairs.append((a, sa.synth_mutate(a, 9000 + p)))
    return pairs


@pytest.mark.parametrize("algo", ALGS)
def test_properties_at_4096(engine, related4096, algo):
    # Whether these pairs reach their whole-matrix affine score at some w has not been established on
    # the CPU, so no equality with the full score is asserted: the inequality, the op accounting and
    # the exact re-score are.
    args = (-3, -1, 1, -1)
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(related4096)
    full = engine.score_packed(algo, sc, s1, o1, s2, o2)
    m = np.diff(o1).astype(np.int64)
    n = np.diff(o2).astype(np.int64)
    for w in (16, 64, 256):
        assert 2 * w + 1 + int(np.abs(n - m).max()) <= MAX_DIAGONALS
        res, ops = engine.align_banded_affine_packed(algo, sc, s1, o1, s2, o2, w)
        assert (res["score"] <= full["score"]).all(), w
        for p in range(len(m)):
            x = pair_ops(res, ops, o1, o2, p)
            assert set(x) <= set(b"MSUL"), (w, p)
            u1 = sum(c in b"MSU" for c in x)
            u2 = sum(c in b"MSL" for c in x)
            if algo == sa.SA_GLOBAL_GOTOH:
                assert (u1, u2) == (m[p], n[p]), (w, p)
            else:
                assert (u1, u2) == (res["end_i"][p] - res["start_i"][p], res["end_j"][p] - res["start_j"][p]), (w, p)
            assert affine_rescore(args, x) == int(res["score"][p]), (w, p)


# ------------------------------------------------------------------------------ 7. memory
def test_banded_affine_fits_where_full_records_do_not(engine):
    rng = np.random.default_rng(5)
    pairs = []
    for p in range(4):
        a = seq(rng, AA, 16384)
        b = bytearray()
        for c in a:   # the mutation model of sa_synth_mutate over 20 letters
            r = int(rng.integers(0, 100))
            if r < 10:
                b.append(AA[rng.integers(0, 20)])
            elif r < 12:
                b.append(AA[rng.integers(0, 20)])
                b.append(c)
            elif r >= 14:
                b.append(c)
        pairs.append((a, bytes(b)))
    args = (-3, -1, 1, -1)
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(pairs)
    w = 256
    assert max(abs(len(a) - len(b)) for a, b in pairs) + 2 * w + 1 <= MAX_DIAGONALS
    need = max(sa.banded_affine_plan_query(sa.SA_GLOBAL_GOTOH, len(a), len(b), w)[2] for a, b in pairs)
    limit = 16 << 20
    assert need <= limit < sa.plan_query_ex(sa.SA_GLOBAL_GOTOH, sc, 16384, 16384, 4, 20)[3]
    engine.set_workspace_limit(limit)
    try:
        for algo in ALGS:
            with pytest.raises(sa.SeqalibError, match="memory"):
                engine.align_packed(algo, sc, s1, o1, s2, o2)
            res, ops = engine.align_banded_affine_packed(algo, sc, s1, o1, s2, o2, w)
            for p in range(len(pairs)):
                assert affine_rescore(args, pair_ops(res, ops, o1, o2, p)) == int(res["score"][p]), (algo, p)
    finally:
        engine.set_workspace_limit(0)


# ---------------------------------------------------------------------- 8. Python classes
def test_python_classes(engine):
    rng = np.random.default_rng(3)
    pairs = []
    for m, n in [(40, 44), (100, 91), (7, 0), (150, 150)]:
        a = seq(rng, ACGT, m)
        pairs.append((a.decode(), related(rng, ACGT, a, n).decode()))
    args = (-3, -1, 1, -1)
    for cls, algo in [(sa.GlobalGotohSA, sa.SA_GLOBAL_GOTOH), (sa.LocalGotohSA, sa.SA_LOCAL_GOTOH)]:
        al = cls(sa.ScoringSystem(*args))
        got = al.getBandedAlignments(pairs, 4)
        scores = al.getBandedScores(pairs, 4)
        models = [banded_affine_model(algo, args, a.encode(), b.encode(), 4) for a, b in pairs]
        for (a, b), g, s, (sc, ei, ej, si, sj, ops) in zip(pairs, got, scores, models):
            want = sa.expand_ops(algo, a, b, sa.PairResult(sc, ei, ej, si, sj, 0, ops))
            assert g.rows() == want.rows()
            assert s == sc
        assert al.getBandedAlignment(*pairs[0], 4).rows() == got[0].rows()
        if algo == sa.SA_LOCAL_GOTOH:
            assert al.getBandedEndCells(pairs, 4) == [x[1:3] for x in models]
        else:
            assert not hasattr(al, "getBandedEndCells")
        with pytest.raises(sa.SeqalibError):    # the old doors keep answering as they did
            al.getScores(pairs, band=4)
        with pytest.raises(sa.SeqalibError):
            al.getAlignments(pairs, band=4)
        withm = cls(sa.ScoringSystem(*args), matrix=np.zeros((256, 256), dtype=np.int16))
        with pytest.raises(sa.SeqalibError):
            withm.getBandedAlignments(pairs, 4)
        with pytest.raises(sa.SeqalibError):
            withm.getBandedScores(pairs, 4)
    for cls in (sa.NeedlemanWunschSA, sa.SmithWatermanSA, sa.MyersMillerSA):
        assert not hasattr(cls, "getBandedAlignments")
