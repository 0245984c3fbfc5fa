"""Banded NW / SW (sa_align_batch_banded, sa_score_batch_banded) on the GPU.

Narrow bands are checked against banded_model() below, a plain-dict restatement of the banded
semantics in include/seqalib_hip.h (only in-band cells exist; a candidate that would read a missing
neighbour is no candidate).  Whole-matrix bands are checked against sa_align_batch and the oracle.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from util import (linear_rescore, named_lut, oracle_align, oracle_batch, pack_bytes, scoring_fields)

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
INT_MIN = -(2 ** 31)
ALGS = [sa.SA_NW, sa.SA_SW]
SCORINGS = [(-1, 1, -1), (-2, 2, -3), (-1, 2)]
EDGE_LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700]
FIELDS = ("score", "end_i", "end_j", "start_i", "start_j", "nops", "flags", "reserved")


# ------------------------------------------------------------------------------- the model
def banded_model(algo, args, s1, s2, w, lut=None):
    """(score, end_i, end_j, start_i, start_j, ops) of the banded recurrence and walk."""
    g, ma, mi, _, _, allow = scoring_fields(args)
    m, n = len(s1), len(s2)
    lo, hi = min(0, n - m) - w, max(0, n - m) + w
    sw = algo == sa.SA_SW

    def match(i, j):
        return bool(lut[s1[i - 1], s2[j - 1]]) if lut is not None else s1[i - 1] == s2[j - 1]

    def diag(H, i, j):   # the diagonal neighbour is on the same diagonal: always in band
        v = match(i, j)
        return v, (H[i - 1, j - 1] + (ma if v else mi)) if (v or allow) else None

    H = {}
    best, maxr, maxc = None, 0, 0
    for i in range(m + 1):
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 or j == 0:
                H[i, j] = 0 if sw else (i + j) * g
                continue
            cands = []
            _, d = diag(H, i, j)
            if d is not None:
                cands.append(d)
            if (i - 1, j) in H:
                cands.append(H[i - 1, j] + g)
            if (i, j - 1) in H:
                cands.append(H[i, j - 1] + g)
            if sw:
                cands.append(0)
            h = H[i, j] = max(cands)
            if sw and (best is None or h >= best):
                best, maxr, maxc = h, i, j
    ops = bytearray()
    if sw:
        i, j = (maxr, maxc) if m and n else (0, 0)
        while i > 0 and j > 0:
            v, d = diag(H, i, j)
            s = max(d, 0) if d is not None else 0
            if H[i, j] == s:
                if s == 0:
                    break
                ops.append(ord(("M" if v else "S") if (v or allow) else "X"))
                i, j = i - 1, j - 1
            elif (i - 1, j) in H and H[i, j] == H[i - 1, j] + g:
                if H[i - 1, j] + g <= 0:
                    break
                ops.append(ord("U"))
                i -= 1
            else:
                assert (i, j - 1) in H
                if H[i, j - 1] + g <= 0:
                    break
                ops.append(ord("L"))
                j -= 1
        return (best if m and n else INT_MIN), maxr, maxc, i, j, bytes(ops)
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            v, d = diag(H, i, j)
            if d is not None and H[i, j] == d:
                ops.append(ord(("M" if v else "S") if (v or allow) else "X"))
                i, j = i - 1, j - 1
                continue
        if i > 0 and (i - 1, j) in H and H[i, j] == H[i - 1, j] + g:
            ops.append(ord("U"))
            i -= 1
        else:
            assert (i, j - 1) in H
            ops.append(ord("L"))
            j -= 1
    return H[m, n], m, n, 0, 0, bytes(ops)


# ---------------------------------------------------------------------------------- inputs
def seq(rng, alphabet, n):
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


def related(rng, alphabet, a, n):
    """A copy of `a` cut or padded to n symbols with a fifth of its symbols redrawn."""
    b = bytearray((a + seq(rng, alphabet, max(0, n - len(a))))[:n])
    for p in rng.integers(0, max(len(b), 1), len(b) // 5):
        b[p] = alphabet[rng.integers(0, len(alphabet))]
    return bytes(b)


def ragged_pairs(seed, alphabet, extra=34):
    """~100 pairs: every edge length in m and in n against random lengths <= 700 and against each
    other, then random related pairs."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k, L in enumerate(EDGE_LENGTHS):
        pairs.append((seq(rng, alphabet, L), seq(rng, alphabet, int(rng.integers(0, 701)))))
        pairs.append((seq(rng, alphabet, int(rng.integers(0, 701))), seq(rng, alphabet, L)))
        pairs.append((seq(rng, alphabet, L), seq(rng, alphabet, EDGE_LENGTHS[-1 - k])))
    for _ in range(extra):
        a = seq(rng, alphabet, int(rng.integers(1, 701)))
        pairs.append((a, related(rng, alphabet, a, int(rng.integers(1, len(a) + 1)))))
    return pairs


NARROW_W = [0, 1, 2, 3, 15, 16, 31, 32, 33, 63, 64, 65]


def narrow_cases():
    """{w: [(s1, s2), ...]} with lengths <= 200 (the shifted bands: <= 400)."""
    rng = np.random.default_rng(2024)
    cases = {w: [] for w in NARROW_W}

    def add(w, m, n, alphabet=ACGT):
        a = seq(rng, alphabet, m)
        cases[w].append((a, related(rng, alphabet, a, n)))

    for w in NARROW_W:
        for m, n in [(0, 0), (0, 1), (1, 0), (1, 1), (0, 7), (7, 0), (1, 9), (9, 1), (37, 37), (120, 131), (131, 120),
                     (200, 200), (199, 173)]:
            add(w, m, n)
        add(w, 90, 97, AA)
        add(w, 64, 64, AA)
    # B = |n - m| + 2 w + 1 on 63..65, 127..129, 255..257, unclipped (m >= w), both ways round
    for w, m, ds in [(15, 20, (32, 33, 34)), (31, 40, (64, 65, 66)), (63, 70, (128, 129, 130))]:
        for d in ds:
            add(w, m, m + d)
            add(w, m + d, m)
    # strongly shifted bands
    add(3, 50, 400)
    add(3, 400, 50)
    # every m + n in a window of 70 around record-packing boundaries: at w = 3 a pair has 7 diagonals,
    # so it runs one cell per lane and step with 16 steps per 32-bit record word per lane, and the word
    # count of a pair changes at every multiple of 16 steps (m + n = 65 .. 134 crosses 80, 96, 112, 128)
    for t in range(65, 135):
        add(3, t // 2, t - t // 2)
    return cases


def mixed_pairs():
    """One batch whose pairs need very different numbers of diagonals at w = 2: B = 5 .. 385."""
    rng = np.random.default_rng(77)
    pairs = []
    for d in [0, 1, 5, 20, 27, 28, 40, 59, 60, 61, 100, 123, 124, 125, 190, 251, 252, 253, 380]:
        m = int(rng.integers(5, 60))
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, m + d)))
        pairs.append((related(rng, ACGT, a, m + d), a))
    return pairs


def run_align(engine, algo, args, pairs, w, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_banded_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, w, lut)
    return res, ops, o1, o2


def pair_ops(res, ops, o1, o2, p):
    o = int(o1[p] + o2[p]) + p
    return ops[o:o + int(res["nops"][p])].tobytes()


def check_model(engine, algo, args, pairs, w, lut=None):
    res, ops, o1, o2 = run_align(engine, algo, args, pairs, w, lut)
    score = engine.score_banded_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), w, lut)
    for p, (a, b) in enumerate(pairs):
        want = banded_model(algo, args, a, b, w, lut)
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
    return {"dna": ragged_pairs(11, ACGT), "aa": ragged_pairs(12, AA)}


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("alphabet", ["dna", "aa"])
@pytest.mark.parametrize("merge", ["1", "0"])
def test_whole_matrix_band_equals_full_path(engine, monkeypatch, ragged, algo, alphabet, merge):
    """merge = 0: every pair runs the narrowest variant that holds its clipped band, so every variant
    up to 16 cells per lane is compared op for op (the default joins neighbouring variants)."""
    monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
    pairs = ragged[alphabet]
    s1, o1, s2, o2 = pack_bytes(pairs)
    for args in SCORINGS:
        sc = sa.ScoringSystem(*args)
        full, fops = engine.align_packed(algo, sc, s1, o1, s2, o2)
        band, bops = engine.align_banded_packed(algo, sc, s1, o1, s2, o2, 4096)
        ora, oops = oracle_batch(algo, args, s1, o1, s2, o2)
        for f in FIELDS:
            assert np.array_equal(full[f], band[f]), (args, f)
        for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops"):
            assert np.array_equal(ora[f], band[f].astype(np.int64)), (args, f)
        for p in range(len(pairs)):
            b = pair_ops(band, bops, o1, o2, p)
            assert b == pair_ops(full, fops, o1, o2, p), (args, p)
            assert b == pair_ops(ora, oops, o1, o2, p), (args, p)
        score = engine.score_banded_packed(algo, sc, s1, o1, s2, o2, 4096)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], band[f]), (args, f)
        assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all()
        assert (score["flags"] == 0).all() and (score["reserved"] == 0).all()


@pytest.mark.parametrize("algo", ALGS)
def test_whole_matrix_band_named_lut(engine, algo):
    pairs = ragged_pairs(13, np.frombuffer(b"ACGTN", dtype=np.uint8), extra=10)[::2]
    lut = named_lut("nwild")
    s1, o1, s2, o2 = pack_bytes(pairs)
    args = (-2, 2, -3)
    sc = sa.ScoringSystem(*args)
    full, fops = engine.align_packed(algo, sc, s1, o1, s2, o2, lut)
    band, bops = engine.align_banded_packed(algo, sc, s1, o1, s2, o2, 4096, lut)
    for f in FIELDS:
        assert np.array_equal(full[f], band[f]), f
    for p, (a, b) in enumerate(pairs):
        got = pair_ops(band, bops, o1, o2, p)
        assert got == pair_ops(full, fops, o1, o2, p), p
        o = oracle_align(algo, args, a, b, lut)
        assert (o["score"], o["end_i"], o["end_j"], o["start_i"], o["start_j"], o["ops"]) == \
            (int(band["score"][p]), int(band["end_i"][p]), int(band["end_j"][p]), int(band["start_i"][p]),
             int(band["start_j"][p]), got), p


# ------------------------------------------------------ 2. narrow bands against the model
@pytest.fixture(scope="module")
def narrow():
    return narrow_cases()


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("w", NARROW_W)
def test_narrow_band_matches_model(engine, narrow, algo, w):
    check_model(engine, algo, (-1, 1, -1) if w % 2 else (-2, 2, -3), narrow[w], w)
    assert engine.last_timings()[1] == 0   # (the score call ran last)
    kernel, _, _, records = engine.last_plan_ex()
    assert (kernel, records) == (sa.SA_KERNEL_BANDED, sa.SA_RECORDS_NONE)
    run_align(engine, algo, (-1, 1, -1), narrow[w][:3], w)
    kernel, _, _, records = engine.last_plan_ex()
    assert (kernel, records) == (sa.SA_KERNEL_BANDED, sa.SA_RECORDS_BAND2)


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("w", [1, 3, 16])
def test_narrow_band_no_mismatch(engine, narrow, algo, w):
    check_model(engine, algo, (-1, 2), narrow[w], w)


@pytest.mark.parametrize("algo", ALGS)
def test_narrow_band_named_lut(engine, narrow, algo):
    check_model(engine, algo, (-2, 2, -3), narrow[15], 15, named_lut("purine"))


@pytest.mark.parametrize("algo", ALGS)
@pytest.mark.parametrize("merge", ["0", "1"])
def test_mixed_bands_in_one_call(engine, monkeypatch, algo, merge):
    """merge = 0: every pair runs the narrowest variant that holds its band, one launch per variant;
    1 (the default): small launches are joined in the wider variant."""
    monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
    pairs = mixed_pairs()
    shapes = {sa.banded_plan_query(algo, len(a), len(b), 2)[:2] for a, b in pairs}
    assert len(shapes) >= 4, shapes   # several (cells per lane, pairs per wave) variants in one call
    check_model(engine, algo, (-1, 1, -1), pairs, 2)
    run_align(engine, algo, (-1, 1, -1), pairs, 2)
    assert engine.last_timings()[2] == expected_launches(shapes, merge == "1")


VARIANTS = [(1, 4), (2, 4), (4, 4), (4, 2), (4, 1), (8, 1), (16, 1), (32, 1)]   # (cells per lane, pairs per wave)


def expected_launches(shapes, merge):
    """Fill launches of a small call whose pairs need these variants: one per variant; with merging a
    variant joins the next one when that is in use too, and a variant that took pairs in stays."""
    used = [v in shapes for v in VARIANTS]
    took_in = False
    for v in range(len(VARIANTS) - 1):
        fixed, took_in = took_in, False
        if merge and not fixed and used[v] and used[v + 1]:
            used[v] = False
            took_in = True
    return sum(used)


@pytest.mark.parametrize("algo", ALGS)
def test_merge_respects_the_workspace_limit(engine, algo):
    """A long narrow pair beside a short wide one, and two pairs of neighbouring variants, under a
    workspace limit of exactly the largest pair's own records (sa_banded_plan_query): the narrow pair
    is not moved to the wide pair's variant, a move that would not fit is not made, and the call
    succeeds with exact results."""
    rng = np.random.default_rng(9)
    w = 8
    a = seq(rng, ACGT, 4096)
    narrow = (a, related(rng, ACGT, a, 4096))           # 17 diagonals
    b = seq(rng, ACGT, 100)
    wide = (b, related(rng, ACGT, b, 3000))             # 2917 diagonals
    c = seq(rng, ACGT, 2000)
    near = (c, related(rng, ACGT, c, 2030))             # 47 diagonals: the variant next to narrow's
    plans = {k: sa.banded_plan_query(algo, len(x), len(y), w) for k, (x, y) in
             dict(narrow=narrow, wide=wide, near=near).items()}
    assert plans["narrow"][0] == 1 and plans["near"][0] == 2 and plans["wide"][0] == 32
    assert plans["narrow"][2] * 8 < plans["wide"][2]
    try:
        for pairs, limit, launches in [([narrow, wide], plans["wide"][2], 2),
                                       ([narrow, near], max(plans["narrow"][2], plans["near"][2]), 2),
                                       ([narrow, near], 2 * plans["narrow"][2] + plans["near"][2], 1)]:
            engine.set_workspace_limit(limit)
            check_model(engine, algo, (-1, 1, -1), pairs, w)
            run_align(engine, algo, (-1, 1, -1), pairs, w)
            assert engine.last_timings()[2] == launches, (limit, launches)
    finally:
        engine.set_workspace_limit(0)


@pytest.mark.parametrize("algo", ALGS)
def test_widest_variant(engine, algo):
    """More than 2048 diagonals inside the matrix: 32 cells per lane and step."""
    rng = np.random.default_rng(41)
    pairs = []
    for m, n in [(1500, 1490), (1100, 1300), (1027, 1029)]:
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, n)))
    assert {sa.banded_plan_query(algo, len(a), len(b), 4096)[0] for a, b in pairs} == {32}
    s1, o1, s2, o2 = pack_bytes(pairs)
    for args in [(-1, 1, -1), (-1, 2)]:
        sc = sa.ScoringSystem(*args)
        full, fops = engine.align_packed(algo, sc, s1, o1, s2, o2)
        band, bops = engine.align_banded_packed(algo, sc, s1, o1, s2, o2, 4096)
        assert engine.last_plan_ex()[1] == 32
        for f in FIELDS:
            assert np.array_equal(full[f], band[f]), (args, f)
        for p in range(len(pairs)):
            assert pair_ops(band, bops, o1, o2, p) == pair_ops(full, fops, o1, o2, p), (args, p)
        score = engine.score_banded_packed(algo, sc, s1, o1, s2, o2, 4096)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], band[f]), (args, f)


def test_band_zero_needs_mismatches(engine):
    with pytest.raises(sa.SeqalibError):
        run_align(engine, sa.SA_NW, (-1, 2), [(b"ACGT", b"ACGT")], 0)


# ------------------------------------------------------------------ 3. properties at size
@pytest.fixture(scope="module")
def related4096():
    pairs = []
    for p in range(64):
        a = sa.synth_dna(5000 + p, 4096)
        pairs.append((a, sa.synth_mutate(a, 9000 + p)))
    return pairs


@pytest.mark.parametrize("algo", ALGS)
def test_properties_at_4096(engine, related4096, algo):
    # One-off CPU check (a vectorised model of the banded score, swept by anti-diagonal and indexed
    # by row, against the oracle's full scores of these 64 pairs): at w = 16, 63 of the 64 pairs
    # reach the full score, NW and SW alike (the other one falls 304 short); at w = 64 and w = 256
    # all 64 do.  So equality is asserted from w = 64 on, and at w = 16 the inequality and the
    # re-score alone.
    args = (-1, 1, -1)
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(related4096)
    full = engine.score_packed(algo, sc, s1, o1, s2, o2)
    m = np.diff(o1).astype(np.int64)
    n = np.diff(o2).astype(np.int64)
    for w in (16, 64, 256):
        res, ops = engine.align_banded_packed(algo, sc, s1, o1, s2, o2, w)
        assert (res["score"] <= full["score"]).all(), w
        assert np.array_equal(linear_rescore(args, res, ops, o1, o2), res["score"].astype(np.int64)), w
        valid = np.zeros(256, dtype=bool)
        valid[[ord(c) for c in "MSUL"]] = True
        c1 = np.zeros(256, dtype=np.int64)
        c2 = np.zeros(256, dtype=np.int64)
        c1[[ord("M"), ord("S"), ord("U")]] = 1
        c2[[ord("M"), ord("S"), ord("L")]] = 1
        for p in range(len(m)):
            o = int(o1[p] + o2[p]) + p
            x = ops[o:o + int(res["nops"][p])]
            assert valid[x].all()
            u1, u2 = int(c1[x].sum()), int(c2[x].sum())
            if algo == sa.SA_NW:
                assert (u1, u2) == (m[p], n[p]), (w, p)
            else:
                assert (u1, u2) == (res["end_i"][p] - res["start_i"][p], res["end_j"][p] - res["start_j"][p]), (w, p)
        if w >= 64:
            assert np.array_equal(res["score"], full["score"]), w


# ------------------------------------------------------------------------------ 4. memory
def test_banded_fits_where_full_records_do_not(engine):
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
    args = (-1, 1, -1)
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(pairs)
    need = sa.banded_plan_query(sa.SA_NW, 16384, max(len(b) for _, b in pairs), 256)[2]
    limit = 8 << 20
    assert need <= limit < sa.plan_query_ex(sa.SA_NW, sc, 16384, 16384, 4, 20)[3]
    engine.set_workspace_limit(limit)
    try:
        for algo in ALGS:
            with pytest.raises(sa.SeqalibError, match="memory"):
                engine.align_packed(algo, sc, s1, o1, s2, o2)
            res, ops = engine.align_banded_packed(algo, sc, s1, o1, s2, o2, 256)
            assert np.array_equal(linear_rescore(args, res, ops, o1, o2), res["score"].astype(np.int64))
            full = engine.score_packed(algo, sc, s1, o1, s2, o2)
            # (one-off CPU check with the vectorised model of test_properties_at_4096: at w = 256
            # each of these four pairs has its whole-matrix score, NW and SW)
            assert np.array_equal(res["score"], full["score"])
    finally:
        engine.set_workspace_limit(0)


# ---------------------------------------------------------------------- 6. Python classes
def test_python_classes(engine):
    rng = np.random.default_rng(3)
    pairs = []
    for m, n in [(40, 44), (100, 91), (7, 0), (150, 150)]:
        a = seq(rng, ACGT, m)
        pairs.append((a.decode(), related(rng, ACGT, a, n).decode()))
    for cls, algo in [(sa.NeedlemanWunschSA, sa.SA_NW), (sa.HirschbergSA, sa.SA_NW), (sa.SmithWatermanSA, sa.SA_SW)]:
        al = cls(sa.ScoringSystem(-1, 1, -1))
        got = al.getAlignments(pairs, band=4)
        scores = al.getScores(pairs, band=4)
        for (a, b), g, s in zip(pairs, got, scores):
            sc, ei, ej, si, sj, ops = banded_model(algo, (-1, 1, -1), a.encode(), b.encode(), 4)
            want = sa.expand_ops(algo, a, b, sa.PairResult(sc, ei, ej, si, sj, 0, ops))
            assert g.rows() == want.rows()
            assert s == sc
        assert al.getAlignment(*pairs[0], band=4).rows() == got[0].rows()
        plain = [x.rows() for x in al.getAlignments(pairs)]
        assert [x.rows() for x in al.getAlignments(pairs, band=None)] == plain
        eng = sa._engine(0)
        ref = eng.align(cls.ALGO, al.scoring, pairs)
        assert plain == [sa.expand_ops(cls.ALGO, a, b, r).rows() for (a, b), r in zip(pairs, ref)]
    sw = sa.SmithWatermanSA(sa.ScoringSystem(-1, 1, -1))
    cells = sw.getEndCells(pairs, band=4)
    assert cells == [banded_model(sa.SA_SW, (-1, 1, -1), a.encode(), b.encode(), 4)[1:3] for a, b in pairs]
    for cls in (sa.GlobalGotohSA, sa.LocalGotohSA, sa.MyersMillerSA):
        with pytest.raises(sa.SeqalibError):
            cls(sa.ScoringSystem(-3, -1, 1, -1)).getScores(pairs, band=4)
        with pytest.raises(sa.SeqalibError):
            cls(sa.ScoringSystem(-3, -1, 1, -1)).getAlignments(pairs, band=4)
