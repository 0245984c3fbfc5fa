"""Seeded ends-free banded NW / GlobalGotoh (sa_align_batch_banded_seeded, sa_score_batch_banded_seeded)
on the GPU.

Every flag set and every geometry class is compared with tests/seeded_model.py, a plain-dict restatement
of the header's contract that tests/test_seeded_model.py pins on the CPU; the interior steps of the wide
variants are compared with the ends-free call through the header's equivalence (b).  The input builders
are those of test_gpu_banded.py and test_gpu_ends_free.py.
"""
import numpy as np
import pytest

import seqalib_amd as sa
from seeded_model import seeded_band, seeded_legal, seeded_model
from test_gpu_banded import ACGT, FIELDS, pair_ops, related, seq
from test_gpu_ends_free import edited, rescore
from util import named_lut, pack_bytes, scoring_fields

pytestmark = pytest.mark.gpu

NW, HB, GG = sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH
# the last of each list lies outside gap < 0 < match
SCORINGS = {NW: [(-1, 1, -1), (-1, 2), (1, -1, -2)],
            GG: [(-3, -1, 1, -1), (-3, -1, 2, -1, False), (2, -1, -1, -2)]}
FIT = sa.SA_FREE_SEQ2_BEGIN | sa.SA_FREE_SEQ2_END
OVERLAP = sa.SA_FREE_SEQ1_BEGIN | sa.SA_FREE_SEQ2_END
PURINE = named_lut("purine")
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals


def cells_per_lane(diagonals):
    return next(R for R, L in VARIANTS if diagonals <= 2 * R * L)


def run_align(engine, algo, args, pairs, diags, w, fe, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_banded_seeded_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, diags, w, fe, lut)
    return res, ops, o1, o2


def run_score(engine, algo, args, pairs, diags, w, fe, lut=None):
    return engine.score_banded_seeded_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), diags, w, fe, lut)


def check_model(engine, algo, args, pairs, diags, w, fe, lut=None):
    """Align and score call against the model: every field and op exact, the score contract kept."""
    res, ops, o1, o2 = run_align(engine, algo, args, pairs, diags, w, fe, lut)
    score = run_score(engine, algo, args, pairs, diags, w, fe, lut)
    for p, (a, b) in enumerate(pairs):
        want = seeded_model(algo, args, a, b, diags[p], w, fe, lut)
        r = res[p]
        got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
               pair_ops(res, ops, o1, o2, p))
        assert got == want, (algo, args, w, fe, p, len(a), len(b), diags[p])
        assert int(r["flags"]) == 0 and int(r["reserved"]) == 0
        s = score[p]
        assert (int(s["score"]), int(s["end_i"]), int(s["end_j"])) == want[:3], (algo, args, w, fe, p, len(a), len(b), diags[p])
        assert (int(s["start_i"]), int(s["start_j"]), int(s["nops"]), int(s["flags"]), int(s["reserved"])) == (-1, -1, 0, 0, 0)
    return res, ops


# ------------------------------------------------------- 1. every flag set against the model
def legal_batch(seed, w, fe, count):
    """Ragged pairs, m, n in [0, 40], with a random seed diagonal each, drawn until the band is legal."""
    rng = np.random.default_rng(seed)
    pairs, diags = [], []
    for a, b in [(b"", b""), (b"A", b""), (b"", b"AB")]:
        for k in range(-len(a), len(b) + 1):
            if seeded_legal(len(a), len(b), k, w, fe) == (True, True):
                pairs.append((a, b))
                diags.append(k)
    while len(pairs) < count:
        a = seq(rng, ACGT, int(rng.integers(0, 41)))
        b = related(rng, ACGT, a, int(rng.integers(0, 41)))
        k = int(rng.integers(-len(a), len(b) + 1))
        if seeded_legal(len(a), len(b), k, w, fe) == (True, True):
            pairs.append((a, b))
            diags.append(k)
    return pairs, diags


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("fe", range(16))
def test_every_flag_set_matches_the_model(engine, algo, fe):
    for n_w, w in enumerate((0, 1, 3, 8)):
        args = SCORINGS[algo][(fe + n_w) % 3]
        if w == 0 and not scoring_fields(args)[5]:
            args = SCORINGS[algo][0]   # one diagonal needs allow_mismatch
        pairs, diags = legal_batch(1000 * fe + w, w, fe, 16)
        assert pairs[0] == (b"", b"")
        check_model(engine, algo, args, pairs, diags, w, fe)
        check_model(engine, algo, args, pairs, diags, w, fe, PURINE)


def test_hirschberg_means_nw(engine):
    pairs, diags = legal_batch(5, 3, 15, 16)
    a, aops = run_align(engine, HB, (-1, 1, -1), pairs, diags, 3, 15)[:2]
    b, bops = run_align(engine, NW, (-1, 1, -1), pairs, diags, 3, 15)[:2]
    assert a.tobytes() == b.tobytes() and aops.tobytes() == bops.tobytes()


# ------------------------------------------------------- 2. the geometry classes, by name
S1B, S1E, S2B, S2E = sa.SA_FREE_SEQ1_BEGIN, sa.SA_FREE_SEQ1_END, sa.SA_FREE_SEQ2_BEGIN, sa.SA_FREE_SEQ2_END
GEOMETRY = {   # name: (m, n, k, w, free_ends, what the clipped band must satisfy)
    "row 0 to last row": (5, 40, 20, 2, S2B | S2E, lambda m, n, lo, hi: 0 < lo and hi < n - m),
    "column 0 to last column": (40, 5, -20, 2, S1B | S1E, lambda m, n, lo, hi: hi < 0 and lo > n - m),
    "upper right corner": (12, 12, 12, 3, S2B | S1E, lambda m, n, lo, hi: 0 < lo and lo > n - m and hi == n),
    "lower left corner": (12, 12, -12, 3, S1B | S2E, lambda m, n, lo, hi: hi < 0 and hi < n - m and lo == -m),
    "(0, 0) to short of (m, n)": (6, 30, 0, 2, S2E, lambda m, n, lo, hi: lo <= 0 <= hi < n - m),
    "row 0 to (m, n)": (6, 30, 24, 2, S2B, lambda m, n, lo, hi: 0 < lo <= n - m <= hi),
}


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry_class(engine, algo, name):
    m, n, k, w, fe, in_class = GEOMETRY[name]
    lo, hi = seeded_band(m, n, k, w)
    assert in_class(m, n, lo, hi), (lo, hi)
    rng = np.random.default_rng(len(name))
    pairs = []
    for _ in range(5):   # (five pairs: four share a wave, the fifth has a wave's other lanes idle)
        a = seq(rng, ACGT, m)
        b = bytearray(seq(rng, ACGT, n))
        if k >= 0:
            b[k:k + m] = a[:n - k]      # the band's diagonal holds an alignment worth finding
        else:
            b[:min(n, m + k)] = a[-k:-k + min(n, m + k)]
        pairs.append((a, bytes(b)))
    for args in SCORINGS[algo]:
        for flags in (fe, 15):
            res, _ = check_model(engine, algo, args, pairs, [k] * 5, w, flags)
    assert seeded_legal(m, n, k, w, fe & (fe - 1)) != (True, True)   # the class needs both of its flags


# ------------------------------------- 3. every variant, both sides of each capacity
def variant_case(w):
    m = 64
    return m, 2 * w + 72, w   # lo' = 0, hi' = 2w: 2w + 1 diagonals, none clipped, begins on row 0, ends on the last row


@pytest.mark.parametrize("algo,w", [(a, w) for a in (NW, GG) for w in (15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023)]
                         + [(NW, 1024), (NW, 2047)])
def test_every_variant_matches_the_model(engine, algo, w):
    m, n, k = variant_case(w)
    assert seeded_band(m, n, k, w) == (0, 2 * w)
    cells = cells_per_lane(2 * w + 1)
    assert sa.banded_seeded_plan_query(algo, m, n, k, w, FIT)[0] == cells
    rng = np.random.default_rng(w)
    pairs = []
    for off in (w, max(w - 9, 0)):   # the read on the seed diagonal, and nine diagonals off it
        window = bytearray(seq(rng, ACGT, n))
        read = seq(rng, ACGT, m)
        window[off:off + m] = read
        pairs.append((edited(rng, read), bytes(window)))
    check_model(engine, algo, SCORINGS[algo][0], pairs, [k, k], w, FIT)
    assert engine.last_plan_ex()[1] == cells


@pytest.mark.parametrize("algo,w", [(NW, 2048), (GG, 1024)])
def test_one_diagonal_past_the_cap_is_refused(engine, algo, w):
    m, n, k = variant_case(w)
    rng = np.random.default_rng(w)
    pairs = [(seq(rng, ACGT, m), seq(rng, ACGT, n))]
    for call in (run_align, run_score):
        with pytest.raises(sa.SeqalibError, match="unsupported|UNSUPPORTED|diagonals"):
            call(engine, algo, SCORINGS[algo][0], pairs, [k], w, FIT)
    with pytest.raises(sa.SeqalibError):
        sa.banded_seeded_plan_query(algo, m, n, k, w, FIT)


# ------------------- 4. interior steps of the wide variants: the ends-free call by equivalence (b)
@pytest.fixture(scope="module")
def related3000():
    """16 related pairs, m about 3000, n = m + 20 or m - 20."""
    rng = np.random.default_rng(41)
    pairs = []
    for p in range(16):
        a = seq(rng, ACGT, 2990 + 3 * p)
        pairs.append((a, related(rng, ACGT, a, len(a) + (20 if p % 2 else -20))))
    return pairs


@pytest.mark.parametrize("algo,w", [(NW, 16), (NW, 600), (NW, 1100), (GG, 16), (GG, 600)])
def test_corridor_seed_equals_the_ends_free_call(engine, related3000, algo, w):
    """diag = (n - m) / 2 and w' = w + |n - m| / 2: the same band, so every field and op agrees, over
    sweeps long enough for steps without border cells at every width up to 32 cells per lane and step."""
    args = SCORINGS[algo][0]
    sc = sa.ScoringSystem(*args)
    s1, o1, s2, o2 = pack_bytes(related3000)
    diags = [(len(b) - len(a)) // 2 for a, b in related3000]
    assert set(diags) == {10, -10}
    for fe in (0, 9, 12, 15):
        want, wops = engine.align_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, w, fe)
        got, gops = engine.align_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diags, w + 10, fe)
        assert engine.last_plan_ex()[1] == cells_per_lane(20 + 2 * w + 1)
        for f in FIELDS:
            assert np.array_equal(want[f], got[f]), (fe, f)
        for p in range(len(related3000)):
            assert pair_ops(got, gops, o1, o2, p) == pair_ops(want, wops, o1, o2, p), (fe, p)
        assert np.array_equal(rescore(algo, args, got, gops, o1, o2), got["score"].astype(np.int64)), fe
        score = engine.score_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diags, w + 10, fe)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], got[f]), (fe, f)


def test_whole_matrix_band_equals_the_ends_free_call(engine):
    """Equivalence (a), w >= m + n, on the ragged batch of section 1."""
    pairs, diags = legal_batch(77, 100, 15, 24)
    s1, o1, s2, o2 = pack_bytes(pairs)
    for algo in (NW, GG):
        sc = sa.ScoringSystem(*SCORINGS[algo][0])
        for fe in range(16):
            want, wops = engine.align_banded_ends_free_packed(algo, sc, s1, o1, s2, o2, 100, fe)
            got, gops = engine.align_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diags, 100, fe)
            assert want.tobytes() == got.tobytes() and wops.tobytes() == gops.tobytes(), (algo, fe)


# --------------------------------------------------------------------- 5. new ground
@pytest.mark.parametrize("algo,args", [(NW, (-2, 2, -3)), (GG, (-3, -1, 2, -3))])
def test_read_in_a_long_window(engine, algo, args):
    """A 150-symbol read with three edits at a random place of a 100,000-symbol window, seeded within 5
    diagonals of the plant at w = 16: 33 diagonals, where the corridor band would need 99,883."""
    rng = np.random.default_rng(61)
    pairs, diags, starts = [], [], []
    for d in (-5, 0, 5, 3):
        window = seq(rng, ACGT, 100000)
        s = int(rng.integers(200, 99000))
        pairs.append((edited(rng, window[s:s + 150]), window))
        starts.append(s)
        diags.append(s + d)
    assert sa.banded_seeded_plan_query(algo, 150, 100000, diags[0], 16, FIT)[:2] == (2, 4)
    res, _ = check_model(engine, algo, args, pairs, diags, 16, FIT)
    assert engine.last_plan_ex()[1] == 2
    for p, s in enumerate(starts):
        r = res[p]
        assert (int(r["start_i"]), int(r["end_i"])) == (0, 150)
        assert abs(int(r["start_j"]) - s) <= 3 and abs(int(r["end_j"]) - (s + 150)) <= 3, (p, r)
        assert int(r["score"]) >= 2 * 147 - 3 - 2 * 3 - 3
    with pytest.raises(sa.SeqalibError, match="diagonals"):
        engine.align_banded_ends_free_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), 16, FIT)


@pytest.mark.parametrize("algo,args", [(NW, (-2, 2, -3)), (GG, (-3, -1, 2, -3))])
def test_dovetail_overlap(engine, algo, args):
    """Two 2000-symbol reads that overlap by 500: the last 500 symbols of Seq1 are, with three edits, the
    first of Seq2.  Seeded at k = -1500 the overlap needs w = 16; the corridor band would need w >= 1500."""
    rng = np.random.default_rng(62)
    pairs = []
    for _ in range(4):
        s1 = seq(rng, ACGT, 2000)
        tail = edited(rng, s1[1500:])
        pairs.append((s1, tail + seq(rng, ACGT, 2000 - len(tail))))
    res, _ = check_model(engine, algo, args, pairs, [-1500] * 4, 16, OVERLAP)
    for p in range(4):
        r = res[p]
        assert (int(r["start_j"]), int(r["end_i"])) == (0, 2000)
        assert abs(int(r["start_i"]) - 1500) <= 3 and abs(int(r["end_j"]) - 500) <= 3, (p, r)
        assert int(r["score"]) >= 2 * 497 - 3 - 2 * 3 - 3
    # the corridor band at the same w does not hold the overlap's diagonal
    free = engine.score_banded_ends_free_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), 16, OVERLAP)
    assert (free["score"] < res["score"]).all()


# ------------------------------------------------------------- 6. reporting, launches, merging
@pytest.mark.parametrize("algo,records", [(NW, sa.SA_RECORDS_BAND2), (GG, sa.SA_RECORDS_BAND4)])
def test_plan_and_timings(engine, algo, records):
    pairs, diags = legal_batch(9, 5, FIT, 16)
    run_align(engine, algo, SCORINGS[algo][0], pairs, diags, 5, FIT)
    kernel, _, waves, rec = engine.last_plan_ex()
    assert (kernel, waves, rec) == (sa.SA_KERNEL_BANDED, 1, records)
    assert engine.last_timings()[2] >= 1
    run_score(engine, algo, SCORINGS[algo][0], pairs, diags, 5, FIT)
    kernel, _, waves, rec = engine.last_plan_ex()
    assert (kernel, waves, rec) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_NONE)
    assert engine.last_timings()[1] == 0


@pytest.mark.parametrize("algo", [NW, GG])
def test_workspace_limit_splits_the_launch(engine, algo):
    rng = np.random.default_rng(51)
    pairs, diags = [], []
    for k in range(12):
        read = seq(rng, ACGT, 150)
        start = 20 * (k + 1)
        pairs.append((read, seq(rng, ACGT, start) + related(rng, ACGT, read, 150) + seq(rng, ACGT, 320 - start)))
        diags.append(start)
    plans = {sa.banded_seeded_plan_query(algo, len(a), len(b), k, 6, FIT) for (a, b), k in zip(pairs, diags)}
    assert len(plans) == 1   # one variant, equal records
    want, wops = check_model(engine, algo, SCORINGS[algo][0], pairs, diags, 6, FIT)
    launches = engine.last_timings()[2]
    try:
        engine.set_workspace_limit(3 * plans.pop()[2])
        got, gops = run_align(engine, algo, SCORINGS[algo][0], pairs, diags, 6, FIT)[:2]
        assert engine.last_timings()[2] == 4 > launches
    finally:
        engine.set_workspace_limit(0)
    assert want.tobytes() == got.tobytes() and wops.tobytes() == gops.tobytes()


@pytest.mark.parametrize("algo", [NW, GG])
def test_mixed_variants_in_one_call(engine, monkeypatch, algo):
    """One w = 100: clipping gives the short pairs narrower variants."""
    rng = np.random.default_rng(77)
    pairs, diags = [], []
    for m, n in [(3, 4), (5, 9), (14, 10), (20, 28), (31, 31), (40, 90), (60, 50), (100, 120), (130, 100), (150, 300),
                 (300, 160), (250, 250)]:
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, n)))
        diags.append(int(rng.integers(-m // 3, n // 3 + 1)))
    plans = {sa.banded_seeded_plan_query(algo, len(a), len(b), k, 100, 15)[:2] for (a, b), k in zip(pairs, diags)}
    assert len(plans) >= 4
    out = {}
    for merge in ("0", "1"):
        monkeypatch.setenv("SEQALIB_BAND_MERGE", merge)
        res, ops = check_model(engine, algo, SCORINGS[algo][0], pairs, diags, 100, 15)
        run_align(engine, algo, SCORINGS[algo][0], pairs, diags, 100, 15)
        out[merge] = (res.tobytes(), ops.tobytes(), engine.last_timings()[2])
    assert out["0"][:2] == out["1"][:2] and out["1"][2] < out["0"][2]


# ---------------------------------------------------------------------- 7. Python classes
def test_python_classes(engine):
    rng = np.random.default_rng(3)
    win = seq(rng, ACGT, 90)
    pairs = [(win[30:60].decode(), win.decode()), (win.decode(), (win[50:] + seq(rng, ACGT, 6)).decode()), ("ACGT", ""),
             ("", "AC")]
    # (free_ends, a seed per pair, the pairs whose band is legal under these flags)
    cases = [(FIT, [30, 0, 0, 0], [0, 2, 3]), (OVERLAP, [28, -50, -2, 0], [1, 2, 3]), (15, [33, -47, -4, 2], [0, 1, 2, 3])]
    for cls, algo, args in [(sa.NeedlemanWunschSA, NW, (-2, 2, -3)), (sa.HirschbergSA, HB, (-2, 2, -3)),
                            (sa.GlobalGotohSA, GG, (-3, -1, 2, -3))]:
        al = cls(sa.ScoringSystem(*args))
        for fe, all_diags, keep in cases:
            sub = [pairs[p] for p in keep]
            diags = [all_diags[p] for p in keep]
            got = al.getSeededAlignments(sub, diags, 5, fe)
            models = [seeded_model(algo, args, a.encode(), b.encode(), k, 5, fe) for (a, b), k in zip(sub, diags)]
            assert al.getScore() == models[-1][0]
            for (a, b), g, (sc, ei, ej, si, sj, ops) in zip(sub, got, models):
                want = sa.expand_ops(sa.SA_SW, a, b, sa.PairResult(sc, ei, ej, si, sj, 0, ops))   # forceGlobal over (start, end)
                assert g.rows() == want.rows()
                assert len(g.rows()[0].replace("-", "")) == len(a) and len(g.rows()[2].replace("-", "")) == len(b)
            assert al.getSeededScores(sub, diags, 5, fe) == [x[0] for x in models]
            assert al.getSeededEndCells(sub, diags, 5, fe) == [x[1:3] for x in models]
            assert al.getSeededAlignment(*sub[0], diags[0], 5, fe).rows() == got[0].rows()
        with pytest.raises(sa.SeqalibError):   # an illegal band: the engine's message
            al.getSeededAlignments(pairs[:1], [30], 5, 0)
        with pytest.raises(sa.SeqalibError):
            al.getSeededAlignments(pairs[:1], [30, 30], 5, FIT)
    for cls in (sa.SmithWatermanSA, sa.LocalGotohSA, sa.MyersMillerSA):
        with pytest.raises(sa.SeqalibError):
            cls().getSeededAlignments(pairs[:1], [30], 5, FIT)
