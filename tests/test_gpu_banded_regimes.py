"""GPU parity of the banded affine, banded matrix, ends-free and seeded calls on the scorings outside
gap < 0 < match, mismatch < 0 (util.REGIME_LINEAR, util.REGIME_AFFINE_BANDED), and of the int32 banded
kernels next to the header's 2^29 score bound.

test_gpu_regimes.py runs those scorings through the linear banded call alone; the four call families
added since have border, sentinel and tie handling of their own (sa_banded_affine_fill.h, the free and
seeded modes of sa_banded_fill.h, the table modes).  Whole-matrix bands are compared with sa_align_batch
and the oracle, narrow bands with the Python models, which tests/test_*_model.py pin on the same scorings
and tests/test_regime_sensitivity.py shows to tell a wrong border constant, gap-term order, tie order or
end cell on these very inputs.  Every comparison is exact -- score, end cell, start cell, nops, op stream,
flags == 0, reserved == 0 and the score call's contract -- and every test asserts SA_KERNEL_BANDED.
gap_extend > 0 is refused by these calls (test_banded_affine_abi.py), so (-3, 1, 1, -1) is not run.
"""
import numpy as np
import pytest

import seqalib_amd as sa
import test_gpu_banded as lin
import test_gpu_banded_affine as aff
import test_gpu_banded_matrix as mat
import test_gpu_banded_seeded as sdd
import test_gpu_ends_free as efr
from seeded_model import seeded_band, seeded_legal
from test_gpu_banded import AA, ACGT, FIELDS, pair_ops, ragged_pairs, related, seq
from test_gpu_ends_free import small   # noqa: F401  (the module fixture, used by name below)
from test_gpu_regimes import _f16_cell_on, assert_exact, ident, narrow_pairs, op_bytes, oracle   # noqa: F401
from util import (LG_HACK_SIZES, REGIME_AFFINE_BANDED, REGIME_DIVERGING, REGIME_LINEAR, pack_bytes, scoring_fields)

pytestmark = pytest.mark.gpu
BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py)

SW, NW, LG, GG = sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH
AFFINE_BANDED = REGIME_AFFINE_BANDED
assert REGIME_DIVERGING[1] not in AFFINE_BANDED   # LocalGotoh (-3, 1, 1, -1): refused, nothing to run
FIT, OVERLAP = efr.FIT, efr.OVERLAP
ID = lambda v: ident(v) if isinstance(v, tuple) else str(v)


def banded(engine):
    assert engine.last_plan_ex()[0] == sa.SA_KERNEL_BANDED, engine.last_plan_ex()


def allows(args):
    return bool(scoring_fields(args)[5])


def same_results(got, want, batch, what):
    """(results, ops) of two calls: every field and every op equal."""
    for f in FIELDS:
        assert np.array_equal(got[0][f], want[0][f]), (what, f)
    assert (got[0]["flags"] == 0).all() and (got[0]["reserved"] == 0).all(), what
    nops = got[0]["nops"]
    assert np.array_equal(op_bytes(nops, got[1], batch[1], batch[3]), op_bytes(nops, want[1], batch[1], batch[3])), (what, "ops")


def score_contract(score, res, what):
    for f in ("score", "end_i", "end_j"):
        assert np.array_equal(score[f], res[f]), (what, f)
    assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all(), what
    assert (score["flags"] == 0).all() and (score["reserved"] == 0).all(), what


# ------------------------------------------------------- a. banded affine, whole-matrix band
@pytest.fixture(scope="module")
def third():
    """Every third pair of test_gpu_banded.py's ragged DNA batch, without the LocalGotoh size-hack shapes."""
    pairs = [p for p in ragged_pairs(11, ACGT)[::3] if (len(p[0]), len(p[1])) not in LG_HACK_SIZES]
    diagonals = max(len(a) + len(b) + 1 for a, b in pairs)
    assert 1024 < diagonals <= aff.MAX_DIAGONALS and len(pairs) >= 30
    return pack_bytes(pairs)


@pytest.mark.parametrize("algo", [LG, GG])
@pytest.mark.parametrize("args", AFFINE_BANDED, ids=ident)
def test_affine_whole_matrix_band(engine, third, algo, args):
    """band = 4096 is sa_align_batch and the oracle, field for field and op for op; a pair of more than
    1024 diagonals puts the call on the 16-cells-per-lane fill."""
    sc = sa.ScoringSystem(*args)
    full = engine.align_packed(algo, sc, *third)
    full = (full[0].copy(), full[1].copy())
    band = engine.align_banded_affine_packed(algo, sc, *third, 4096)
    plan = engine.last_plan_ex()
    assert plan[0] == sa.SA_KERNEL_BANDED and plan[1] == 16, plan
    same_results(band, full, third, ("full", algo, args))
    assert_exact(band, oracle(f"third{algo}", algo, args, third), third, ("band", algo, args))
    score = engine.score_banded_affine_packed(algo, sc, *third, 4096)
    banded(engine)
    score_contract(score, band[0], (algo, args))


# ---------------------------------------- b. banded affine, narrow bands against the model
AFFINE_NARROW_W = (0, 1, 3, 32, 65)


def affine_narrow_pairs(alphabet=ACGT):
    """test_gpu_regimes.narrow_pairs() (nine pairs <= 80 long) and two related pairs of 300 x 330 and
    330 x 300, which have 161 diagonals at w = 65."""
    rng = np.random.default_rng(88)
    pairs = narrow_pairs()
    for m, n in ((300, 330), (330, 300)):
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, n)))
    if alphabet is not ACGT:
        pairs = mat.redraw(pairs, alphabet, 89)
    return pairs


def narrow_widths(args):
    return [w for w in AFFINE_NARROW_W if w or allows(args)]   # one diagonal needs allow_mismatch


@pytest.mark.parametrize("algo", [LG, GG])
@pytest.mark.parametrize("args", AFFINE_BANDED, ids=ident)
def test_affine_narrow_band_matches_model(engine, algo, args):
    pairs = affine_narrow_pairs()
    variants = set()
    for w in narrow_widths(args):
        aff.check_model(engine, algo, args, pairs, w)
        banded(engine)
        variants |= {sa.banded_affine_plan_query(algo, len(a), len(b), w)[:2] for a, b in pairs}
    # (cells per lane, pairs per wave): fewer than 4 pairs per wave means lanes of more than one 16-lane group
    assert len(variants) >= 3 and any(per_wave < 4 for _, per_wave in variants), variants


# ------------------------------------------------------------------ c. at the score bound
BOUND_LINEAR = (-1048575, 1048575, -1048575)
BOUND_AFFINE = (-1048000, -1048000, 2096000, -2096000)


def bound_pairs(linear):
    rng = np.random.default_rng(29)
    pairs = []
    for m, n in ((100, 97), (64, 64), (120, 131)):
        a = seq(rng, ACGT, m)
        pairs.append((a, related(rng, ACGT, a, n)))
    pairs.append((seq(rng, ACGT, 110), seq(rng, ACGT, 100)))
    pairs += [(b"G", b"G"), (b"", seq(rng, ACGT, 7))]
    if linear:
        pairs += [(b"", seq(rng, ACGT, 250)), (seq(rng, ACGT, 250), b"")]
    return pairs


@pytest.mark.parametrize("algo", [SW, NW, LG, GG])
def test_at_the_score_bound(engine, algo):
    """Gap terms of a million and scores of up to 2.6e8 in magnitude, every pair inside the header's bound
    (the 120 x 131 pair reaches 98 % of the affine one, the 250-long border pairs half the linear one):
    the out-of-band sentinel (-2^30) plus one gap term must not meet a real score, and nothing may wrap."""
    linear = algo in (SW, NW)
    args = BOUND_LINEAR if linear else BOUND_AFFINE
    pairs = bound_pairs(linear)
    for a, b in pairs:
        if linear:
            assert (len(a) + len(b) + 1) * 1048575 < 2 ** 29
        else:
            assert (len(a) + len(b) + 1) * 2096000 + 10000 < 2 ** 29
    assert max(len(a) + len(b) for a, b in pairs) >= 250
    batch = pack_bytes(pairs)
    sc = sa.ScoringSystem(*args)
    align = engine.align_banded_packed if linear else engine.align_banded_affine_packed
    score = engine.score_banded_packed if linear else engine.score_banded_affine_packed
    band = align(algo, sc, *batch, 4096)
    banded(engine)
    assert_exact(band, oracle(f"bound{algo}", algo, args, batch), batch, ("bound", algo))
    score_contract(score(algo, sc, *batch, 4096), band[0], ("bound", algo))
    banded(engine)
    for w in (1, 8):
        (lin if linear else aff).check_model(engine, algo, args, pairs, w)
        banded(engine)
    if algo in (NW, GG):
        for w in (1, 8, 4096):
            efr.check_model(engine, algo, args, pairs, w, 15)
            banded(engine)


# ------------------------------------------------- d. banded matrix with regime gap terms
def matrix_cases():
    """(algorithm, scoring): every regime scoring that allows mismatches, under the algorithms it applies to."""
    return [(algo, s) for algo in (SW, NW, LG, GG) for s in (REGIME_LINEAR if algo in (SW, NW) else AFFINE_BANDED)
            if allows(s)]


@pytest.mark.parametrize("algo,args", matrix_cases(), ids=ID)
def test_degenerate_table_equals_the_call_without_a_table(engine, algo, args):
    """S[a][b] = (a == b ? match : mismatch): sa_align_batch_banded_matrix is the same family's call
    without a table in every field and op, at a narrow and at a whole-matrix band."""
    _, ma, mi, _, _, _ = scoring_fields(args)
    tab = np.where(np.eye(256, dtype=bool), ma, mi).astype(np.int16)
    assert int(tab[0, 0]) == ma and int(tab[0, 1]) == mi   # (both fit int16)
    batch = pack_bytes(affine_narrow_pairs())
    sc = sa.ScoringSystem(*args)
    plain = engine.align_banded_affine_packed if mat.affine(algo) else engine.align_banded_packed
    for w in (3, 4096):
        want = plain(algo, sc, *batch, w)
        want = (want[0].copy(), want[1].copy())
        banded(engine)
        got = engine.align_banded_matrix_packed(algo, sc, *batch, tab, w)
        banded(engine)
        same_results(got, want, batch, (algo, args, w))
        score_contract(engine.score_banded_matrix_packed(algo, sc, *batch, tab, w), want[0], (algo, args, w))
        banded(engine)


MATRIX_LINEAR_GAPS = [0, 1, 2, -700, -4097]
MATRIX_AFFINE_GAPS = [(0, 0), (-3, 0), (1, -1), (2, -1), (0, -2), (-2048, -512), (-6000, -5000)]


@pytest.fixture(scope="module")
def narrow_aa():
    return affine_narrow_pairs(AA)


@pytest.mark.parametrize("algo,gaps", [(a, g) for a in (SW, NW) for g in MATRIX_LINEAR_GAPS]
                         + [(a, g) for a in (LG, GG) for g in MATRIX_AFFINE_GAPS], ids=ID)
def test_random_table_with_regime_gap_terms(engine, narrow_aa, algo, gaps):
    """An asymmetric random table with gap terms 0, > 0 and in the thousands, against banded_matrix_model."""
    tab = mat.random_table(102)
    args = (gaps[0], gaps[1], 1000, -1000) if mat.affine(algo) else (gaps, 1000, -1000)   # (match / mismatch: ignored)
    for w in (0, 2, 16):
        mat.check_model(engine, algo, args, narrow_aa, tab, 102, w)
        banded(engine)


# ----------------------------------------------------------------------------- e. ends-free
ENDS_FREE_CASES = [(NW, s) for s in REGIME_LINEAR] + [(GG, s) for s in AFFINE_BANDED]


def scoring_number(algo, args):
    return (REGIME_LINEAR if algo == NW else AFFINE_BANDED).index(args)


def flag_sets(k):
    """The flag sets of scoring number k, in a fixed order."""
    return list(dict.fromkeys([0, 15, FIT, OVERLAP, (k % 14) + 1]))


def test_ends_free_cases_run_all_sixteen_flag_sets():
    for algo in (NW, GG):
        ran = set()
        for a, s in ENDS_FREE_CASES:
            if a == algo:
                ran |= set(flag_sets(scoring_number(a, s)))
        assert ran == set(range(16)), (algo, ran)


def ends_free_pairs(small):
    """The first eleven shapes of test_gpu_ends_free.py's `small` and its two planted pairs."""
    assert len(small) == 17
    return small[:11] + small[15:]


@pytest.mark.parametrize("algo,args", ENDS_FREE_CASES, ids=ID)
def test_ends_free_matches_model(engine, small, algo, args):
    pairs = ends_free_pairs(small)
    batch = pack_bytes(pairs)
    sc = sa.ScoringSystem(*args)
    base = engine.align_banded_affine_packed if algo == GG else engine.align_banded_packed
    for w in (0, 1, 5, 40):
        if w == 0 and not allows(args):
            continue
        for fe in flag_sets(scoring_number(algo, args)):
            res, ops = efr.check_model(engine, algo, args, pairs, w, fe)
            banded(engine)
            if fe == 0:   # the banded global call, byte for byte
                want, wops = base(algo, sc, *batch, w)
                banded(engine)
                assert res.tobytes() == want.tobytes() and ops.tobytes() == wops.tobytes(), (algo, args, w)


# -------------------------------------------------------------------------------- f. seeded
def geometry_pairs(name):
    """The five pairs of test_gpu_banded_seeded.test_geometry_class: the band's diagonal holds an alignment."""
    m, n, k, w, fe, in_class = sdd.GEOMETRY[name]
    assert in_class(m, n, *seeded_band(m, n, k, w))
    rng = np.random.default_rng(len(name))
    pairs = []
    for _ in range(5):
        a = seq(rng, ACGT, m)
        b = bytearray(seq(rng, ACGT, n))
        if k >= 0:
            b[k:k + m] = a[:n - k]
        else:
            b[:min(n, m + k)] = a[-k:-k + min(n, m + k)]
        pairs.append((a, bytes(b)))
    return pairs


@pytest.mark.parametrize("algo,args", ENDS_FREE_CASES, ids=ID)
def test_seeded_matches_model(engine, small, algo, args):
    k = scoring_number(algo, args)
    sets = flag_sets(k)
    # ragged legal batches, the flag set rotating with the scoring and the width
    for x, w in enumerate((1, 3, 8)):
        fe = sets[(k + x) % len(sets)]
        pairs, diags = sdd.legal_batch(1000 * k + w, w, fe, 16)
        sdd.check_model(engine, algo, args, pairs, diags, w, fe)
        banded(engine)
    # the six geometry classes with their own flags
    for name, (m, n, diag, w, fe, _) in sdd.GEOMETRY.items():
        assert seeded_legal(m, n, diag, w, fe) == (True, True)
        sdd.check_model(engine, algo, args, geometry_pairs(name), [diag] * 5, w, fe)
        banded(engine)
    # equivalence (b) of the header against the ends-free call, where n - m is even: one call per |n - m|
    sc = sa.ScoringSystem(*args)
    groups = {}
    for a, b in ends_free_pairs(small):
        if (len(b) - len(a)) % 2 == 0:
            groups.setdefault(abs(len(b) - len(a)) // 2, []).append((a, b))
    assert len(groups) >= 4
    for x, (half, pairs) in enumerate(sorted(groups.items())):
        fe = sets[(k + x) % len(sets)]
        batch = pack_bytes(pairs)
        want, wops = engine.align_banded_ends_free_packed(algo, sc, *batch, 3, fe)
        want, wops = want.copy(), wops.copy()
        banded(engine)
        diags = [(len(b) - len(a)) // 2 for a, b in pairs]
        got, gops = engine.align_banded_seeded_packed(algo, sc, *batch, diags, 3 + half, fe)
        banded(engine)
        assert got.tobytes() == want.tobytes() and gops.tobytes() == wops.tobytes(), (algo, args, half, fe)
