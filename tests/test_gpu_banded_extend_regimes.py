"""GPU parity of the banded X-drop extension calls (sa_align_batch_banded_extend, sa_score_batch_banded_extend)
on the scorings outside gap < 0 < match, mismatch < 0 (util.REGIME_LINEAR under NW, util.REGIME_AFFINE_BANDED
under GlobalGotoh), next to the header's 2^29 score bound, on waves whose pairs have different lo' and
different checkpoint phases, and on mixed waves of 2 and of 1 pair.

test_gpu_banded_regimes.py put the four earlier banded families through these scorings; extension has code
of its own where they bite (the end-cell key that starts at (0, 0), the window maximum over interior cells
only, the int32 stop test against the -2^30 sentinel, the t < tend rule).  Every comparison is exact --
score, end cell, start, nops, every op, flags 0 or SA_FLAG_DROPPED as the model says, reserved == 0 and the
score call's contract (test_gpu_banded_extend.check_model) -- against tests/extend_model.py, which
tests/test_extend_model.py pins on the same scorings; tests/test_extend_sensitivity.py shows that these very
inputs tell nine planted faults from the model.  The xdrop values come from the model's checkpoints, never
from the kernel, and what an input is meant to do (some pair stops, some does not, nothing stops, the last
window would trip the rule, a wave holds two different lo') is asserted on the model before the GPU is
called.
"""
import functools

import numpy as np
import pytest

import seqalib_amd as sa
from extend_model import XDROP_PERIOD, extend_band, extend_fill_np, extend_model
from extend_mutants import mutant
from test_gpu_banded import ACGT, pair_ops, seq
from test_gpu_banded_extend import (DROPPED, GG, NW, OFF, PURINE, cells_per_lane, check_model, drop_inputs, edited, model,
                                    variant_pairs)
from test_gpu_banded_regimes import BOUND_AFFINE, BOUND_LINEAR, bound_pairs
from test_gpu_regimes import ident
from util import REGIME_AFFINE_BANDED, REGIME_LINEAR, pack_bytes, scoring_fields

pytestmark = pytest.mark.gpu
BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py)

CASES = [(NW, s) for s in REGIME_LINEAR] + [(GG, s) for s in REGIME_AFFINE_BANDED]
assert len(CASES) == 53
ID = lambda v: ident(v) if isinstance(v, tuple) else str(v)
WIDTHS = (0, 1, 3, 8)
INT_MAX_W = 3   # the width that also runs xdrop = 2^31 - 1
INT_MAX = 2 ** 31 - 1


def banded(engine):
    assert engine.last_plan_ex()[0] == sa.SA_KERNEL_BANDED, engine.last_plan_ex()


def launch_order(pairs):
    """The order in which a launch takes the pairs of one fill variant: longest m + n first, ties in input
    order (sa_band_group.h, tests/cpp/band_group_test.cpp); consecutive pairs share a wave."""
    return sorted(range(len(pairs)), key=lambda p: -(len(pairs[p][0]) + len(pairs[p][1])))


def disjoint_tails(rng, head, ta, tb):
    """A related head (about 5 % edits), then tails over disjoint symbols: the score falls wherever it can."""
    h = seq(rng, ACGT, head)
    return h + b"A" * ta, edited(rng, h, 0.05) + b"C" * tb


# ------------------------------------------------------- a. model parity per (algorithm, scoring)
def uses_table(k):
    return k % 2 == 1   # the purine table on every other scoring


@functools.lru_cache(maxsize=None)
def regime_batch(k):
    """The 16 pairs of scoring number k, at most 80 symbols each."""
    rng = np.random.default_rng(7000 + k)
    pairs = [(b"", b""), (b"A", b""), (b"", b"AB")]
    for _ in range(6):   # ragged: a related prefix and an unrelated rest
        a = seq(rng, ACGT, int(rng.integers(1, 61)))
        n = int(rng.integers(1, 61))
        r = int(rng.integers(0, min(len(a), n) + 1))
        pairs.append((a, edited(rng, a[:r], 0.1)[:n] + seq(rng, ACGT, max(0, n - r))))
    for head in (0, 5, 20, 33):
        pairs.append(disjoint_tails(rng, head, int(rng.integers(20, min(60, 78 - head) + 1)),
                                    int(rng.integers(20, min(60, 78 - head) + 1))))
    for x in range(3):   # m < w at w = 8 (lo' = -m), and one n < w
        a = seq(rng, ACGT, int(rng.integers(3, 8)))
        b = edited(rng, a, 0.1) + seq(rng, ACGT, int(rng.integers(30, 61)))
        pairs.append((b, a) if x == 2 else (a, b))
    assert len(pairs) == 16 and all(len(a) <= 80 and len(b) <= 80 for a, b in pairs)
    assert sum(0 < len(a) < 8 < len(b) for a, b in pairs) >= 2
    return pairs


def regime_widths(args):
    return [w for w in WIDTHS if w or scoring_fields(args)[5]]   # (w = 0 without allow_mismatch: the contract's status)


@functools.lru_cache(maxsize=None)
def regime_falls(k, w):
    """best - recent of every checkpoint of the batch's unstopped model runs."""
    algo, args = CASES[k]
    out = []
    for a, b in regime_batch(k):
        trace = []
        extend_model(algo, args, a, b, w, OFF, PURINE if uses_table(k) else None, trace=trace)
        out += [best - recent for _, best, recent in trace]
    return out


def xdrops_of(falls):
    """(xdrops, g, largest): {OFF, 0, g - 1, g, largest + 1} with g the median of the positive falls, an
    element of them, so xdrop = g meets a checkpoint with best - recent == xdrop; (OFF, 0, 5) where the score
    never falls."""
    pos = sorted(v for v in falls if v > 0)
    if not pos:
        return [OFF, 0, 5], None, None
    g = pos[(len(pos) - 1) // 2]
    return list(dict.fromkeys([OFF, 0, g - 1, g, pos[-1] + 1])), g, pos[-1]


def can_stop(k):
    return any(v > 0 for w in regime_widths(CASES[k][1]) for v in regime_falls(k, w))


def regime_inputs(k):
    """[(w, xdrops, g, largest)] of scoring number k: what test_regime_batches_match_the_model sends to the GPU
    (with regime_batch(k) and uses_table(k))."""
    out = []
    for w in regime_widths(CASES[k][1]):
        xs, g, largest = xdrops_of(regime_falls(k, w))
        out.append((w, xs + [INT_MAX] * (w == INT_MAX_W), g, largest))
    return out


def test_at_least_thirty_scorings_can_stop():
    """On the CPU: the scorings under which some checkpoint of some pair has best - recent > 0."""
    n = sum(can_stop(k) for k in range(len(CASES)))
    print(f"{n} of {len(CASES)} scorings can stop")
    assert n >= 30


@pytest.mark.parametrize("algo,args", CASES, ids=ID)
def test_regime_batches_match_the_model(engine, algo, args):
    k = CASES.index((algo, args))
    pairs, table = regime_batch(k), uses_table(k)
    for w, xs, g, largest in regime_inputs(k):
        flags = lambda x: [model(algo, args, a, b, w, x, table)[6] for a, b in pairs]
        if g is None:
            assert not any(any(flags(x)) for x in xs), (w, "nothing stops")
        else:
            some = flags(g - 1)
            assert any(some) and not all(some), (w, g, "some pair stops, some pair runs on")
            assert not any(flags(largest + 1)), (w, largest)
        for x in xs:
            check_model(engine, algo, args, pairs, w, x, table)
            banded(engine)


# ------------------------------------------------- b. the wide variants under regime scorings
# per algorithm: gap (gap_open) > 0, match <= 0, gap terms in the thousands
WIDE_SCORINGS = {NW: [(1, 1, -1), (-1, 0, -1), (-4096, 31, -32)],
                 GG: [(2, -1, 1, -1, True), (-3, -1, 0, -1, True), (-2048, -512, 15, -16, True)]}
# GlobalGotoh stops at w = 511: at w = 1023 (16 cells per lane) under the first scoring the clipped pair of
# variant_pairs() -- 40 x 1073, whose best cell is the last cell of the sweep -- came back with a walk that
# read record words the call had not written (start (39, 1063), not (0, 0); the result changed with
# SA_HOOK_POISON_WS), and the same shape as a fresh context's first call ended in an illegal memory access.
# Score, end cell and flag were the numpy fill's.  The cause is not found, so the case is not run (DESIGN.md
# section 2.18); test_gpu_banded_extend.test_every_variant still runs that variant with its ordinary scoring.
WIDE_W = {NW: (15, 31, 63, 127, 255, 511, 1023, 2047), GG: (15, 31, 63, 127, 255, 511)}


def test_the_wide_scorings_are_regime_scorings():
    for algo, ss in WIDE_SCORINGS.items():
        assert all((algo, s) in CASES for s in ss)
        gap = lambda s: scoring_fields(s)[3] if algo == GG else scoring_fields(s)[0]
        assert gap(ss[0]) > 0 and scoring_fields(ss[1])[1] <= 0 and gap(ss[2]) <= -2048


@pytest.mark.parametrize("algo,w", [(a, w) for a in (NW, GG) for w in WIDE_W[a]])
def test_every_variant_under_a_regime_scoring(engine, algo, w):
    """Score, end cell and flag against the numpy fill; the ops through the header's equivalence (a) against
    the seeded call (test_mixed_waves_of_two_and_one below compares the family's ops with the model)."""
    args = WIDE_SCORINGS[algo][WIDE_W[algo].index(w) % 3]
    pairs = variant_pairs(w)
    assert sa.banded_extend_plan_query(algo, len(pairs[0][0]), len(pairs[0][1]), w)[0] == cells_per_lane(2 * w + 1)
    off, falls = [], []
    for a, b in pairs:
        trace = []
        off.append(extend_fill_np(algo, args, a, b, w, OFF, trace=trace))
        falls.append([best - recent for _, best, recent in trace])
    xs, g, largest = xdrops_of(sum(falls, []))

    def fill(p, x):   # a pair whose unstopped checkpoints never exceed x runs as the unstopped sweep does
        return off[p] if x == OFF or max(falls[p], default=0) <= x else extend_fill_np(algo, args, *pairs[p], w, x)

    if g is None:
        assert WIDE_SCORINGS[algo].index(args) == 0   # (gap > 0: the score rises with every step)
    else:
        assert any(fill(p, g - 1)[3] for p in range(3)) and not any(fill(p, largest + 1)[3] for p in range(3))
    s1, o1, s2, o2 = pack_bytes(pairs)
    sc = sa.ScoringSystem(*args)
    for x in xs:
        res, ops = engine.align_banded_extend_packed(algo, sc, s1, o1, s2, o2, w, x)
        assert engine.last_plan_ex()[:2] == (sa.SA_KERNEL_BANDED, cells_per_lane(2 * w + 1))
        score = engine.score_banded_extend_packed(algo, sc, s1, o1, s2, o2, w, x)
        banded(engine)
        for p in range(3):
            want, ei, ej, drop, _ = fill(p, x)
            for r in (res[p], score[p]):
                assert (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["flags"]), int(r["reserved"])) == \
                    (want, ei, ej, DROPPED if drop else 0, 0), (w, x, p)
            assert (int(res[p]["start_i"]), int(res[p]["start_j"])) == (0, 0)
            assert (int(score[p]["start_i"]), int(score[p]["start_j"]), int(score[p]["nops"])) == (-1, -1, 0)
        prefixes = [(a[:int(r["end_i"])], b[:int(r["end_j"])]) for (a, b), r in zip(pairs, res)]
        p1, q1, p2, q2 = pack_bytes(prefixes)
        sres, sops = engine.align_banded_seeded_packed(algo, sc, p1, q1, p2, q2, [0] * 3, w, 0)
        banded(engine)
        for p in range(3):
            for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops"):
                assert int(res[p][f]) == int(sres[p][f]), (w, x, p, f)
            assert pair_ops(res, ops, o1, o2, p) == pair_ops(sres, sops, q1, q2, p), (w, x, p)


# ------------------------------------------------------------------ c. at the score bound
BOUND_W = (1, 8, 256)
BOUND_XDROPS = (OFF, 0, 2 ** 20, 2 ** 29, 2 ** 30, INT_MAX)


@functools.lru_cache(maxsize=None)
def bound_batch(linear):
    return bound_pairs(linear) + [disjoint_tails(np.random.default_rng(31), 30, 60, 50)]


@pytest.mark.parametrize("algo", [NW, GG])
def test_at_the_score_bound(engine, algo):
    """Gap terms of a million, scores of up to 2.6e8 in magnitude and xdrop up to INT32_MAX: best - recent is
    taken in int32 against the -2^30 sentinel, and nothing may wrap."""
    args = BOUND_LINEAR if algo == NW else BOUND_AFFINE
    pairs = bound_batch(algo == NW)
    for a, b in pairs:
        if algo == NW:
            assert (len(a) + len(b) + 1) * 1048575 < 2 ** 29
        else:
            assert (len(a) + len(b) + 1) * 2096000 + 10000 < 2 ** 29
        for w in BOUND_W:
            lo, hi, _ = extend_band(len(a), len(b), w)
            assert (len(a) + 1) * (hi - lo + 1) < 2 ** 31
    assert max(max(len(a), len(b)) for a, b in pairs) <= BOUND_W[-1]   # (the last width holds the whole matrix)
    stops = {x: sum(model(algo, args, a, b, w, x)[6] for a, b in pairs for w in BOUND_W) for x in BOUND_XDROPS}
    assert stops[2 ** 20] > 0 and stops[2 ** 30] == 0 and stops[INT_MAX] == 0, stops
    for w in BOUND_W:
        for x in BOUND_XDROPS:
            check_model(engine, algo, args, pairs, w, x)
            banded(engine)


# ------------------------------------ d. checkpoint phase and clipped bands in one wave
PHASE_W = 12
PHASE_SCORING = {NW: (-2, 1, -3), GG: (-4, -1, 1, -3)}
# in launch order (m + n falls): every wave of four holds pairs with m < w (lo' = -m, both parities), and
# transposes (n < w), unclipped pairs or the phase pairs (lo' = -w)
PHASE_SHAPES = [(11, 70), (70, 10), (4, 70), (66, 7),
                (34, 35), (3, 66), (34, 34), (8, 60),
                (33, 34), (7, 60), (33, 33), (6, 60),
                (9, 55), (50, 10), (5, 50), (25, 28),
                (10, 40), (40, 3), (3, 40), (20, 20),
                (12, 13), (0, 0)]
PHASE_PAIRS = {14: (33, 33), 15: (33, 34), 0: (34, 34), 1: (34, 35)}   # tend % 16: (m, n)
PHASE_HEAD = 17


@functools.lru_cache(maxsize=None)
def phase_batch():
    """PHASE_SHAPES, shuffled.  A phase pair is 17 equal symbols and disjoint tails: its best cell (17, 17) is
    step 46, so the checkpoint after step 63 sees a fall of one mismatch and the window 64 .. 79 one of nine."""
    rng = np.random.default_rng(12)
    pairs = []
    for m, n in PHASE_SHAPES:
        if (m, n) in PHASE_PAIRS.values():
            h = seq(rng, ACGT, PHASE_HEAD)
            pairs.append((h + b"A" * (m - PHASE_HEAD), h + b"C" * (n - PHASE_HEAD)))
        else:
            a = seq(rng, ACGT, m)
            r = min(m, n, 24) if len(pairs) % 3 else 0   # related up to 24 symbols, or not at all
            pairs.append((a, (edited(rng, a[:r], 0.05) + seq(rng, ACGT, n))[:n]))
    order = rng.permutation(len(pairs))
    return [pairs[p] for p in order]


def test_phase_batch_is_what_it_is_meant_to_be():
    """On the CPU: the conditions of test_checkpoint_phases_and_clipped_bands_share_waves."""
    pairs = phase_batch()
    shapes = [(len(a), len(b)) for a, b in pairs]
    assert sorted(shapes) == sorted(PHASE_SHAPES)
    clipped = [(m, n) for m, n in shapes if 3 <= m < PHASE_W]
    assert all(40 <= n <= 70 for _, n in clipped) and {m % 2 for m, _ in clipped} == {0, 1}
    assert sum(n < PHASE_W <= m for m, n in shapes) >= 4 and sum(min(m, n) >= PHASE_W for m, n in shapes) >= 7
    order = launch_order(pairs)
    for k in range(0, len(pairs), 4):
        assert len({extend_band(*shapes[p], PHASE_W)[0] for p in order[k:k + 4]}) >= 2, (k, [shapes[p] for p in order[k:k + 4]])
    at_tend = mutant("checkpoint at tend")
    for algo, args in PHASE_SCORING.items():
        for phase, shape in PHASE_PAIRS.items():
            a, b = pairs[shapes.index(shape)]
            tend = extend_band(len(a), len(b), PHASE_W)[2]
            assert tend % XDROP_PERIOD == phase
            want = model(algo, args, a, b, PHASE_W, 10)
            # 14, 15: the pair runs to its last step; 0, 1: the checkpoint after step tend - 1 or tend - 2 stops it
            assert want[7] == (None if phase >= 14 else tend - 1 - phase), (phase, want)
            if phase == 15:   # the last window would trip the rule, were there a checkpoint after step tend
                trace = []
                got = at_tend(algo, args, a, b, PHASE_W, 10, trace=trace)
                t, best, recent = trace[-1]
                assert t == tend and best - recent > 10 and got[7] == tend and got[:6] == want[:6]
        stopped = [model(algo, args, a, b, PHASE_W, 10)[6] for a, b in pairs]
        assert any(stopped) and not all(stopped)


@pytest.mark.parametrize("algo", [NW, GG])
def test_checkpoint_phases_and_clipped_bands_share_waves(engine, algo):
    """Pairs of one wave with different lo' start at different steps (tb) and have different record phases
    while sharing the wave-uniform checkpoints; a pair whose last step is a checkpoint step does not stop
    there.  Also over a poisoned workspace: a stopped pair leaves record words unwritten."""
    pairs = phase_batch()
    test_phase_batch_is_what_it_is_meant_to_be()
    assert all(sa.banded_extend_plan_query(algo, len(a), len(b), PHASE_W)[:2] == (1, 4) for a, b in pairs)
    for x in (10, OFF):
        check_model(engine, algo, PHASE_SCORING[algo], pairs, PHASE_W, x)
        banded(engine)
    for value in (0xFFFFFFFF, 0):
        engine.test_hook(sa.SA_HOOK_POISON_WS, value)
        check_model(engine, algo, PHASE_SCORING[algo], pairs, PHASE_W, 10)


# ----------------------------- e. mixed waves at 2 and at 1 pair per wave, ops against the model
@functools.lru_cache(maxsize=None)
def mixed_seven():
    """Diverging, island, related and empty pairs of test_gpu_banded_extend.drop_inputs(), cut so that in
    launch order (m + n falls) stopped and running pairs alternate."""
    div, isl, rel = drop_inputs()
    cut = lambda pair, k: (pair[0][:k], pair[1][:k])
    pairs = [cut(rel[2], 130), div[0], (b"", b""), cut(isl[0], 190), rel[0], cut(div[1], 150), rel[1]]
    assert all(len(a) <= 250 and len(b) <= 250 for a, b in pairs)
    return pairs


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("w,per_wave", [(100, 2), (200, 1)])
def test_mixed_waves_of_two_and_one(engine, algo, w, per_wave):
    args = PHASE_SCORING[algo]
    pairs = mixed_seven()
    full = [(a, b) for a, b in pairs if a]
    assert len(pairs) == 7 and len(full) == 6
    plans = {sa.banded_extend_plan_query(algo, len(a), len(b), w)[:2] for a, b in full}
    assert len(plans) == 1 and plans.pop()[1] == per_wave   # one variant: one launch in launch_order()
    flags = [model(algo, args, *full[p], w, 10)[6] for p in launch_order(full)]
    if per_wave == 2:
        assert all(flags[k] != flags[k + 1] for k in (0, 2, 4)), flags   # every wave: a stopped and a running pair
    assert sum(flags[k] != flags[k + 1] for k in range(5)) >= 3, flags
    check_model(engine, algo, args, pairs, w, 10)
    banded(engine)
