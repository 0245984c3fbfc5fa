"""CPU: the inputs of tests/test_gpu_banded_extend_regimes.py can see nine faults an extension kernel could
have.  Each fault is planted in a copy of tests/extend_model.py (tests/extend_mutants.py: one str.replace
whose old text must occur exactly once), and the mutant must give another result than the model on those
inputs.  This is a condition on the inputs, checked on the reference model alone: the GPU tests that
compare a kernel with the model on them would fail for a kernel with the same fault.

The GPU inputs are regime_batch(k) x regime_inputs(k) -- the widths and the xdrop values taken from the
model's own checkpoints -- for each of the 53 (algorithm, scoring) cases, and phase_batch() at w = 12.  Of
the former, ten of the sixteen pairs at w in (3, 8) are searched here: a subset, so a difference found on
it is a difference on the GPU inputs, at a fraction of the model's time.
"""
import pytest

import test_gpu_banded_extend_regimes as reg
from extend_model import GLOBAL_GOTOH, NW, XDROP_PERIOD, extend_band
from extend_mutants import AFFINE_ONLY, MUTATIONS, mutant
from util import scoring_fields

WIDTHS = (3, 8)
SUBSET = (2, 4, 6, 8, 9, 10, 11, 12, 13, 14)   # (b"", b"AB"), three ragged pairs, the disjoint tails, two with m < w


def inputs(k, nonempty=False):
    """(a, b, w, xdrop, table) of scoring number k, the likeliest to stop first."""
    pairs = reg.regime_batch(k)
    assert reg.WIDTHS.count(3) == reg.WIDTHS.count(8) == 1 and len(pairs) == 16
    out = []
    for w, xs, _, _ in reg.regime_inputs(k):
        if w in WIDTHS:
            out += [(*pairs[p], w, x, reg.uses_table(k)) for x in xs[::-1] for p in SUBSET[::-1]
                    if not nonempty or (pairs[p][0] and pairs[p][1])]
    return out


def differs(fn, algo, args, cases):
    """Does the mutant give another result than the model (a walk that dead-ends or trips one of the model's
    assertions is another result)?"""
    for a, b, w, x, table in cases:
        try:
            if fn(algo, args, a, b, w, x, reg.PURINE if table else None) != reg.model(algo, args, a, b, w, x, table):
                return True
        except AssertionError:
            return True
    return False


def seen(name, nonempty=False):
    fn = mutant(name)
    return [reg.CASES[k] for k in range(len(reg.CASES))
            if (name not in AFFINE_ONLY or reg.CASES[k][0] == GLOBAL_GOTOH) and differs(fn, *reg.CASES[k], inputs(k, nonempty))]


def positive_border(case):
    g, _, _, go, ge, _ = scoring_fields(case[1])
    return (go + ge if case[0] == GLOBAL_GOTOH else g) > 0


def test_there_are_nine_faults():
    assert len(MUTATIONS) == 9 and set(AFFINE_ONLY) < set(MUTATIONS)


@pytest.mark.parametrize("name", [n for n in MUTATIONS if n != "checkpoint at tend"])
def test_the_regime_inputs_see_the_mutant(name):
    # (0, 0) as no candidate changes every empty pair's score: the pairs without symbols are left out, so that
    # what is seen is an interior cell that lost to (0, 0)
    cases = seen(name, nonempty=name == "(0, 0) is no candidate")
    print(f"{name}: differs under {len(cases)} scorings: {cases}")
    assert cases, name
    if name == "border cells are candidates":
        assert any(positive_border(c) for c in cases), cases   # a border that rises: it beats the interior
    if name == "recent takes border cells":
        # Seen where the border falls (gap < 0: a window maximum taken from a border cell hides a fall of the
        # interior).  Not where it rises: with gap > 0 (gap_open + gap_extend > 0) and w >= 1 every interior
        # cell has an upper or a left neighbour in the band and exceeds it, so the window that follows the
        # best cell holds a larger one, best - recent is never positive, nothing stops at any xdrop and
        # `recent` decides nothing -- and w = 0 has no border cell but (0, 0).  Asserted, not assumed:
        assert not any(positive_border(c) for c in cases), cases
        for k, case in enumerate(reg.CASES):
            if positive_border(case):
                assert all(v <= 0 for w in reg.regime_widths(case[1]) if w for v in reg.regime_falls(k, w)), case
        assert any(scoring_fields(c[1])[0] < 0 or scoring_fields(c[1])[3] + scoring_fields(c[1])[4] < 0 for c in cases)
    if name == "first maximum":
        assert (NW, (0, 0, 0)) in cases   # every cell ties
    if name == "(0, 0) is no candidate":
        assert any(scoring_fields(c[1])[1] <= 0 for c in cases), cases   # match <= 0: every interior cell can be negative
    if name == "border constant":
        # gap terms in the thousands: the only scorings under which pairs this short show the constant
        assert all(scoring_fields(c[1])[3] <= -2048 for c in cases), cases


def test_the_phase_pairs_see_a_checkpoint_at_tend():
    """Among the 53 cases the fault shows only where a pair's tend happens to be 15 mod 16; the phase pairs of
    phase_batch() are built for it."""
    fn = mutant("checkpoint at tend")
    pairs = reg.phase_batch()
    for algo, args in reg.PHASE_SCORING.items():
        hit = [(len(a), len(b)) for a, b in pairs if differs(fn, algo, args, [(a, b, reg.PHASE_W, 10, False)])]
        print(f"checkpoint at tend, algorithm {algo}: differs on {hit}")
        assert reg.PHASE_PAIRS[15] in hit
        assert all(extend_band(m, n, reg.PHASE_W)[2] % XDROP_PERIOD == XDROP_PERIOD - 1 for m, n in hit)
    cases = seen("checkpoint at tend")
    print(f"checkpoint at tend: differs under {len(cases)} scorings of the regime batches: {cases}")


def test_the_unmutated_copy_is_the_model():
    copy = mutant(None)
    for k in (5, 40):
        assert not differs(copy, *reg.CASES[k], inputs(k))
    assert not differs(copy, NW, reg.PHASE_SCORING[NW], [(a, b, reg.PHASE_W, 10, False) for a, b in reg.phase_batch()])


def test_at_least_thirty_scorings_can_stop():
    """The count test_gpu_banded_extend_regimes.py asserts before it calls the GPU, for the runs without one."""
    n = sum(reg.can_stop(k) for k in range(len(reg.CASES)))
    print(f"{n} of {len(reg.CASES)} scorings can stop")
    assert n >= 30
