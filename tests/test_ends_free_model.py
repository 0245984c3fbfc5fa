"""CPU: tests/ends_free_model.py, the restatement the GPU tests of the ends-free banded calls compare
with, is pinned before it is trusted: free_ends = 0 is the banded global model / the oracle, every flag
set agrees with a brute force over trimmed substrings scored by the oracle's global algorithms, and the
model's op stream rescored gives its score."""
import itertools

import numpy as np
import pytest

from banded_affine_model import affine_rescore, banded_affine_model
from ends_free_model import (GLOBAL_GOTOH, NW, SEQ1_BEGIN, SEQ1_END, SEQ2_BEGIN, SEQ2_END, ends_free_model)
from util import REGIME_AFFINE_BANDED, REGIME_LINEAR, linear_rescore, oracle_align, scoring_fields

LINEAR = [(-1, 1, -1), (-2, 2, -3), (0, 1, -1), (-1, -1, -2)]          # gap <= 0
AFFINE = [(-3, -1, 1, -1), (-2, 0, 2, -3), (1, -1, 1, -1), (0, 0, 1, -2)]   # extend <= 0, open + extend <= 0
WHOLE = 64   # a band that is the whole matrix of every pair here
ZERO = np.zeros(2, dtype=np.uint64)   # the offsets of a one-pair batch whose ops start at 0


def _seq(rng, letters, n):
    return bytes(rng.choice(list(letters), n).tolist()) if n else b""


def _pairs(seed, count, letters, max_len=8):
    rng = np.random.default_rng(seed)
    out = [(b"", b""), (b"A", b""), (b"", b"AB"), (b"A", b"A")]
    while len(out) < count:
        out.append((_seq(rng, letters, int(rng.integers(0, max_len + 1))), _seq(rng, letters, int(rng.integers(0, max_len + 1)))))
    return out


def test_no_free_end_is_the_banded_global_model():
    rng = np.random.default_rng(5)
    for args in AFFINE + [(-3, -1, 2, -1, False)] + REGIME_AFFINE_BANDED:
        for _ in range(40):
            a, b = _seq(rng, b"ACG", int(rng.integers(0, 30))), _seq(rng, b"ACG", int(rng.integers(0, 30)))
            w = int(rng.integers(1, 12))
            assert ends_free_model(GLOBAL_GOTOH, args, a, b, w, 0) == banded_affine_model(GLOBAL_GOTOH, args, a, b, w)


def test_no_free_end_whole_band_is_the_oracle_nw():
    rng = np.random.default_rng(6)
    for args in LINEAR + [(-1, 2)] + REGIME_LINEAR:
        for _ in range(40):
            a, b = _seq(rng, b"ACG", int(rng.integers(0, 30))), _seq(rng, b"ACG", int(rng.integers(0, 30)))
            o = oracle_align(NW, args, a, b)
            exp = (o["score"], o["end_i"], o["end_j"], o["start_i"], o["start_j"], o["ops"])
            assert ends_free_model(NW, args, a, b, WHOLE, 0) == exp, (args, a, b)


def _brute(algo, args, a, b, fe):
    """The best global score over the trimmed substrings the flags allow: a1 * a2 == 0,
    (m - b1) * (n - b2) == 0, a trim only where its flag is set."""
    m, n = len(a), len(b)
    best = None
    for a1, a2 in itertools.product(range(m + 1) if fe & SEQ1_BEGIN else [0], range(n + 1) if fe & SEQ2_BEGIN else [0]):
        if a1 * a2:
            continue
        for b1, b2 in itertools.product(range(a1, m + 1) if fe & SEQ1_END else [m], range(a2, n + 1) if fe & SEQ2_END else [n]):
            if (m - b1) * (n - b2):
                continue
            s = oracle_align(algo, args, a[a1:b1], b[a2:b2])["score"]
            best = s if best is None else max(best, s)
    return best


def _border_costs(algo, args):
    """Entering a border costs nothing positive: gap <= 0 (linear), gap_open + gap_extend <= 0 (affine).
    Only then is the brute force the ends-free DP: with a positive border term a trimmed global alignment
    collects k * gap > 0 on a border the flags did not free, where the DP's free border holds 0 and its
    end cell is chosen among the candidates alone -- the two answer different questions."""
    g, _, _, go, ge, _ = scoring_fields(args)
    return go + ge <= 0 if algo == GLOBAL_GOTOH else g <= 0


REGIME = [(NW, s) for s in REGIME_LINEAR] + [(GLOBAL_GOTOH, s) for s in REGIME_AFFINE_BANDED]
# the regime scorings outside the rule of _border_costs: the model and _brute disagree under exactly
# these six and under no other (test_brute_force_exclusion_is_exactly_these_six)
NOT_THE_BRUTE_FORCE = [(NW, (1, 1, -1)), (NW, (1, -1, -1)), (NW, (2, 1, -3)), (NW, (1, 2)), (NW, (1, 2, -1, False)),
                       (GLOBAL_GOTOH, (2, -1, 1, -1, True))]
# One scoring inside the rule is not compared either, for another reason.  The oracle that scores the
# trimmed substrings puts the reference's X = Y = -10000 on the borders of each *trimmed* matrix; the
# header's DP has that constant on the borders of the untrimmed matrix alone.  Without mismatches and
# with gap terms past the constant (one opened gap costs -11000), a pair with no common symbol is all
# gaps and the constant wins cells in both -- different cells.  b"CCC" / b"AA" with SEQ1_BEGIN: the DP
# gives -16000 (all of Seq1 trimmed, gap_open + 2 gap_extend), the trim to b"C" scores -15000 through the
# trimmed matrix's own X(0, 2) = -10000.  3 of this scoring's 80 cases differ; with mismatches allowed,
# (-6000, -5000, 1, -1, True), a diagonal always beats the constant on pairs this short and all 80 agree.
BORDER_CONSTANT_IN_THE_TRIMS = (GLOBAL_GOTOH, (-6000, -5000, 1, -1, False))


def _regime_pairs(fe, k):
    """Five pairs per (flag set, scoring): two of the fixed edge shapes and three random ones <= 6 long."""
    return _pairs(1000 * fe + k, 7, b"AC", 6)[2:]


@pytest.mark.parametrize("fe", range(16))
def test_score_is_the_best_trimmed_global_score(fe):
    """Also under every regime scoring (util.REGIME_LINEAR, REGIME_AFFINE_BANDED) where entering a border
    costs nothing positive (_border_costs).  Outside that rule the brute force is not the ends-free DP and
    the model is right to differ: checked over 16 flag sets x 5 pairs per scoring, the model and _brute
    disagree under exactly the six scorings of NOT_THE_BRUTE_FORCE among those the rule excludes and under
    none it admits but BORDER_CONSTANT_IN_THE_TRIMS (see there).  Those seven are skipped here and
    asserted to disagree in test_brute_force_exclusion_is_exactly_these_six."""
    for algo, scorings in ((NW, LINEAR[:3]), (GLOBAL_GOTOH, AFFINE[:3])):
        for k, args in enumerate(scorings):
            for a, b in _pairs(100 * fe + k, 10, b"AC" if k else b"ACG"):
                got = ends_free_model(algo, args, a, b, WHOLE, fe)
                assert got[0] == _brute(algo, args, a, b, fe), (algo, args, a, b, fe, got)
    for k, (algo, args) in enumerate(REGIME):
        if (algo, args) in NOT_THE_BRUTE_FORCE or (algo, args) == BORDER_CONSTANT_IN_THE_TRIMS:
            continue
        for a, b in _regime_pairs(fe, k):
            got = ends_free_model(algo, args, a, b, WHOLE, fe)
            assert got[0] == _brute(algo, args, a, b, fe), (algo, args, a, b, fe, got)


def test_brute_force_exclusion_is_exactly_these_six():
    """The six skipped scorings are the ones the rule excludes, no more and no fewer, and under each of
    them -- and under the one left out for the oracle's border constant, which the rule admits -- the model
    and the brute force do disagree on the inputs the others agree on."""
    assert [s for s in REGIME if not _border_costs(*s)] == NOT_THE_BRUTE_FORCE
    assert _border_costs(*BORDER_CONSTANT_IN_THE_TRIMS) and BORDER_CONSTANT_IN_THE_TRIMS in REGIME
    for algo, args in NOT_THE_BRUTE_FORCE + [BORDER_CONSTANT_IN_THE_TRIMS]:
        k = REGIME.index((algo, args))
        differ = sum(ends_free_model(algo, args, a, b, WHOLE, fe)[0] != _brute(algo, args, a, b, fe)
                     for fe in range(16) for a, b in _regime_pairs(fe, k))
        assert differ, (algo, args)


@pytest.mark.parametrize("fe", range(16))
def test_ops_rescore_to_the_score(fe):
    """The ops between (start) and (end) add up to the score (free borders start from 0), and the walk
    ends on a border the flags free, or at (0, 0).  (Affine: scorings with gap_open <= 0 only.  With
    gap_open > 0 the recurrence itself scores a run of k gap symbols as k gaps of one, which a rescoring
    by maximal runs does not.)"""
    rng = np.random.default_rng(fe)
    for algo, scorings in ((NW, LINEAR), (GLOBAL_GOTOH, [a for a in AFFINE if a[0] <= 0])):
        for args in scorings:
            for _ in range(12):
                a, b = _seq(rng, b"ACG", int(rng.integers(0, 40))), _seq(rng, b"ACG", int(rng.integers(0, 40)))
                w = int(rng.integers(0, 10))
                score, ei, ej, si, sj, ops = ends_free_model(algo, args, a, b, w, fe)
                if algo == NW:
                    res = np.array([(len(ops),)], dtype=[("nops", "<i4")])
                    packed = np.frombuffer(ops + b"\0", dtype=np.uint8)
                    assert linear_rescore(args, res, packed, ZERO, ZERO)[0] == score
                else:
                    assert affine_rescore(args, ops) == score
                assert si == 0 or sj == 0
                assert si == 0 or fe & SEQ1_BEGIN
                assert sj == 0 or fe & SEQ2_BEGIN
                assert (ei, ej) == (len(a), len(b)) or (ej == len(b) and fe & SEQ1_END) or (ei == len(a) and fe & SEQ2_END)
                assert ei - si == sum(c in b"MSU" for c in ops) and ej - sj == sum(c in b"MSL" for c in ops)
