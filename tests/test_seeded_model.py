"""CPU: tests/seeded_model.py, the restatement the GPU tests of the seeded banded calls compare with, is
pinned before it is trusted: by the header's equivalences (a), (b), (c) against tests/ends_free_model.py,
by the reversal symmetry of the NW score, by its op stream rescoring to its score, and by a brute force
over in-band paths that knows nothing of borders."""
import functools

import numpy as np
import pytest

from banded_affine_model import affine_rescore
from ends_free_model import ends_free_model
from seeded_model import (GLOBAL_GOTOH, NW, SEQ1_BEGIN, SEQ1_END, SEQ2_BEGIN, SEQ2_END, seeded_band, seeded_legal,
                          seeded_model)
from util import REGIME_AFFINE_BANDED, REGIME_LINEAR, linear_rescore, scoring_fields

LINEAR = [(-1, 1, -1), (-2, 2, -3), (0, 1, -1), (-1, -1, -2)]          # gap <= 0
AFFINE = [(-3, -1, 1, -1), (-2, 0, 2, -3), (1, -1, 1, -1), (0, 0, 1, -2)]   # extend <= 0, open + extend <= 0
ZERO = np.zeros(2, dtype=np.uint64)   # the offsets of a one-pair batch whose ops start at 0
NEG = -10 ** 9


def _seq(rng, letters, n):
    return bytes(rng.choice(list(letters), n).tolist()) if n else b""


def _legal_cases(seed, count, max_len, max_w):
    """Random (a, b, k, w, free_ends), drawn until the legality rule admits them."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        a, b = _seq(rng, b"ACG", int(rng.integers(0, max_len + 1))), _seq(rng, b"ACG", int(rng.integers(0, max_len + 1)))
        k, w, fe = int(rng.integers(-len(a), len(b) + 1)), int(rng.integers(0, max_w + 1)), int(rng.integers(0, 16))
        if seeded_legal(len(a), len(b), k, w, fe) == (True, True):
            out.append((a, b, k, w, fe))
    return out


def _scorings():
    return [(NW, s) for s in LINEAR] + [(GLOBAL_GOTOH, s) for s in AFFINE]


def test_legality_rule_leaves_no_dead_end_and_the_walk_stays_in_the_band():
    """The model asserts both itself (an empty candidate set raises in max())."""
    for n_case, (a, b, k, w, fe) in enumerate(_legal_cases(1, 400, 14, 6)):
        algo, args = _scorings()[n_case % 8]
        score, ei, ej, si, sj, ops = seeded_model(algo, args, a, b, k, w, fe)
        lo, hi = seeded_band(len(a), len(b), k, w)
        assert lo <= ej - ei <= hi
        assert si == 0 or sj == 0
        assert (si, sj) == (0, 0) or (si == 0 and fe & SEQ2_BEGIN) or (sj == 0 and fe & SEQ1_BEGIN)
        assert (ei, ej) == (len(a), len(b)) or (ej == len(b) and fe & SEQ1_END) or (ei == len(a) and fe & SEQ2_END)
        assert ei - si == sum(c in b"MSU" for c in ops) and ej - sj == sum(c in b"MSL" for c in ops)


def test_a_whole_matrix_band_is_the_ends_free_model():
    """Equivalence (a): w >= m + n."""
    rng = np.random.default_rng(2)
    for n_case in range(160):
        algo, args = _scorings()[n_case % 8]
        a, b = _seq(rng, b"ACG", int(rng.integers(0, 15))), _seq(rng, b"ACG", int(rng.integers(0, 15)))
        k, fe = int(rng.integers(-len(a), len(b) + 1)), int(rng.integers(0, 16))
        w = len(a) + len(b) + int(rng.integers(0, 3))
        assert seeded_model(algo, args, a, b, k, w, fe) == ends_free_model(algo, args, a, b, w, fe), (algo, args, a, b, k, fe)


def test_the_corridor_seed_is_the_ends_free_model():
    """Equivalence (b): n - m even, diag = (n - m) / 2, w' = w + |n - m| / 2."""
    rng = np.random.default_rng(3)
    done = 0
    while done < 240:
        a, b = _seq(rng, b"ACG", int(rng.integers(0, 15))), _seq(rng, b"ACG", int(rng.integers(0, 15)))
        d = len(b) - len(a)
        if d % 2:
            continue
        algo, args = _scorings()[done % 8]
        w, fe = int(rng.integers(0, 7)), int(rng.integers(0, 16))
        got = seeded_model(algo, args, a, b, d // 2, w + abs(d) // 2, fe)
        assert got == ends_free_model(algo, args, a, b, w, fe), (algo, args, a, b, w, fe)
        done += 1


REGIME = [(NW, s) for s in REGIME_LINEAR] + [(GLOBAL_GOTOH, s) for s in REGIME_AFFINE_BANDED]


@pytest.mark.parametrize("algo,args", REGIME, ids=lambda v: "_".join(str(int(x)) for x in v) if isinstance(v, tuple) else str(v))
def test_the_equivalences_hold_under_the_regime_scorings(algo, args):
    """Equivalences (a) and (b) under every scoring of util.REGIME_LINEAR / REGIME_AFFINE_BANDED: gap
    terms 0 and > 0, in the thousands, match <= 0, mismatch >= match.  (Without mismatches a band of one
    diagonal has no candidate, so w' >= 1 there.)"""
    rng = np.random.default_rng(7)
    wmin = 0 if scoring_fields(args)[5] else 1
    done = 0
    while done < 24:
        a, b = _seq(rng, b"ACG", int(rng.integers(0, 15))), _seq(rng, b"ACG", int(rng.integers(0, 15)))
        d = len(b) - len(a)
        fe = int(rng.integers(0, 16))
        whole = len(a) + len(b) + 1
        k = int(rng.integers(-len(a), len(b) + 1))
        assert seeded_model(algo, args, a, b, k, whole, fe) == ends_free_model(algo, args, a, b, whole, fe), (a, b, k, fe)
        if d % 2 == 0:
            w = int(rng.integers(wmin, 7))
            got = seeded_model(algo, args, a, b, d // 2, w + abs(d) // 2, fe)
            assert got == ends_free_model(algo, args, a, b, w, fe), (a, b, w, fe)
            done += 1


def test_the_score_does_not_fall_as_the_band_grows():
    """Equivalence (c), for a fixed diag."""
    for n_case, (a, b, k, w, fe) in enumerate(_legal_cases(4, 240, 14, 5)):
        algo, args = _scorings()[n_case % 8]
        scores = [seeded_model(algo, args, a, b, k, ww, fe)[0] for ww in range(w, w + 4)]
        assert scores == sorted(scores), (algo, args, a, b, k, w, fe, scores)


def _swap_ends(fe):
    return ((fe & SEQ1_BEGIN) << 1) | ((fe & SEQ1_END) >> 1) | ((fe & SEQ2_BEGIN) << 1) | ((fe & SEQ2_END) >> 1)


def test_nw_score_is_invariant_under_reversal():
    """Both sequences reversed, BEGIN <-> END, k -> (n - m) - k: the same band, cells and paths, mirrored."""
    for n_case, (a, b, k, w, fe) in enumerate(_legal_cases(5, 320, 14, 6)):
        args = LINEAR[n_case % 4]
        rk = (len(b) - len(a)) - k
        assert seeded_legal(len(a), len(b), rk, w, _swap_ends(fe)) == (True, True)
        assert seeded_model(NW, args, a, b, k, w, fe)[0] == seeded_model(NW, args, a[::-1], b[::-1], rk, w, _swap_ends(fe))[0]


def test_ops_rescore_to_the_score():
    """The ops between (start) and (end) add up to the score (free borders start from 0).  Affine:
    scorings with gap_open <= 0 only, as in test_ends_free_model.py."""
    cases = _legal_cases(6, 480, 40, 8)
    for n_case, (a, b, k, w, fe) in enumerate(cases):
        algo, args = [(NW, s) for s in LINEAR][n_case % 4] if n_case % 2 else [(GLOBAL_GOTOH, s) for s in AFFINE if s[0] <= 0][n_case % 3]
        score, ei, ej, si, sj, ops = seeded_model(algo, args, a, b, k, w, fe)
        if algo == NW:
            res = np.array([(len(ops),)], dtype=[("nops", "<i4")])
            packed = np.frombuffer(ops + b"\0", dtype=np.uint8)
            assert linear_rescore(args, res, packed, ZERO, ZERO)[0] == score
        else:
            assert affine_rescore(args, ops) == score


def _brute(algo, args, a, b, k, w, fe):
    """The best score of a path of diagonal / up / left moves that stays in the band, from a legal begin
    cell ((0, 0); with SEQ2_BEGIN any (0, j); with SEQ1_BEGIN any (i, 0)) to a legal end cell ((m, n);
    with SEQ1_END any (i, n); with SEQ2_END any (m, j)).  Linear: every gap symbol costs gap.  Affine: a
    maximal run of k gap symbols of one kind costs gap_open + k * gap_extend.  A recursion over
    (i, j, last move) with no notion of a border."""
    g, ma, mi, go, ge, allow = scoring_fields(args)
    affine = algo == GLOBAL_GOTOH
    m, n = len(a), len(b)
    lo, hi = seeded_band(m, n, k, w)

    def cell(i, j):
        return 0 <= i <= m and 0 <= j <= n and lo <= j - i <= hi

    def begin(i, j):
        return (i, j) == (0, 0) or (i == 0 and fe & SEQ2_BEGIN) or (j == 0 and fe & SEQ1_BEGIN)

    @functools.lru_cache(maxsize=None)
    def best(i, j, last):   # last: 0 none (the path begins here), 1 diagonal, 2 up, 3 left
        if not cell(i, j):
            return NEG
        if last == 0:
            return 0 if begin(i, j) else NEG
        if last == 1:
            if i == 0 or j == 0 or not (a[i - 1] == b[j - 1] or allow):
                return NEG
            return max(best(i - 1, j - 1, x) for x in range(4)) + (ma if a[i - 1] == b[j - 1] else mi)
        pi, pj = (i - 1, j) if last == 2 else (i, j - 1)
        if not affine:
            return max(best(pi, pj, x) for x in range(4)) + g
        return max(best(pi, pj, last) + ge, max(best(pi, pj, x) for x in range(4) if x != last) + go + ge)

    ends = {(m, n)}
    if fe & SEQ1_END:
        ends |= {(i, n) for i in range(m + 1)}
    if fe & SEQ2_END:
        ends |= {(m, j) for j in range(n + 1)}
    return max(best(i, j, x) for (i, j) in ends for x in range(4))


@pytest.mark.parametrize("fe", range(16))
def test_score_is_the_best_in_band_path(fe):
    """gap <= 0 (gap_open <= 0, gap_extend <= 0), so that a free border's 0 is the best way to reach it."""
    rng = np.random.default_rng(100 + fe)
    scorings = [(NW, s) for s in LINEAR] + [(GLOBAL_GOTOH, s) for s in AFFINE if s[0] <= 0]
    done = 0
    while done < 70:
        a, b = _seq(rng, b"AC", int(rng.integers(0, 9))), _seq(rng, b"AC", int(rng.integers(0, 9)))
        k, w = int(rng.integers(-len(a), len(b) + 1)), int(rng.integers(0, 5))
        if seeded_legal(len(a), len(b), k, w, fe) != (True, True):
            continue
        algo, args = scorings[done % 7]
        got = seeded_model(algo, args, a, b, k, w, fe)[0]
        exp = _brute(algo, args, a, b, k, w, fe)
        assert exp > NEG // 2 and got == exp, (algo, args, a, b, k, w, fe, got, exp)
        done += 1
