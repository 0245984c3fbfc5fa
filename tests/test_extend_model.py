"""CPU: tests/extend_model.py, the restatement the GPU tests of the banded extension calls compare with,
is pinned before it is trusted: by a brute force over the full matrix (a band that holds all of it, the
drop off), by the header's equivalences (a) -- through tests/seeded_model.py -- and (b), and the numpy
fill by the dict model; first on four ordinary scorings per algorithm, then on the scorings outside
gap < 0 < match, mismatch < 0 that tests/test_gpu_banded_extend_regimes.py runs on the GPU
(util.REGIME_LINEAR under NW, util.REGIME_AFFINE_BANDED under GlobalGotoh)."""
import numpy as np

from extend_model import (FLAG_DROPPED, GLOBAL_GOTOH, NW, XDROP_OFF, XDROP_PERIOD, extend_band, extend_fill_np,
                          extend_model)
from seeded_model import seeded_model
from util import REGIME_AFFINE_BANDED, REGIME_LINEAR, named_lut, scoring_fields

LINEAR = [(-2, 1, -3), (-1, 1, -1), (0, 1, -1), (-1, 2, -1, False)]
AFFINE = [(-4, -1, 1, -3), (-3, -1, 1, -1), (0, 0, 1, -1), (-3, -1, 1, -1, False)]
XDROPS = [XDROP_OFF, 0, 2, 5, 1000]
REGIME = [(NW, s) for s in REGIME_LINEAR] + [(GLOBAL_GOTOH, s) for s in REGIME_AFFINE_BANDED]
assert len(REGIME) == 53
NEG = -10 ** 9
# what the regime cases below are counted to do: the model gives 61 pairs that end at (0, 0), 50 dropped
# results in (a), 47 cases that stop at xdrop = 0 in (b) and 50 dropped results in the numpy comparison for
# their seeds; the asserted counts are those, rounded down
REGIME_AT_ORIGIN, REGIME_A_DROPPED, REGIME_B_STOPPED, REGIME_NP_DROPPED = 50, 40, 40, 40


def _seq(rng, letters, n):
    return bytes(rng.choice(list(letters), n).tolist()) if n else b""


def _scorings():
    return [(NW, s) for s in LINEAR] + [(GLOBAL_GOTOH, s) for s in AFFINE]


def _related(rng, n, rate):
    """(a, b): b is a with about `rate` of its symbols substituted, inserted before or deleted."""
    a = _seq(rng, b"ACGT", n)
    b = bytearray()
    for ch in a:
        r = rng.random()
        if r < rate / 2:
            b.append(int(rng.choice(list(b"ACGT"))))
        elif r < 3 * rate / 4:
            b.append(int(rng.choice(list(b"ACGT"))))
            b.append(ch)
        elif r < rate:
            continue
        else:
            b.append(ch)
    return a, bytes(b)


def _brute(algo, args, a, b):
    """(score, end_i, end_j) over the whole matrix: the last row-major maximum over (0, 0) and the interior."""
    g, ma, mi, go, ge, allow = scoring_fields(args)
    m, n = len(a), len(b)
    M = [[NEG] * (n + 1) for _ in range(m + 1)]
    X = [[NEG] * (n + 1) for _ in range(m + 1)]
    Y = [[NEG] * (n + 1) for _ in range(m + 1)]
    affine = algo == GLOBAL_GOTOH
    for i in range(m + 1):
        for j in range(n + 1):
            if i == 0 or j == 0:
                k = i + j
                M[i][j] = 0 if k == 0 else (go + k * ge if affine else k * g)
                X[i][j] = Y[i][j] = -10000
                continue
            same = a[i - 1] == b[j - 1]
            d = M[i - 1][j - 1] + (ma if same else mi) if (same or allow) else NEG
            if affine:
                X[i][j] = max(M[i - 1][j] + go + ge, X[i - 1][j] + ge)
                Y[i][j] = max(M[i][j - 1] + go + ge, Y[i][j - 1] + ge)
                M[i][j] = max(d, X[i][j], Y[i][j])
            else:
                M[i][j] = max(d, M[i - 1][j] + g, M[i][j - 1] + g)
    best, end = 0, (0, 0)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if M[i][j] >= best:
                best, end = M[i][j], (i, j)
    return best, end[0], end[1]


def test_a_whole_matrix_band_without_the_drop_is_the_brute_force():
    rng = np.random.default_rng(1)
    for n_case in range(240):
        algo, args = _scorings()[n_case % 8]
        a, b = _seq(rng, b"ACG", int(rng.integers(0, 13))), _seq(rng, b"ACG", int(rng.integers(0, 13)))
        w = max(len(a), len(b), 1) + int(rng.integers(0, 3))
        got = extend_model(algo, args, a, b, w, XDROP_OFF)
        assert got[:3] == _brute(algo, args, a, b), (algo, args, a, b)
        assert got[3:5] == (0, 0) and got[6:] == (False, None)
        assert got[0] >= 0


def test_a_whole_matrix_band_is_the_brute_force_on_the_regime_scorings():
    rng = np.random.default_rng(11)
    at_origin = 0
    for n_case in range(530):
        algo, args = REGIME[n_case % 53]
        a, b = _seq(rng, b"ACG", int(rng.integers(0, 13))), _seq(rng, b"ACG", int(rng.integers(0, 13)))
        w = max(len(a), len(b), 1) + int(rng.integers(0, 3))
        got = extend_model(algo, args, a, b, w, XDROP_OFF)
        assert got[:3] == _brute(algo, args, a, b), (algo, args, a, b)
        assert got[3:5] == (0, 0) and got[6:] == (False, None)
        assert got[0] >= 0   # ((0, 0) is a candidate)
        g, ma, mi, go, ge, allow = scoring_fields(args)
        terms = (ma, mi if allow else 0, go + ge if algo == GLOBAL_GOTOH else g, ge)
        # match <= 0, mismatch <= 0, gap <= 0, not all zero: no alignment of non-empty sequences gains
        if a and b and max(terms) <= 0 and min(terms) < 0:
            assert got[0] == 0
            at_origin += got[1:3] == (0, 0) and got[5] == b""
    print("regime brute force: pairs that end at (0, 0) with no ops:", at_origin)
    assert at_origin >= REGIME_AT_ORIGIN


def _unit(args):
    """What an xdrop of this scoring is a multiple of: its largest term in magnitude."""
    g, ma, mi, go, ge, allow = scoring_fields(args)
    return max(1, abs(g), abs(ma), abs(mi) if allow else 0, abs(go) + abs(ge))


def _cases(seed, count, max_len, scorings=None):
    """(algo, args, a, b, w, xdrop): the scorings rotate through the cases; under `scorings` (the regime list)
    the xdrop values are multiples of the scoring's largest term."""
    rng = np.random.default_rng(seed)
    for n_case in range(count):
        algo, args = (scorings or _scorings())[n_case % len(scorings or _scorings())]
        if n_case % 3 == 0:
            a, b = _related(rng, int(rng.integers(0, max_len + 1)), 0.15)
            a, b = a + _seq(rng, b"ACGT", int(rng.integers(0, 30))), b + _seq(rng, b"ACGT", int(rng.integers(0, 30)))
        else:
            a, b = _seq(rng, b"AC", int(rng.integers(0, max_len + 1))), _seq(rng, b"AC", int(rng.integers(0, max_len + 1)))
        w = int(rng.integers(0 if scoring_fields(args)[5] else 1, 9))
        xdrop = XDROPS[int(rng.integers(0, len(XDROPS)))]
        yield algo, args, a, b, w, xdrop * _unit(args) if scorings and xdrop > 0 else xdrop


def _check_prefixes(cases):
    dropped = 0
    for algo, args, a, b, w, xdrop in cases:
        score, ei, ej, si, sj, ops, drop, stop = extend_model(algo, args, a, b, w, xdrop)
        lo, hi, tend = extend_band(len(a), len(b), w)
        assert lo <= ej - ei <= hi and (si, sj) == (0, 0)
        assert (ei, ej) == (0, 0) or (ei >= 1 and ej >= 1)
        assert drop == (stop is not None) and (stop is None or (stop % XDROP_PERIOD == XDROP_PERIOD - 1 and stop < tend))
        assert not drop or ei + ej - lo <= stop
        assert (score, ei, ej, 0, 0, ops) == seeded_model(algo, args, a[:ei], b[:ej], 0, w, 0), (algo, args, a, b, w, xdrop)
        dropped += drop
    return dropped


def test_a_result_is_the_seeded_alignment_of_its_prefixes():
    """Equivalence (a), dropped or not."""
    assert _check_prefixes(_cases(2, 400, 60)) >= 40   # (the cases do exercise the rule)


def test_a_regime_result_is_the_seeded_alignment_of_its_prefixes():
    assert _check_prefixes(_cases(12, 530, 60, REGIME)) >= REGIME_A_DROPPED


def _check_monotone(cases, unit):
    """How many cases stop at xdrop = 0."""
    moved = 0
    for algo, args, a, b, w, _ in cases:
        u = unit(args)
        off = extend_model(algo, args, a, b, w, XDROP_OFF)
        scores = [extend_model(algo, args, a, b, w, x * u)[0] for x in (0, 1, 2, 3, 5, 8, 13, 40, 1000)]
        assert scores == sorted(scores) and scores[-1] == off[0], (algo, args, a, b, w)
        big = extend_model(algo, args, a, b, w, 10 ** 6 * u)
        assert big == off
        moved += extend_model(algo, args, a, b, w, 0)[6]
    return moved


def test_the_score_rises_with_xdrop_up_to_the_unstopped_score():
    """Equivalence (b)."""
    assert _check_monotone(_cases(3, 120, 60), lambda args: 1) >= 25


def test_the_regime_score_rises_with_xdrop_up_to_the_unstopped_score():
    """Equivalence (b), the xdrop values scaled to the scoring."""
    assert _check_monotone(_cases(13, 212, 60, REGIME), _unit) >= REGIME_B_STOPPED


def test_the_trace_holds_the_checkpoints_the_rule_reads():
    rng = np.random.default_rng(4)
    a, b = _related(rng, 40, 0.05)
    a, b = a + _seq(rng, b"ACGT", 120), b + _seq(rng, b"ACGT", 120)
    trace = []
    stop = extend_model(NW, (-2, 1, -3), a, b, 8, 10, trace=trace)[7]
    assert stop is not None and trace[-1][0] == stop and trace[-1][1] - trace[-1][2] > 10
    assert all(t % XDROP_PERIOD == XDROP_PERIOD - 1 and best - recent <= 10 for t, best, recent in trace[:-1])


def _check_numpy(cases):
    purine = named_lut("purine")
    n_drop = 0
    for n_case, (algo, args, a, b, w, xdrop) in enumerate(cases):
        lut = purine if n_case % 4 == 1 else None
        t_model, t_np = [], []
        want = extend_model(algo, args, a, b, w, xdrop, lut, trace=t_model)
        assert extend_fill_np(algo, args, a, b, w, xdrop, lut, trace=t_np) == want[:3] + want[6:], (algo, args, a, b, w, xdrop)
        assert t_np == t_model, (algo, args, a, b, w, xdrop)   # (every checkpoint's step, best and recent)
        n_drop += want[6]
    return n_drop


def test_the_numpy_fill_is_the_dict_model():
    assert _check_numpy(_cases(5, 400, 70)) >= 40


def test_the_numpy_fill_is_the_dict_model_on_the_regime_scorings():
    assert _check_numpy(_cases(15, 530, 70, REGIME)) >= REGIME_NP_DROPPED


def test_the_flag_is_the_headers():
    assert FLAG_DROPPED == 32 and XDROP_PERIOD == 16 and XDROP_OFF == -1
