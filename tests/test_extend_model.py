"""CPU: tests/extend_model.py, the restatement the GPU tests of the banded extension calls compare with,
is pinned before it is trusted: by a brute force over the full matrix (a band that holds all of it, the
drop off), by the header's equivalences (a) -- through tests/seeded_model.py -- and (b), and the numpy
fill by the dict model."""
import numpy as np

from extend_model import (FLAG_DROPPED, GLOBAL_GOTOH, NW, XDROP_OFF, XDROP_PERIOD, extend_band, extend_fill_np,
                          extend_model)
from seeded_model import seeded_model
from util import named_lut, scoring_fields

LINEAR = [(-2, 1, -3), (-1, 1, -1), (0, 1, -1), (-1, 2, -1, False)]
AFFINE = [(-4, -1, 1, -3), (-3, -1, 1, -1), (0, 0, 1, -1), (-3, -1, 1, -1, False)]
XDROPS = [XDROP_OFF, 0, 2, 5, 1000]
NEG = -10 ** 9


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


def _cases(seed, count, max_len):
    rng = np.random.default_rng(seed)
    for n_case in range(count):
        algo, args = _scorings()[n_case % 8]
        if n_case % 3 == 0:
            a, b = _related(rng, int(rng.integers(0, max_len + 1)), 0.15)
            a, b = a + _seq(rng, b"ACGT", int(rng.integers(0, 30))), b + _seq(rng, b"ACGT", int(rng.integers(0, 30)))
        else:
            a, b = _seq(rng, b"AC", int(rng.integers(0, max_len + 1))), _seq(rng, b"AC", int(rng.integers(0, max_len + 1)))
        w = int(rng.integers(0 if scoring_fields(args)[5] else 1, 9))
        yield algo, args, a, b, w, XDROPS[int(rng.integers(0, len(XDROPS)))]


def test_a_result_is_the_seeded_alignment_of_its_prefixes():
    """Equivalence (a), dropped or not."""
    dropped = 0
    for algo, args, a, b, w, xdrop in _cases(2, 400, 60):
        score, ei, ej, si, sj, ops, drop, stop = extend_model(algo, args, a, b, w, xdrop)
        lo, hi, tend = extend_band(len(a), len(b), w)
        assert lo <= ej - ei <= hi and (si, sj) == (0, 0)
        assert (ei, ej) == (0, 0) or (ei >= 1 and ej >= 1)
        assert drop == (stop is not None) and (stop is None or (stop % XDROP_PERIOD == XDROP_PERIOD - 1 and stop < tend))
        assert not drop or ei + ej - lo <= stop
        assert (score, ei, ej, 0, 0, ops) == seeded_model(algo, args, a[:ei], b[:ej], 0, w, 0), (algo, args, a, b, w, xdrop)
        dropped += drop
    assert dropped >= 40   # (the cases do exercise the rule)


def test_the_score_rises_with_xdrop_up_to_the_unstopped_score():
    """Equivalence (b)."""
    for algo, args, a, b, w, _ in _cases(3, 120, 60):
        off = extend_model(algo, args, a, b, w, XDROP_OFF)
        scores = [extend_model(algo, args, a, b, w, x)[0] for x in (0, 1, 2, 3, 5, 8, 13, 40, 1000)]
        assert scores == sorted(scores) and scores[-1] == off[0], (algo, args, a, b, w)
        big = extend_model(algo, args, a, b, w, 10 ** 6)
        assert big == off


def test_the_trace_holds_the_checkpoints_the_rule_reads():
    rng = np.random.default_rng(4)
    a, b = _related(rng, 40, 0.05)
    a, b = a + _seq(rng, b"ACGT", 120), b + _seq(rng, b"ACGT", 120)
    trace = []
    stop = extend_model(NW, (-2, 1, -3), a, b, 8, 10, trace=trace)[7]
    assert stop is not None and trace[-1][0] == stop and trace[-1][1] - trace[-1][2] > 10
    assert all(t % XDROP_PERIOD == XDROP_PERIOD - 1 and best - recent <= 10 for t, best, recent in trace[:-1])


def test_the_numpy_fill_is_the_dict_model():
    purine = named_lut("purine")
    n_drop = 0
    for n_case, (algo, args, a, b, w, xdrop) in enumerate(_cases(5, 400, 70)):
        lut = purine if n_case % 4 == 1 else None
        want = extend_model(algo, args, a, b, w, xdrop, lut)
        assert extend_fill_np(algo, args, a, b, w, xdrop, lut) == want[:3] + want[6:], (algo, args, a, b, w, xdrop)
        n_drop += want[6]
    assert n_drop >= 40


def test_the_flag_is_the_headers():
    assert FLAG_DROPPED == 32 and XDROP_PERIOD == 16 and XDROP_OFF == -1
