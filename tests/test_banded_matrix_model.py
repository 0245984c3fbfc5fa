"""CPU: pins tests/banded_matrix_model.py, the model the GPU tests of the banded matrix calls are
checked against.  (a) With the two-valued table S = match / mismatch it is banded_model
(test_gpu_banded.py) and banded_affine_model at narrow bands; (b) at a whole-matrix band it is
submat_model.model_align for asymmetric random tables; (c) a narrow band never scores above the whole
matrix."""
import numpy as np
import pytest

from banded_affine_model import banded_affine_model
from banded_matrix_model import GLOBAL_GOTOH, LOCAL_GOTOH, NW, SW, banded_matrix_model
from submat_model import model_align
from test_gpu_banded import banded_model
from util import REGIME_AFFINE_BANDED, REGIME_LINEAR, scoring_fields

FIELDS = ("score", "end_i", "end_j", "start_i", "start_j", "ops")
ABC = np.frombuffer(b"ABC", dtype=np.uint8)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def model_pairs(alphabet, seed, count=24, top=40):
    """Pairs of up to `top` symbols, empty ones included: unrelated ones and related ones (a with a few
    symbols redrawn, dropped or doubled)."""
    rng = np.random.default_rng(seed)
    k = len(alphabet)
    pairs = [(b"", b""), (b"", alphabet[:3].tobytes()), (alphabet[:3].tobytes(), b""),
             (alphabet[:1].tobytes(), alphabet[:1].tobytes()), (alphabet[:1].tobytes(), alphabet[1:2].tobytes())]
    while len(pairs) < count:
        a = alphabet[rng.integers(0, k, int(rng.integers(0, top + 1)))].tobytes()
        if len(pairs) % 2:
            b = alphabet[rng.integers(0, k, int(rng.integers(0, top + 1)))].tobytes()
        else:
            out = bytearray()
            for c in a:
                r = int(rng.integers(0, 10))
                if r == 0:
                    out.append(alphabet[rng.integers(0, k)])
                elif r == 1:
                    out += bytes([c, c])
                elif r != 2:
                    out.append(c)
            b = bytes(out[:top])
        pairs.append((a, b))
    return pairs


def random_table(alphabet, seed):
    """An asymmetric 256 x 256 table with entries in [-8, 8] on the alphabet (0 elsewhere)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((256, 256), dtype=np.int16)
    t[np.ix_(alphabet, alphabet)] = rng.integers(-8, 9, (len(alphabet), len(alphabet)))
    assert (t != t.T).any()
    return t


PAIRS3 = model_pairs(ABC, 21)
PAIRS20 = model_pairs(AA, 22)


# ------------------------------------------------- (a) two-valued table = the banded models
@pytest.mark.parametrize("algo", [SW, NW])
@pytest.mark.parametrize("args", [(-1, 1, -1), (-2, 2, -3), (-3, 5, 0)])
def test_two_valued_table_is_the_linear_banded_model(algo, args):
    g, ma, mi = args
    S = lambda a, b: ma if a == b else mi
    for p, (a, b) in enumerate(PAIRS3 + PAIRS20):
        for w in (0, 1, 3, 16):
            assert banded_matrix_model(algo, g, S, a, b, w) == banded_model(algo, args, a, b, w), (p, w)


@pytest.mark.parametrize("algo", [LOCAL_GOTOH, GLOBAL_GOTOH])
@pytest.mark.parametrize("args", [(-3, -1, 1, -1), (0, -1, 1, -1), (-4, 0, 2, -1), (2, -2, 1, -1)])
def test_two_valued_table_is_the_affine_banded_model(algo, args):
    go, ge, ma, mi = args
    S = lambda a, b: ma if a == b else mi
    for p, (a, b) in enumerate(PAIRS3 + PAIRS20):
        for w in (0, 1, 3, 16):
            assert banded_matrix_model(algo, (go, ge), S, a, b, w) == banded_affine_model(algo, args, a, b, w), (p, w)


def regime_pairs():
    """Nine pairs: the empty and one-symbol shapes, two over ABC and two over the twenty letters."""
    return PAIRS3[:5] + [PAIRS3[8], PAIRS3[13], PAIRS20[10], PAIRS20[15]]


def regime_scorings(algo):
    """The regime scorings, gap_extend <= 0, with mismatches allowed (a table scores every cell): one that
    forbids them is taken with its mismatch value allowed, the two-argument ones (no mismatch value) are
    left out -- their gap terms, 0 and 1, come with other scorings."""
    out = []
    for s in (REGIME_LINEAR if algo in (SW, NW) else REGIME_AFFINE_BANDED):
        if len(s) >= 3 and s[:3 if algo in (SW, NW) else 4] not in out:
            out.append(s[:3 if algo in (SW, NW) else 4])
    return out


def test_regime_gap_terms():
    assert {s[0] for s in regime_scorings(NW)} == {-4097, -4096, -700, -3, -2, -1, 0, 1, 2}
    assert {s[:2] for s in regime_scorings(GLOBAL_GOTOH)} == {(-6000, -5000), (-2049, -513), (-2048, -512), (-3, -5), (-3, -1),
                                                             (-3, 0), (0, -2), (0, -1), (0, 0), (1, -1), (2, -1)}


@pytest.mark.parametrize("algo", [SW, NW, LOCAL_GOTOH, GLOBAL_GOTOH])
def test_two_valued_table_is_the_banded_model_under_the_regime_scorings(algo):
    """The degenerate table S[a][b] = (a == b ? match : mismatch) gives the model without a table under
    every regime scoring that allows mismatches: gap terms 0, > 0 and in the thousands, match <= 0,
    mismatch >= match; and no assertion of either model's walk fires."""
    for args in regime_scorings(algo):
        g, ma, mi, go, ge, _ = scoring_fields(args)
        S = lambda a, b: ma if a == b else mi
        for p, (a, b) in enumerate(regime_pairs()):
            for w in (0, 1, 3, 100):
                if algo in (SW, NW):
                    assert banded_matrix_model(algo, g, S, a, b, w) == banded_model(algo, args, a, b, w), (args, p, w)
                else:
                    assert banded_matrix_model(algo, (go, ge), S, a, b, w) == banded_affine_model(algo, args, a, b, w), (args, p, w)


def test_labels_follow_the_match_function():
    S = random_table(AA, 5)
    match = lambda a, b: a % 3 == b % 3
    for algo, gaps in [(SW, -2), (NW, -2), (LOCAL_GOTOH, (-3, -1)), (GLOBAL_GOTOH, (-3, -1))]:
        for a, b in PAIRS20:
            plain = banded_matrix_model(algo, gaps, S, a, b, 3)
            named = banded_matrix_model(algo, gaps, S, a, b, 3, match)
            assert plain[:5] == named[:5]
            assert plain[5].replace(b"M", b"S") == named[5].replace(b"M", b"S")
            i, j = named[1], named[2]
            for c in named[5]:   # traceback order: from the end cell back
                if c in b"MS":
                    assert (c == ord("M")) == match(a[i - 1], b[j - 1])
                    i, j = i - 1, j - 1
                elif c == ord("U"):
                    i -= 1
                else:
                    j -= 1


# ----------------------------------- (b), (c) whole-matrix band = submat_model; narrow <= whole
LINEAR_GAPS = [-1, -2, -5]
AFFINE_GAPS = [(go, ge) for go in (-11, -4, -1, 0, 3) for ge in (0, -1, -2)]
TABLES = [("abc", ABC, PAIRS3, 31), ("aa", AA, PAIRS20, 32)]


@pytest.mark.parametrize("name", ["abc", "aa"])
@pytest.mark.parametrize("algo", [SW, NW, LOCAL_GOTOH, GLOBAL_GOTOH])
def test_whole_matrix_band_is_the_matrix_model_and_bounds_narrow_bands(name, algo):
    _, alphabet, pairs, seed = next(t for t in TABLES if t[0] == name)
    S = random_table(alphabet, seed)
    for gaps in (LINEAR_GAPS if algo in (SW, NW) else AFFINE_GAPS):
        for p, (a, b) in enumerate(pairs):
            want = model_align(algo, gaps, S, a, b)
            assert not want["diverged"], (gaps, p)
            full = banded_matrix_model(algo, gaps, S, a, b, max(len(a), len(b)))
            assert full == tuple(want[f] for f in FIELDS), (gaps, p, len(a), len(b))
            assert banded_matrix_model(algo, gaps, S, a, b, 4096) == full
            for w in (0, 1, 3, 16):
                assert banded_matrix_model(algo, gaps, S, a, b, w)[0] <= full[0], (gaps, p, w)
