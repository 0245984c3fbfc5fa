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
