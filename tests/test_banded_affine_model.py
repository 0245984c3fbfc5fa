"""CPU: the banded affine model (tests/banded_affine_model.py) at a whole-matrix band is the oracle's
Gotoh, field for field and op for op, and a narrow band never scores above it."""
import numpy as np
import pytest

from banded_affine_model import GLOBAL, LOCAL, affine_rescore, banded_affine_model
from util import LG_HACK_SIZES, REGIME_AFFINE_BANDED, oracle_align

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SCORINGS = [(-3, -1, 1, -1), (0, -1, 1, -1), (-4, 0, 2, -1), (2, -2, 1, -1), (-3, -1, 2, -1, False)]


def model_pairs():
    rng = np.random.default_rng(7)
    pairs = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C")]
    while len(pairs) < 60:
        m = int(rng.integers(0, 61))
        a = ACGT[rng.integers(0, 4, m)].tobytes()
        if len(pairs) % 2:
            b = ACGT[rng.integers(0, 4, int(rng.integers(0, 61)))].tobytes()
        else:   # related: a with a few symbols redrawn, dropped or doubled
            out = bytearray()
            for c in a:
                r = int(rng.integers(0, 10))
                if r == 0:
                    out.append(ACGT[rng.integers(0, 4)])
                elif r == 1:
                    out += bytes([c, c])
                elif r != 2:
                    out.append(c)
            b = bytes(out[:60])
        if (len(a), len(b)) not in LG_HACK_SIZES:   # (the oracle applies the LocalGotoh size hack)
            pairs.append((a, b))
    return pairs


PAIRS = model_pairs()


def regime_pairs():
    """Ten pairs up to 90 long for the regime scorings (util.REGIME_AFFINE_BANDED): the edge shapes and
    related pairs, long enough for the -10000 border to win a cell under gap terms in the thousands."""
    rng = np.random.default_rng(17)
    pairs = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C")]
    for m, n in ((7, 9), (33, 31), (64, 70), (90, 88), (75, 12)):
        a = ACGT[rng.integers(0, 4, m)].tobytes()
        b = bytearray((a + ACGT[rng.integers(0, 4, n)].tobytes())[:n])
        for q in rng.integers(0, n, n // 5):
            b[q] = ACGT[rng.integers(0, 4)]
        pairs.append((a, bytes(b)))
    return pairs


REGIME_PAIRS = regime_pairs()


@pytest.mark.parametrize("algo", [GLOBAL, LOCAL])
@pytest.mark.parametrize("args", SCORINGS + REGIME_AFFINE_BANDED)
def test_whole_matrix_band_is_the_oracle(algo, args):
    """SCORINGS on the 60 pairs; the regime scorings (gap_open of either sign, gap_extend = 0,
    match <= 0, mismatch >= match, gap terms in the thousands) on REGIME_PAIRS."""
    pairs = PAIRS if args in SCORINGS else REGIME_PAIRS
    assert not any((len(a), len(b)) in LG_HACK_SIZES for a, b in pairs)
    for p, (a, b) in enumerate(pairs):
        o = oracle_align(algo, args, a, b)
        assert o["rc"] == 0
        want = (o["score"], o["end_i"], o["end_j"], o["start_i"], o["start_j"], o["ops"])
        for w in (max(len(a), len(b)), 4096):
            assert banded_affine_model(algo, args, a, b, w) == want, (p, len(a), len(b), w)


@pytest.mark.parametrize("algo", [GLOBAL, LOCAL])
@pytest.mark.parametrize("args", SCORINGS)
def test_narrow_band_scores_at_most_the_whole_band(algo, args):
    for p, (a, b) in enumerate(PAIRS):
        full = banded_affine_model(algo, args, a, b, 4096)[0]
        for w in (0, 1, 3, 8):
            if w == 0 and len(args) == 5 and not args[4]:
                continue   # (band 0 without mismatches has no candidate: the calls reject it)
            got = banded_affine_model(algo, args, a, b, w)
            assert got[0] <= full, (p, w)
            if args[0] <= 0:   # (one open per maximal run holds only when opening costs)
                i, j = got[1] - got[3], got[2] - got[4]
                assert (sum(c in b"MSXU" for c in got[5]), sum(c in b"MSXL" for c in got[5])) == (i, j)
                if b"X" not in got[5]:
                    assert affine_rescore(args, got[5]) == got[0], (p, w)
