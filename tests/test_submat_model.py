"""CPU: pins tests/submat_model.py.  With S(a, b) = match(a, b) ? match : mismatch the model must be the
oracle (oracle/sa_oracle.c) on score, end cell, start cell and ops, for all four algorithms -- on golden
vectors (random.jsonl, kat.jsonl, with their named match functions) and on seeded random pairs up to
80 symbols.  The oracle has no table scoring, so this equality is all that stands behind the model
the GPU tests of the matrix calls are checked against."""
import numpy as np
import pytest

from submat_model import model_align
from util import ALGOS, golden_sequences, load_golden, named_lut, oracle_align, scoring_fields

HACK_SIZES = {(314, 288), (60, 57), (61, 58)}   # LocalGotoh runs NW there (the oracle does, the model does not)
FIELDS = ("score", "end_i", "end_j", "start_i", "start_j", "ops")


def degenerate(args, lut):
    """(gaps, S, match) of the model for a ScoringSystem argument tuple with allow_mismatch."""
    g, ma, mi, go, ge, allow = scoring_fields(args)
    assert allow
    if lut is None:
        match = lambda a, b: a == b
    else:
        rows = lut.tolist()
        match = lambda a, b: rows[a][b] != 0
    S = lambda a, b: ma if match(a, b) else mi
    return g, (go, ge), S, match


def check(algo, args, a, b, lut=None):
    g, aff, S, match = degenerate(args, lut)
    want = oracle_align(algo, args, a, b, lut)
    got = model_align(algo, aff if algo >= 2 else g, S, a, b, match)
    if want["rc"] == -3:   # the reference's walk does not terminate: both must say so
        assert got["diverged"]
        return
    assert want["rc"] == 0
    assert not got["diverged"]
    for f in FIELDS:
        assert got[f] == want[f], (algo, args, len(a), len(b), f)


def golden_cases():
    out = []
    for name, cap in (("random.jsonl", 250), ("kat.jsonl", 250)):
        n = 0
        for e in load_golden(name):
            algo = ALGOS[e["algo"]]
            if algo > 3 or e["m"] * e["n"] > 6400 or not scoring_fields(e["scoring"])[5]:
                continue
            if algo == 2 and (e["m"], e["n"]) in HACK_SIZES:
                continue
            out.append(e)
            n += 1
            if n == cap:
                break
    return out


def test_model_equals_oracle_on_golden_vectors():
    cases = golden_cases()
    assert len(cases) >= 300
    assert {ALGOS[e["algo"]] for e in cases} == {0, 1, 2, 3}
    for e in cases:
        a, b = golden_sequences(e)
        check(ALGOS[e["algo"]], tuple(e["scoring"]), a, b, named_lut(e["match"]))


LINEAR = [(-1, 1, -1), (-2, 2, -3), (-3, 5, -4), (-1, 3, 0)]
AFFINE = [(-3, -1, 1, -1), (-5, -2, 4, -3), (-2, -2, 3, -2), (0, -1, 2, -1)]


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_model_equals_oracle_on_random_pairs(algo):
    rng = np.random.default_rng(500 + algo)
    alphabets = [b"ACGT", b"ACGTN", b"ACDEFGHIKLMNPQRSTVWY", b"AB"]
    for k in range(120):
        al = np.frombuffer(alphabets[k % 4], dtype=np.uint8)
        m, n = int(rng.integers(0, 81)), int(rng.integers(0, 81))
        a = al[rng.integers(0, len(al), m)].tobytes()
        if k % 3 == 0 and m:   # a related pair: long paths with gaps
            keep = rng.random(m) > 0.15
            b = bytes(c for c, kp in zip(a, keep) if kp)[:80]
        else:
            b = al[rng.integers(0, len(al), n)].tobytes()
        if algo == 2 and (len(a), len(b)) in HACK_SIZES:
            continue
        args = (AFFINE if algo >= 2 else LINEAR)[k % 4]
        lut = named_lut("nwild") if k % 4 == 1 else named_lut("purine") if k % 8 == 0 else None
        check(algo, args, a, b, lut)
