"""GPU: setSubstitution() with a band on the C++ drop-in classes (include/seqalib/): SmithWatermanSA,
NeedlemanWunschSA, LocalGotohSA and GlobalGotohSA through sa_align_batch_banded_matrix /
sa_score_batch_banded_matrix.

tests/cpp/dropin_banded_matrix aligns std::string pairs and std::vector<int> pairs with each class: at
a whole-matrix band it compares getAlignments(pairs, band) with getAlignments(pairs) itself, entry for
entry; at band 8 it prints its inputs, scores, end cells and aligned rows, and everything is recomputed
here from the printed inputs with tests/banded_matrix_model.py.  A batch with more than 64 distinct
symbols must throw.  The program is built here with its own g++ command line (-std=c++14: the headers'
language level), as tests/test_dropin_submat.py builds its own."""
import os
import subprocess

import pytest

import seqalib_amd as sa
from banded_matrix_model import banded_matrix_model
from util import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "seqalib_amd", "lib")
BAND = 8
NPAIRS = 7
CLASSES = {"SmithWatermanSA": sa.SA_SW, "NeedlemanWunschSA": sa.SA_NW, "LocalGotohSA": sa.SA_LOCAL_GOTOH,
           "GlobalGotohSA": sa.SA_GLOBAL_GOTOH}
GAPS = {sa.SA_SW: -2, sa.SA_NW: -2, sa.SA_LOCAL_GOTOH: (-4, -1), sa.SA_GLOBAL_GOTOH: (-4, -1)}
# the score and label rules of tests/cpp/dropin_banded_matrix.cpp, and the blank of each sequence type
KINDS = {
    "string": (lambda x, y: 5 + x % 3 if x == y else (x * 7 + y * 3) % 11 - 6, lambda x, y: x == y, ord("-")),
    "vector<int>": (lambda x, y: 6 if x == y else (x * 5 + y) % 9 - 5, lambda x, y: x % 10 == y % 10, 0),
}


@pytest.fixture(scope="module")
def output():
    exe = os.path.join(CPP, "dropin_banded_matrix")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(CPP, "dropin_banded_matrix.cpp"), "-L" + LIBDIR, "-lseqalib_hip",
                           "-Wl,-rpath," + LIBDIR, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.strip().split("\n")


def test_banded_substitution_dropin(output, engine):
    lines = output
    bad = [ln for ln in lines if ln.startswith("FAIL")]
    assert not bad, bad
    pairs, scores, cells = {}, {}, {}
    k = 0
    while k < len(lines):
        w = lines[k].split(" ")
        if w[0] == "pair":
            kind, cls, p = w[1], w[2], int(w[3])
            s1 = [int(x) for x in lines[k + 1].split()[1:]]
            s2 = [int(x) for x in lines[k + 2].split()[1:]]
            rows = [tuple(int(x) for x in e.split(":")) for e in lines[k + 3].split()[1:]]
            pairs[kind, cls, p] = (s1, s2, rows)
            k += 4
            continue
        if w[0] == "scores":
            scores[w[1], w[2]] = [int(x) for x in w[3:]]
        if w[0] == "cells":
            cells[w[1], w[2]] = [tuple(int(x) for x in c.split(",")) for c in w[3:]]
        k += 1
    assert len(pairs) == 2 * 4 * NPAIRS and len(scores) == 8 and len(cells) == 4
    for (kind, cls, p), (s1, s2, rows) in sorted(pairs.items()):
        algo = CLASSES[cls]
        S, label, blank = KINDS[kind]
        score, ei, ej, si, sj, ops = banded_matrix_model(algo, GAPS[algo], S, bytes(s1), bytes(s2), BAND, label)
        want = sa.expand_ops(algo, s1, s2, sa.PairResult(score, ei, ej, si, sj, 0, ops), blank=blank)
        assert rows == [(e.first, e.second, int(e.is_match)) for e in want], (kind, cls, p)
        assert score == scores[kind, cls][p], (kind, cls, p)
        if (kind, cls) in cells:
            assert cells[kind, cls][p] == (ei, ej), (kind, cls, p)
    assert any(r[2] == 0 and r[0] != r[1] and 0 not in r[:2] for v in pairs.values() for r in v[2])   # an 'S' entry
    for kind in KINDS:
        for cls in CLASSES:
            assert f"ok {kind} {cls} whole-matrix band equals getAlignments(pairs)" in lines
            assert f"ok {kind} {cls} whole-matrix band scores" in lines
        for cls in ("SmithWatermanSA", "LocalGotohSA"):
            assert f"ok {kind} {cls} whole-matrix band end cells" in lines
    for cls in ("NeedlemanWunschSA", "LocalGotohSA"):
        assert f"ok vector<int> wide {cls} wide batch throws" in lines
