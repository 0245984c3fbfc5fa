"""GPU: the ends-free extensions of the C++ drop-in headers (include/seqalib/): getAlignments(pairs, band,
freeEnds) and getScores(pairs, band, freeEnds) on NeedlemanWunschSA, HirschbergSA and GlobalGotohSA.

tests/cpp/dropin_ends_free aligns std::string pairs with each class at band 8 under the fit, overlap,
all-free and no-free flag sets and prints the inputs, the three rows of every alignment and the scores;
here the Python classes' getEndsFreeAlignments / getEndsFreeScores must give the same strings and
numbers.  The program also checks that freeEnds = 0 is getAlignments(pairs, band), and that freeEnds >
15 and substitution scoring with free ends throw.  It prints "ok ..." lines for those and is built here
with its own g++ command line."""
import os
import subprocess

import pytest

import seqalib_amd as sa
from util import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "seqalib_amd", "lib")
BAND = 8
NPAIRS = 7
FLAGS = (12, 9, 15, 0)
# the classes and scorings of tests/cpp/dropin_ends_free.cpp
CLASSES = {"NeedlemanWunschSA": (sa.NeedlemanWunschSA, (-2, 2, -3)), "HirschbergSA": (sa.HirschbergSA, (-2, 2, -3)),
           "GlobalGotohSA": (sa.GlobalGotohSA, (-3, -1, 2, -3))}


@pytest.fixture(scope="module")
def output():
    exe = os.path.join(CPP, "dropin_ends_free")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(CPP, "dropin_ends_free.cpp"), "-L" + LIBDIR, "-lseqalib_hip",
                           "-Wl,-rpath," + LIBDIR, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.rstrip("\n").split("\n")


def _value(line, tag):
    assert line.startswith(tag + " [") and line.endswith("]"), line
    return line[len(tag) + 2:-1]


def test_ends_free_dropin(output, engine):
    lines = output
    bad = [ln for ln in lines if ln.startswith("FAIL")]
    assert not bad, bad
    pairs, scores = {}, {}
    k = 0
    while k < len(lines):
        w = lines[k].split(" ")
        if w[0] == "pair":
            pairs[w[1], int(w[2]), int(w[3])] = tuple(_value(lines[k + 1 + t], tag) for t, tag in enumerate(("s1", "s2", "r0", "bars", "r1")))
            k += 6
            continue
        if w[0] == "scores":
            scores[w[1], int(w[2])] = [int(x) for x in w[3:]]
        k += 1
    assert len(pairs) == len(CLASSES) * len(FLAGS) * NPAIRS and len(scores) == len(CLASSES) * len(FLAGS)
    for cls, (pycls, args) in CLASSES.items():
        al = pycls(sa.ScoringSystem(*args))
        for fe in FLAGS:
            batch = [pairs[cls, fe, p][:2] for p in range(NPAIRS)]
            want = al.getEndsFreeAlignments(batch, BAND, fe)
            for p in range(NPAIRS):
                assert pairs[cls, fe, p][2:] == want[p].rows(), (cls, fe, p)
            assert scores[cls, fe] == al.getEndsFreeScores(batch, BAND, fe), (cls, fe)
            assert f"ok {cls} {fe} getScore() is the last pair's" in lines
        assert f"ok {cls} freeEnds 16 throws" in lines
    # the fit found its read inside the window: free Seq2 symbols on both sides of the core
    r0 = pairs["NeedlemanWunschSA", 12, 0][2]
    assert r0.startswith("-" * 30) and r0.endswith("-" * 30)
    for cls in ("NeedlemanWunschSA", "GlobalGotohSA"):
        assert f"ok {cls} freeEnds 0 equals getAlignments(pairs, band)" in lines
        assert f"ok {cls} substitution scoring with free ends throws" in lines
