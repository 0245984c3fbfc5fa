"""GPU: the seeded extensions of the C++ drop-in headers (include/seqalib/): getAlignments(pairs, diags,
band, freeEnds) and getScores(pairs, diags, band, freeEnds) on NeedlemanWunschSA, HirschbergSA and
GlobalGotohSA.

tests/cpp/dropin_seeded aligns std::string pairs with each class at band 6, each pair round its seed
diagonal, under the fit, overlap, all-free and no-free flag sets and prints the inputs, the seeds, the
three rows of every alignment and the scores; here the Python classes' getSeededAlignments /
getSeededScores must give the same strings and numbers.  The program also checks that freeEnds > 15, a
diags of another size than pairs, a band with no legal begin and substitution scoring throw.  It prints
"ok ..." lines for those and is built here with its own g++ command line."""
import os
import subprocess

import pytest

import seqalib_amd as sa
from util import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "seqalib_amd", "lib")
BAND = 6
NPAIRS = {12: 3, 9: 2, 15: 7, 0: 3}   # free_ends: the pairs of tests/cpp/dropin_seeded.cpp's case
# the classes and scorings of tests/cpp/dropin_seeded.cpp
CLASSES = {"NeedlemanWunschSA": (sa.NeedlemanWunschSA, (-2, 2, -3)), "HirschbergSA": (sa.HirschbergSA, (-2, 2, -3)),
           "GlobalGotohSA": (sa.GlobalGotohSA, (-3, -1, 2, -3))}


@pytest.fixture(scope="module")
def output():
    exe = os.path.join(CPP, "dropin_seeded")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(CPP, "dropin_seeded.cpp"), "-L" + LIBDIR, "-lseqalib_hip",
                           "-Wl,-rpath," + LIBDIR, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.rstrip("\n").split("\n")


def _value(line, tag):
    assert line.startswith(tag + " [") and line.endswith("]"), line
    return line[len(tag) + 2:-1]


def test_seeded_dropin(output, engine):
    lines = output
    bad = [ln for ln in lines if ln.startswith("FAIL")]
    assert not bad, bad
    pairs, diags, scores = {}, {}, {}
    k = 0
    while k < len(lines):
        w = lines[k].split(" ")
        if w[0] == "pair":
            key = (w[1], int(w[2]), int(w[3]))
            diags[key] = int(w[4])
            pairs[key] = tuple(_value(lines[k + 1 + t], tag) for t, tag in enumerate(("s1", "s2", "r0", "bars", "r1")))
            k += 6
            continue
        if w[0] == "scores":
            scores[w[1], int(w[2])] = [int(x) for x in w[3:]]
        k += 1
    assert len(pairs) == len(CLASSES) * sum(NPAIRS.values()) and len(scores) == len(CLASSES) * len(NPAIRS)
    for cls, (pycls, args) in CLASSES.items():
        al = pycls(sa.ScoringSystem(*args))
        for fe, count in NPAIRS.items():
            batch = [pairs[cls, fe, p][:2] for p in range(count)]
            seeds = [diags[cls, fe, p] for p in range(count)]
            want = al.getSeededAlignments(batch, seeds, BAND, fe)
            for p in range(count):
                assert pairs[cls, fe, p][2:] == want[p].rows(), (cls, fe, p)
            assert scores[cls, fe] == al.getSeededScores(batch, seeds, BAND, fe), (cls, fe)
            assert f"ok {cls} {fe} getScore() is the last pair's" in lines
        for what in ("freeEnds 16 throws", "a diags of another size throws", "a band with no legal begin throws"):
            assert f"ok {cls} {what}" in lines
    # the fit found its read inside the window: free Seq2 symbols on both sides of the core
    r0 = pairs["NeedlemanWunschSA", 12, 0][2]
    assert r0.startswith("-" * 30) and r0.endswith("-" * 30)
    for cls in ("NeedlemanWunschSA", "GlobalGotohSA"):
        assert f"ok {cls} substitution scoring with a seeded band throws" in lines
