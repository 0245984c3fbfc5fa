"""GPU: the extension doors of the C++ drop-in headers (include/seqalib/): getExtensions(pairs, band, xdrop),
getExtensionScores and getExtensionEndCells on NeedlemanWunschSA, HirschbergSA and GlobalGotohSA.

tests/cpp/dropin_extend extends a small batch of std::string pairs with each class at band 6 under xdrop 8
and SA_XDROP_OFF and prints the inputs, the three rows of every alignment, the scores and the end cells;
here the Python classes' getExtensionAlignments / getExtensionScores / getExtensionEndCells must give the
same strings and numbers.  The program also checks that xdrop = -2 and substitution scoring throw.  It
prints "ok ..." lines for those and is built here with its own g++ command line."""
import os
import subprocess

import pytest

import seqalib_amd as sa
from util import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "seqalib_amd", "lib")
BAND, NPAIRS, XDROPS = 6, 5, (8, sa.SA_XDROP_OFF)
# the classes and scorings of tests/cpp/dropin_extend.cpp
CLASSES = {"NeedlemanWunschSA": (sa.NeedlemanWunschSA, (-2, 1, -3)), "HirschbergSA": (sa.HirschbergSA, (-2, 1, -3)),
           "GlobalGotohSA": (sa.GlobalGotohSA, (-4, -1, 1, -3))}


@pytest.fixture(scope="module")
def output():
    exe = os.path.join(CPP, "dropin_extend")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(CPP, "dropin_extend.cpp"), "-L" + LIBDIR, "-lseqalib_hip",
                           "-Wl,-rpath," + LIBDIR, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.rstrip("\n").split("\n")


def _value(line, tag):
    assert line.startswith(tag + " [") and line.endswith("]"), line
    return line[len(tag) + 2:-1]


def test_extend_dropin(output, engine):
    lines = output
    bad = [ln for ln in lines if ln.startswith("FAIL")]
    assert not bad, bad
    pairs, scores, ends = {}, {}, {}
    k = 0
    while k < len(lines):
        w = lines[k].split(" ")
        if w[0] == "pair":
            pairs[w[1], int(w[2]), int(w[3])] = tuple(_value(lines[k + 1 + t], tag) for t, tag in enumerate(("s1", "s2", "r0", "bars", "r1")))
            k += 6
            continue
        if w[0] == "scores":
            scores[w[1], int(w[2])] = [int(x) for x in w[3:]]
        if w[0] == "ends":
            v = [int(x) for x in w[3:]]
            ends[w[1], int(w[2])] = list(zip(v[0::2], v[1::2]))
        k += 1
    assert len(pairs) == len(CLASSES) * len(XDROPS) * NPAIRS and len(scores) == len(ends) == len(CLASSES) * len(XDROPS)
    for cls, (pycls, args) in CLASSES.items():
        al = pycls(sa.ScoringSystem(*args))
        for xdrop in XDROPS:
            batch = [pairs[cls, xdrop, p][:2] for p in range(NPAIRS)]
            want = al.getExtensionAlignments(batch, BAND, xdrop)
            for p in range(NPAIRS):
                assert pairs[cls, xdrop, p][2:] == want[p].rows(), (cls, xdrop, p)
            assert scores[cls, xdrop] == al.getExtensionScores(batch, BAND, xdrop), (cls, xdrop)
            assert ends[cls, xdrop] == al.getExtensionEndCells(batch, BAND, xdrop), (cls, xdrop)
            assert f"ok {cls} {xdrop} getScore() is the last pair's" in lines
        assert f"ok {cls} xdrop -2 throws" in lines and f"ok {cls} an empty batch gives nothing" in lines
        # the diverging pair stops under xdrop 8 and keeps its unextended tails in the printed rows
        drops = al.getExtensionDropped([pairs[cls, 8, p][:2] for p in range(NPAIRS)], BAND, 8)
        assert drops[0] and not drops[3] and not drops[4]
        s1, s2, r0, _, r1 = pairs[cls, 8, 0]
        assert r0.replace("-", "") == s1 and r1.replace("-", "") == s2 and r0.endswith("-" * 20)
    for cls in ("NeedlemanWunschSA", "GlobalGotohSA"):
        assert f"ok {cls} substitution scoring with an extension throws" in lines
