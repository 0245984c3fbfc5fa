"""GPU: the banded affine extensions of the C++ drop-in headers (include/seqalib/): getAlignments(pairs,
band) and getScores(pairs, band) on LocalGotohSA / GlobalGotohSA, getEndCells(pairs, band) on
LocalGotohSA.

tests/cpp/dropin_banded_affine checks, for std::string and for std::vector<int> with a lambda match,
that a whole-matrix band gives getAlignments(pairs) entry for entry (sizes of the LocalGotoh size hack
avoided) and that getScores(pairs, 8) gives the scores collected from getAlignments(pairs, 8); a batch
with more than 256 distinct symbols must throw, and so must a band that does not fit 32 bits.  It
prints one "ok ..." line per check and is built here with its own g++ command line."""
import os
import subprocess

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "seqalib_amd", "lib")


@pytest.fixture(scope="module")
def binary():
    exe = os.path.join(CPP, "dropin_banded_affine")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(CPP, "dropin_banded_affine.cpp"), "-L" + LIBDIR, "-lseqalib_hip",
                           "-Wl,-rpath," + LIBDIR, "-pthread"])
    return exe


def test_banded_affine_dropin(binary, engine):
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    lines = p.stdout.strip().split("\n")
    bad = [ln for ln in lines if not ln.startswith("ok ")]
    assert p.returncode == 0 and not bad, (p.returncode, bad, p.stderr[-2000:])
    for kind in ("string", "vector<int> lambda"):
        for cls in ("LocalGotohSA", "GlobalGotohSA"):
            assert f"ok {kind} {cls} whole-matrix band" in lines
            assert f"ok {kind} {cls} getScores band 8" in lines
        assert f"ok {kind} LocalGotohSA getEndCells band 8" in lines
    for cls in ("LocalGotohSA", "GlobalGotohSA"):
        assert f"ok vector<int> wide {cls} wide batch throws" in lines
        assert f"ok string {cls} huge band throws" in lines
    assert len(lines) == 2 * 5 + 2 + 2, lines
