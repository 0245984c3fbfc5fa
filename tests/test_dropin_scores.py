"""GPU: the score-only extensions of the C++ drop-in headers (include/seqalib/): getScores() on
SmithWatermanSA / NeedlemanWunschSA / LocalGotohSA / GlobalGotohSA / HirschbergSA and getEndCells()
on the two local classes.

tests/cpp/dropin_scores compares them with getScore() / getEndCell() collected from getAlignment()
pair by pair, for std::string, std::vector<int> with a lambda match and a batch with more than 256
distinct symbols, and prints one "ok ..." line per check.  It is built here with its own g++
command line (the drop-in headers need no HIP compiler)."""
import os
import subprocess

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "seqalib_amd", "lib")


@pytest.fixture(scope="module")
def binary():
    exe = os.path.join(CPP, "dropin_scores")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(CPP, "dropin_scores.cpp"), "-L" + LIBDIR, "-lseqalib_hip",
                           "-Wl,-rpath," + LIBDIR, "-pthread"])
    return exe


def run(binary, env=None):
    p = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    lines = p.stdout.strip().split("\n")
    bad = [ln for ln in lines if not ln.startswith("ok ")]
    assert p.returncode == 0 and not bad, (p.returncode, bad, p.stderr[-2000:])
    return lines


def test_get_scores_and_end_cells(binary, engine):
    lines = run(binary)
    # 3 container kinds x (5 classes x 2 score checks + 2 local classes x 2 cell checks)
    assert len(lines) == 3 * (5 * 2 + 2 * 2), lines
    for kind in ("string", "vector<int> lambda", "vector<int> wide"):
        for cls in ("SmithWatermanSA", "NeedlemanWunschSA", "LocalGotohSA", "GlobalGotohSA", "HirschbergSA"):
            assert f"ok {kind} {cls} getScores" in lines
        for cls in ("SmithWatermanSA", "LocalGotohSA"):
            assert f"ok {kind} {cls} getEndCells" in lines


def test_get_scores_over_two_contexts(binary, engine):
    """SEQALIB_DEVICES=0,0: the batches go through sa_multi_score_batch."""
    run(binary, env=dict(os.environ, SEQALIB_DEVICES="0,0"))
