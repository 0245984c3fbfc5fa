"""CPU: the banded calls' grouping of pairs into launches (seqalib_amd/csrc/sa_band_group.h) follows the
rule its comment states -- narrowest variant or one step up, merges only where allowed, longest first,
record offsets, the workspace budget -- on random batches and hand-worked ones
(tests/cpp/band_group_test.cpp, a stand-alone host program built here).  No GPU is touched."""
import os
import subprocess

from util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_band_grouping_follows_its_rule(tmp_path):
    exe = str(tmp_path / "band_group_test")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-x", "hip", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "band_group_test.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "ok"
