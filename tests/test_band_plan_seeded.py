"""CPU: what the device-resident seeded band calls rest on (seqalib_amd/csrc/sa_band_plan.h).  The bound the host
provisions from (max_m, max_n, band, algorithm) alone holds every pair inside it at every seed diagonal, the
per-pair function the planner kernel runs gives the host layer's variant and record words, and the legality
function shared by the host call and the planner agrees with the header's rule restated over the band's cells
(tests/cpp/band_plan_seeded_test.cpp, a stand-alone host program built here, once plain and once with the address
and undefined-behaviour sanitizers).  No GPU is touched."""
import os
import subprocess

import pytest

from util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "cpp", "band_plan_seeded_test.cpp")


@pytest.mark.parametrize("flags", [[], ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-fsanitize=address,undefined",
                                        "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_seeded_bound_holds_every_pair_and_diagonal(tmp_path, flags):
    exe = str(tmp_path / "band_plan_seeded_test")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-x", "hip", *flags, "-o", exe, SRC], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "ok"
