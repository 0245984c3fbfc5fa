"""CPU: the per-pair function the device planner of the device-resident banded extension calls runs
(seqalib_amd/csrc/sa_band_plan.h) gives every pair the variant and record words the host layer gives it, the
bound the host provisions from (max_m, max_n, band, algorithm) holds every pair inside it, and the chunk
arithmetic keeps a chunk inside the workspace limit (tests/cpp/band_plan_test.cpp, a stand-alone host program
built here, once plain and once with the address and undefined-behaviour sanitizers).  No GPU is touched."""
import os
import subprocess

import pytest

from util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "cpp", "band_plan_test.cpp")


@pytest.mark.parametrize("flags", [[], ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-fsanitize=address,undefined",
                                        "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_band_plan_matches_the_host_layer(tmp_path, flags):
    exe = str(tmp_path / "band_plan_test")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-x", "hip", *flags, "-o", exe, SRC], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "ok"
