#!/usr/bin/env python3
"""Register and scratch use of every fill_kernel instantiation of a translation unit, from the
compiler's own resource-usage remarks (no GPU needed).

    tools/kernel_resources.py seqalib_amd/csrc/sa_fill_sw_score.hip [more units ...] > table.txt
    tools/kernel_resources.py --parse remarks.txt ...      # remarks captured earlier

One line per kernel: algorithm, R, match flavour, ALLOW, KEYED, plan (one workgroup per pair /
SPLIT), VGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD), LDS bytes.  Exits 1 if any
kernel uses scratch."""
import re
import subprocess
import sys

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--offload-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null"]
NAME = re.compile(r"Function Name: _ZN2sa11fill_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")
FIELD = re.compile(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)")
ALG = ["SW", "NW", "LocalGotoh", "GlobalGotoh"]
MM = ["eq", "lut", "bits"]


def remarks(unit):
    p = subprocess.run([HIPCC] + FLAGS + [unit], capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr[-4000:])
    return p.stderr


def parse(text):
    rows, cur = [], None
    for line in text.splitlines():
        m = NAME.search(line)
        if m:
            cur = {"args": tuple(int(x) for x in m.groups())}
            rows.append(cur)
            continue
        if "Function Name:" in line:
            cur = None
            continue
        f = FIELD.search(line)
        if f and cur is not None:
            cur[f.group(1).split(" ")[0]] = int(f.group(2))
    return rows


def main(argv):
    parse_only = argv[:1] == ["--parse"]
    files = argv[1:] if parse_only else argv
    rows = []
    for f in files:
        rows += parse(open(f).read() if parse_only else remarks(f))
    rows.sort(key=lambda r: r["args"])
    print(f"{'algorithm':<12}{'R':>3} {'match':<5}{'allow':>6}{'keyed':>6} {'plan':<6}{'norec':>6}{'VGPRs':>6}{'SGPRs':>6}"
          f"{'scratch':>8}{'waves':>6}{'LDS':>7}")
    bad = 0
    for r in rows:
        alg, R, mm, allow, keyed, t16, cmax, split, so, norec = r["args"]
        if t16:
            continue
        print(f"{ALG[alg]:<12}{R:>3} {MM[mm]:<5}{allow:>6}{keyed:>6} {'SPLIT' if split else 'pair':<6}{norec:>6}"
              f"{r['VGPRs']:>6}{r['TotalSGPRs']:>6}{r['ScratchSize']:>8}{r['Occupancy']:>6}{r['LDS']:>7}")
        bad += r["ScratchSize"] != 0
    print(f"# {len(rows)} kernels, {bad} with scratch")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
