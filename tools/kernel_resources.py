#!/usr/bin/env python3
"""Register and scratch use of every fill_kernel, fill_so2_kernel and banded (affine) fill kernel instantiation
of a translation unit, from the compiler's own resource-usage remarks (no GPU needed).

    tools/kernel_resources.py seqalib_amd/csrc/sa_fill_sw_score.hip [more units ...] > table.txt
    tools/kernel_resources.py --parse remarks.txt ...      # remarks captured earlier

One line per kernel: algorithm, R, match flavour, ALLOW, KEYED, plan (one workgroup per pair /
SPLIT), VGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD), LDS bytes.  Exits 1 if any
kernel uses scratch -- the two-pairs-per-wave fills (fill_so2_kernel: algorithm, R, cell, column table)
excepted: theirs holds unit-prologue state outside the chunk loop (tools/issue_model.py prices the
loop)."""
import re
import subprocess
import sys

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--offload-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null"]
NAME = re.compile(r"Function Name: _ZN2sa11fill_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E")
FIELD = re.compile(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)")
# the banded fills: band_sweep_kernel<BandFill | BandAffineFill<algorithm, BandMode, R, L, match mode, REC>>
BANDED = re.compile(r"Function Name: _ZN2sa\d+_GLOBAL__N_117band_sweep_kernelINS\d+_(?:8BandFill|14BandAffineFill)"
                    r"ILi(\d+)ELNS_8BandModeE(\d)ELi(\d+)ELi(\d+)ELi(\d)ELb(\d)E")
# sa_banded_affine_extend.hip alone keeps the fills it had before the shared sweep (its header says why):
# banded_affine_fill_kernel<LOCAL, R, L, match mode | kMatchExtBit, REC>
AFFINE_EXT = re.compile(r"Function Name: _ZN2sa\d+_GLOBAL__N_125banded_affine_fill_kernelILb0ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E")
MATCH_EXT_BIT = 32
SO2 = re.compile(r"Function Name: _ZN2sa15fill_so2_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E")
CELL = ["i16 6-op", "f16 5-op", "f16 4-op"]
ALG = ["SW", "NW", "LocalGotoh", "GlobalGotoh"]
# BandMode (sa_internal.h): 0 the corridor, then the ends-free, seeded, extension and device-planned seeded
# fills (sa_banded[_affine]_{free,seeded,extend,seeded_dev}.hip), which are NW's and GlobalGotoh's
MODE = [None, {1: "NW free", 3: "GGotoh free"}, {1: "NW seeded", 3: "GGotoh seeded"}, {1: "NW extend", 3: "GGotoh extend"},
        {1: "NW planned", 3: "GGotoh planned"}]
MM = ["eq", "lut", "bits", "sub"]


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
        m = BANDED.search(line)
        if m:   # the banded fills: algorithm (SA_SW .. SA_GLOBAL_GOTOH), mode, R, L, match mode, REC
            cur = {"banded": tuple(int(x) for x in m.groups())}
            rows.append(cur)
            continue
        m = AFFINE_EXT.search(line)
        if m:   # GlobalGotoh (3), extension (mode 3), R, L, match mode, REC
            g = tuple(int(x) for x in m.groups())
            cur = {"banded": (3, 3, g[0], g[1], g[2] & ~MATCH_EXT_BIT, g[3])}
            rows.append(cur)
            continue
        m = SO2.search(line)
        if m:   # the two-pairs-per-wave fills (sa_fill_so2.hip): algorithm, R, FK, TAB
            cur = {"so2": tuple(int(x) for x in m.groups())}
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
    banded = sorted((r for r in rows if "banded" in r), key=lambda r: r["banded"])
    so2 = sorted((r for r in rows if "so2" in r), key=lambda r: r["so2"])
    rows = [r for r in rows if "args" in r]
    rows.sort(key=lambda r: r["args"])
    if so2:
        print(f"{'so2':<5}{'R':>3} {'cell':<9}{'table':>6}{'VGPRs':>6}{'AGPRs':>6}{'SGPRs':>6}{'scratch':>8}{'waves':>6}{'LDS':>7}")
        for r in so2:
            alg, R, fk, tab = r["so2"]
            print(f"{ALG[alg]:<5}{R:>3} {CELL[fk]:<9}{'LDS' if tab else 'DPP':>6}{r['VGPRs']:>6}{r.get('AGPRs', 0):>6}{r['TotalSGPRs']:>6}"
                  f"{r['ScratchSize']:>8}{r['Occupancy']:>6}{r['LDS']:>7}")
        print(f"# {len(so2)} two-pairs-per-wave kernels")
        if not rows and not banded:
            return 0
    if banded:
        wide = 14 if any(r["banded"][1] >= 2 for r in banded) else 8
        print(f"{'banded':<{wide}}{'R':>3}{'L':>4} {'match':<5}{'records':>8}{'VGPRs':>6}{'AGPRs':>6}{'SGPRs':>6}{'scratch':>8}{'waves':>6}{'LDS':>7}")
        bad_banded = 0
        for r in banded:
            alg, mode, R, L, lut, rec = r["banded"]
            print(f"{MODE[mode][alg] if mode else ALG[alg]:<{wide}}{R:>3}{L:>4} {MM[lut]:<5}{rec:>8}{r['VGPRs']:>6}{r.get('AGPRs', 0):>6}{r['TotalSGPRs']:>6}{r['ScratchSize']:>8}"
                  f"{r['Occupancy']:>6}{r['LDS']:>7}")
            bad_banded += r["ScratchSize"] != 0
        print(f"# {len(banded)} banded kernels, {bad_banded} with scratch")
        if not rows:
            return 1 if bad_banded else 0
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
    return 1 if bad or (banded and bad_banded) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
