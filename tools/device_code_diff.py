#!/usr/bin/env python3
"""Compare the gfx950 device code of translation units between two trees of this project, kernel by kernel
(no GPU needed).

    tools/device_code_diff.py OLD_TREE NEW_TREE seqalib_amd/csrc/sa_banded.hip [more units ...]
    tools/device_code_diff.py --plain OLD_TREE NEW_TREE seqalib_amd/csrc/sa_fill_sw.hip ...

Each unit is compiled in both trees as DESIGN.md 2.17 does (the Makefile's HIPFLAGS, --offload-device-only -S,
from the tree's root, lines containing __hip_cuid_ dropped).  --plain compares the two remainders as they are.
Otherwise the assembly is split per function -- its code, its .amdhsa_kernel block and its metadata entry --
and the functions of the two sides are paired by what they are, not by what they are called: a banded kernel
by its decoded template arguments (family, fill or walk, algorithm, band mode, R, L, match mode, REC / LUT),
in the parent's spelling (kBandAlg* algorithm values, kMatch*Bit match-mode bits, one walk kernel per mode)
or this tree's (BandMode), every other function by its demangled name.  Inside a function every symbol of
namespace sa is replaced by a placeholder numbered by first appearance, and the compiler's per-file label
numbers are dropped, so a renamed kernel with the same code compares equal.

Per unit: functions paired, identical, differing; for a differing pair the line counts and VGPRs / SGPRs /
scratch / LDS / occupancy of both sides.  A function without a partner is an error: the set of
instantiations must neither grow nor shrink.  Exits 1 on an unpaired function or a failed --plain
comparison, 0 otherwise (differing kernels are reported, not judged).

--keep DIR keeps the assembly as DIR/{old,new}/UNIT.s and reuses the old side's files on the next run."""
import argparse
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or sys.exit("needs llvm-cxxfilt or c++filt")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result",
         "--offload-device-only", "-S", "-o", "-"]

SYMBOL = re.compile(r"_ZZ?NK?2sa\w+")
LABEL = re.compile(r"(BB|Lfunc_begin|Lfunc_end|Ltmp)\d+")   # .LBB12_3, "Header=BB12_3" in a comment, .Lfunc_end12
BEGIN = re.compile(r"; -- Begin function (\S+)")
META_NAME = re.compile(r"^\s+\.name:\s+(\S+)")
OCCUPANCY = re.compile(r"^; Occupancy: (\d+)", re.M)
DIRECTIVE = {"VGPRs": r"\.amdhsa_next_free_vgpr (\d+)", "AGPR offset": r"\.amdhsa_accum_offset (\d+)",
             "SGPRs": r"\.amdhsa_next_free_sgpr (\d+)", "scratch": r"\.amdhsa_private_segment_fixed_size (\d+)",
             "LDS": r"\.amdhsa_group_segment_fixed_size (\d+)"}

# The parent's spelling of a band mode, as (algorithm value) of the linear kernels and (match-mode bits) of the
# affine fills; modes: 0 corridor, 1 ends-free, 2 seeded, 3 extension, 4 device-planned seeded.
OLD_ALG_MODE = {100: 1, 101: 2, 102: 3, 103: 4}
OLD_BITS_MODE = {0: 0, 8: 1, 8 | 16: 2, 32: 3, 8 | 16 | 64: 4}
OLD_AFFINE_WALK = {"banded_affine_free_tb_kernel": 1, "banded_affine_seeded_tb_kernel": 2,
                   "banded_affine_extend_tb_kernel": 3, "banded_affine_seeded_dev_tb_kernel": 4}
NS = r"sa::\(anonymous namespace\)::"
INT, BOOL, MODE = r"(\d+)", r"(true|false)", r"\(sa::BandMode\)(\d)"
SEP = r",\s*"


def _b(s):
    return s == "true"


def banded_key(name):
    """(family, kind, algorithm (linear) or local (affine), mode, R, L, match mode, REC or LUT) of a banded kernel, else None."""
    def m(pat):
        return re.match(r"void " + NS + pat, name)
    # this tree
    g = m(r"band_sweep_kernel<" + NS + r"BandFill<" + SEP.join([INT, MODE, INT, INT, INT, BOOL]) + ">")
    if g:
        return ("linear", "fill", int(g[1]), int(g[2]), int(g[3]), int(g[4]), int(g[5]), _b(g[6]))
    g = m(r"band_sweep_kernel<" + NS + r"BandAffineFill<" + SEP.join([INT, MODE, INT, INT, INT, BOOL]) + ">")
    if g:   # (SA_LOCAL_GOTOH = 2, SA_GLOBAL_GOTOH = 3)
        return ("affine", "fill", int(g[1] == "2"), int(g[2]), int(g[3]), int(g[4]), int(g[5]), _b(g[6]))
    g = m(r"banded_tb_kernel<" + SEP.join([MODE, INT, BOOL]) + ">")
    if g:
        return ("linear", "walk", int(g[2]), int(g[1]), 0, 0, 0, _b(g[3]))
    g = m(r"banded_affine_tb_kernel<" + SEP.join([MODE, BOOL, BOOL]) + ">")
    if g:
        return ("affine", "walk", int(_b(g[2])), int(g[1]), 0, 0, 0, _b(g[3]))
    # the parent
    g = m(r"banded_fill_kernel<" + SEP.join([INT, INT, INT, INT, BOOL]) + ">")
    if g:
        alg = int(g[1])
        return ("linear", "fill", 1 if alg in OLD_ALG_MODE else alg, OLD_ALG_MODE.get(alg, 0), int(g[2]), int(g[3]), int(g[4]), _b(g[5]))
    g = m(r"banded_affine_fill_kernel<" + SEP.join([BOOL, INT, INT, INT, BOOL]) + ">")
    if g:
        mmf = int(g[4])
        return ("affine", "fill", int(_b(g[1])), OLD_BITS_MODE[mmf & ~7], int(g[2]), int(g[3]), mmf & 7, _b(g[5]))
    g = m(r"banded_tb_kernel<" + SEP.join([INT, BOOL]) + ">")
    if g:
        alg = int(g[1])
        return ("linear", "walk", 1 if alg in OLD_ALG_MODE else alg, OLD_ALG_MODE.get(alg, 0), 0, 0, 0, _b(g[2]))
    g = m(r"banded_affine_tb_kernel<" + SEP.join([BOOL, BOOL]) + ">")
    if g:
        return ("affine", "walk", int(_b(g[1])), 0, 0, 0, 0, _b(g[2]))
    g = m(r"(banded_affine_\w+_tb_kernel)<" + BOOL + ">")
    if g and g[1] in OLD_AFFINE_WALK:
        return ("affine", "walk", 0, OLD_AFFINE_WALK[g[1]], 0, 0, 0, _b(g[2]))
    return None


def compile_unit(tree, unit):
    p = subprocess.run([HIPCC] + FLAGS + [unit], cwd=tree, capture_output=True, text=True)
    if p.returncode:
        sys.exit(f"{tree}: {unit}: hipcc failed\n{p.stderr[-4000:]}")
    return "".join(l + "\n" for l in p.stdout.splitlines() if "__hip_cuid_" not in l)


def assembly(tree, unit, keep, side):
    path = os.path.join(keep, side, os.path.basename(unit) + ".s") if keep else None
    if path and side == "old" and os.path.exists(path):
        return open(path).read()
    text = compile_unit(tree, unit)
    if path:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return text


def demangle(names):
    if not names:
        return {}
    out = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def split(text):
    """{mangled name: [lines]}: a function's code with its .amdhsa_kernel block, then its metadata entry."""
    lines = text.splitlines()
    meta_at = next((k for k, l in enumerate(lines) if l.strip() == ".amdgpu_metadata"), len(lines))
    funcs, cur = {}, None
    for l in lines[:meta_at]:
        b = BEGIN.search(l)
        if b:
            cur = funcs.setdefault(b[1], [])
        if cur is not None:
            cur.append(l)
    entry = []
    def close():
        name = next((META_NAME.match(l)[1] for l in entry if META_NAME.match(l)), None)
        if name in funcs:
            funcs[name] += entry
    for l in lines[meta_at:]:
        if l.startswith("  - ") or not l.startswith("    "):   # a new kernel entry, or the end of the list
            close()
            entry = []
        if l.startswith("  - ") or (entry and l.startswith("    ")):
            entry.append(l)
    close()
    return funcs


def normalise(lines):
    seen = {}
    def sym(m):
        return "<sa%d>" % seen.setdefault(m[0], len(seen))
    return [LABEL.sub(r"\1#", SYMBOL.sub(sym, l)) for l in lines]


def resources(lines):
    text = "\n".join(lines)
    r = {}
    for k, pat in DIRECTIVE.items():
        g = re.search(pat, text)
        r[k] = int(g[1]) if g else 0
    g = OCCUPANCY.search(text)
    r["waves"] = int(g[1]) if g else 0
    return r


def keyed(funcs):
    names = demangle(list(funcs))
    out = {}
    for mangled, lines in funcs.items():
        key = banded_key(names[mangled]) or names[mangled]
        if key in out:
            sys.exit(f"two functions decode to {key}")
        out[key] = (names[mangled], lines)
    return out


def show(key):
    return key if isinstance(key, str) else " ".join(str(x) for x in key)


def compare(unit, old, new):
    a, b = keyed(split(old)), keyed(split(new))
    unpaired = [("old", k) for k in a if k not in b] + [("new", k) for k in b if k not in a]
    same, differing = 0, []
    for k in a:
        if k not in b:
            continue
        la, lb = normalise(a[k][1]), normalise(b[k][1])
        if la == lb:
            same += 1
        else:
            differing.append((k, len(la), len(lb), resources(a[k][1]), resources(b[k][1])))
    kernels = sum(1 for k in a if ".amdhsa_kernel" in "\n".join(a[k][1]))
    print(f"{os.path.basename(unit)}: {len(a) - sum(s == 'old' for s, _ in unpaired)} paired ({kernels} kernels old), "
          f"{same} identical, {len(differing)} differing, {len(unpaired)} unpaired; "
          f"{len(old.splitlines())} / {len(new.splitlines())} lines")
    for k, na, nb, ra, rb in differing:
        print(f"  differs: {show(k)}: {na} / {nb} lines; " + ", ".join(f"{f} {ra[f]} / {rb[f]}" for f in ra))
    for side, k in unpaired:
        print(f"  unpaired ({side}): {show(k)}")
    return len(unpaired), len(differing)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("units", nargs="+")
    ap.add_argument("--plain", action="store_true", help="compare each unit's whole assembly, unnormalised")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly here and reuse the old side's")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compilations at a time")
    args = ap.parse_args()
    jobs = [(t, u, s) for u in args.units for t, s in ((args.old_tree, "old"), (args.new_tree, "new"))]
    with ThreadPoolExecutor(args.j) as pool:
        texts = list(pool.map(lambda j: assembly(j[0], j[1], args.keep, j[2]), jobs))
    bad = differing = 0
    for n, unit in enumerate(args.units):
        old, new = texts[2 * n], texts[2 * n + 1]
        if args.plain:
            same = old == new
            print(f"{os.path.basename(unit)}: {'identical' if same else 'DIFFERENT'}, {old.count('.amdhsa_kernel ')} kernels, {len(old.splitlines())} lines")
            bad += not same
        else:
            u, d = compare(unit, old, new)
            bad += u
            differing += d
    if not args.plain:
        print(f"# {len(args.units)} units: {differing} kernels differing, {bad} unpaired")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
