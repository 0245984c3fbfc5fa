"""CPU: the banded fill, walk and planner kernels' own source, run on the host under the address and
undefined-behaviour sanitizers, against the Python models.  No GPU is touched and nothing is loaded into
Python: tests/cpp/banded_emu.cpp is a stand-alone program linked against the twelve sa_banded*.hip units and
sa_band_planner.hip, each compiled as C++ through the wave shim tests/cpp/wave_emu/hip/hip_runtime.h (a wave is 64
host threads that meet at a barrier at every cross-lane operation).  The program takes the host layer's own path --
band_group, band_idx_with_diagonals, the launch_banded_* launchers, the planner's kernels -- but gives every kernel
buffers that are heap allocations of exactly the contract's size, runs every case under two poison patterns, and
reports per pair the record words of its own range that were never written.

What the GPU suite cannot see: a load or store a few words outside a pair's records lands
inside the context's workspace, and a walk that reads a word the fill never wrote usually reads the right stale
value of the previous call.  Here the first is a sanitizer report and the second a difference between the two
poison runs.

Every comparison is exact: score, end cell, start, nops, every op, flags, reserved.  The inputs are the GPU
tests' own generators, so both suites see the same bytes; what a case is there for (which variant, clipped or not,
the end cell in the sweep's last step, who stops) is asserted on the model or the geometry before the run.

$SEQALIB_EMU_BUILD_DIR keeps the objects between runs (rebuilt when a source is newer); by default the build lives
in pytest's temporary directory.
"""
import functools
import os
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import seqalib_amd as sa
from banded_affine_model import banded_affine_model
from banded_matrix_model import banded_matrix_model
from ends_free_model import ends_free_model
from extend_model import XDROP_PERIOD, extend_band, extend_fill_np, extend_model
from seeded_model import seeded_band, seeded_legal, seeded_model, seeded_steps
from test_gpu_banded import ACGT, banded_model, seq
from test_gpu_banded_extend import drop_inputs, edited, mixed_batch, variant_pairs
from test_gpu_banded_extend_regimes import (PHASE_PAIRS, PHASE_SCORING, PHASE_W, WIDE_SCORINGS, launch_order, mixed_seven,
                                            phase_batch, regime_batch)
from test_gpu_banded_seeded import legal_batch
from util import ROOT, named_lut, scoring_fields

SW, NW, LG, GG = sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH
OFF, DROPPED = sa.SA_XDROP_OFF, sa.SA_FLAG_DROPPED
INT_MAX = 2 ** 31 - 1
PURINE = named_lut("purine")
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals
CXX = os.environ.get("CXX", "g++")
CSRC = os.path.join(ROOT, "seqalib_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
SHIM = os.path.join(CPP, "wave_emu")
# longest build first (measured)
UNITS = ["sa_banded_affine", "sa_banded", "sa_banded_affine_seeded", "sa_banded_affine_free", "sa_banded_affine_extend",
         "sa_banded_affine_seeded_dev", "sa_banded_affine_sub", "sa_banded_free", "sa_banded_extend", "sa_banded_seeded",
         "sa_banded_seeded_dev", "sa_banded_sub", "sa_band_planner"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FLAGS = ["-std=c++20", "-O1", "-g", "-pthread", "-I", SHIM] + SANITIZE
# the sanitizer runtimes are linked statically: a dynamic one refuses to start unless it is the first library loaded,
# which is not the programs' to decide where something else is preloaded
LINK = ["-static-libasan", "-static-libubsan"]
JOBS = max(1, min(8, os.cpu_count() or 1))   # (never more than 16)
RUNNERS = max(1, min(4, (os.cpu_count() or 1) // 2))   # driver processes side by side: each runs 64 threads


def affine(algo):
    return algo in (LG, GG)


def variant_of(diagonals):
    return next(v for v, (R, L) in enumerate(VARIANTS) if diagonals <= 2 * R * L)


# --------------------------------------------------------------------------------------------- the build
def newer(target, sources):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(s) for s in sources)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """{"driver": path, "selftest": path}: both built with the sanitizers, the objects JOBS at a time."""
    keep = os.environ.get("SEQALIB_EMU_BUILD_DIR")
    out = keep or str(tmp_path_factory.mktemp("banded_emu"))
    os.makedirs(out, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in ("sa_internal.h", "sa_layout.h", "sa_band_plan.h", "sa_band_group.h",
                                                "sa_band_sweep.h", "sa_banded_fill.h", "sa_banded_affine_fill.h")]
    headers += [os.path.join(SHIM, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "seqalib_hip.h")]
    t0 = time.time()

    def compile_unit(unit):
        src, obj = os.path.join(CSRC, unit + ".hip"), os.path.join(out, unit + ".o")
        if not newer(obj, [src] + headers):
            subprocess.run([CXX, *FLAGS, "-x", "c++", "-c", src, "-o", obj], check=True)
        return obj

    with ThreadPoolExecutor(JOBS) as pool:
        objs = list(pool.map(compile_unit, UNITS))
    exe = {"driver": os.path.join(out, "banded_emu"), "selftest": os.path.join(out, "wave_emu_selftest")}
    src = os.path.join(CPP, "banded_emu.cpp")
    if not newer(exe["driver"], [src] + objs + headers):
        subprocess.run([CXX, *FLAGS, *LINK, src, *objs, "-o", exe["driver"]], check=True)
    src = os.path.join(CPP, "wave_emu_selftest.cpp")
    if not newer(exe["selftest"], [src] + headers):
        subprocess.run([CXX, *FLAGS, *LINK, src, "-o", exe["selftest"]], check=True)
    exe["dir"] = out
    print(f"banded_emu: built in {time.time() - t0:.0f} s with {JOBS} jobs")
    return exe


# --------------------------------------------------------------------------------------------- the cases
class Case:
    """One call: family corridor / ends_free / seeded / extend, or seeded_dev (dev: a dict of descriptors)."""
    count = 0

    def __init__(self, family, algo, args, w, pairs, diags=None, xdrop=OFF, fe=0, lut=False, merge=True, notb=False, simds=1024,
                 budget=None, dev=None, short_rec=0, walk_shift=0, submat=None, name=None):
        Case.count += 1
        self.name = f"{name or family}_{Case.count}"
        self.family, self.algo, self.args, self.w, self.pairs = family, algo, args, w, pairs
        self.diags = diags if diags is not None else [0] * len(pairs)
        self.xdrop, self.fe, self.lut, self.merge, self.notb, self.simds = xdrop, fe, lut, merge, notb, simds
        self.budget, self.dev, self.short_rec, self.walk_shift = budget, dev, short_rec, walk_shift
        self.submat = submat   # the matrix calls: a 256 x 256 int16 table (family corridor)

    def text(self):
        g, ma, mi, go, ge, allow = scoring_fields(self.args)
        hx = lambda b: bytes(b).hex() or "-"
        lines = [f"case {self.name}", f"family {self.family}", f"algo {self.algo}",
                 f"scoring {g} {ma} {mi} {int(bool(allow))} {go} {ge}", f"w {self.w}", f"xdrop {self.xdrop}", f"free_ends {self.fe}",
                 f"merge {int(self.merge)}", f"notb {int(self.notb)}", f"simds {self.simds}"]
        if self.budget is not None:
            lines.append(f"budget {self.budget}")
        if self.short_rec:
            lines.append(f"short_rec {self.short_rec}")
        if self.walk_shift:
            lines.append(f"walk_shift {self.walk_shift}")
        label, pairs = PURINE.reshape(256, 256) != 0, self.pairs
        if self.submat is not None:
            # sub_recode (sa_api_ctx.h): the batch's symbols in byte order become codes, the table its dense K x K
            # corner, the label table one over codes; match / mismatch carry the corner's extremes and are not read
            syms = sorted(set(b"".join(a + b for a, b in pairs))) or [0]
            code = {b: k for k, b in enumerate(syms)}
            pairs = [(bytes(code[x] for x in a), bytes(code[x] for x in b)) for a, b in pairs]
            corner = np.asarray(self.submat)[np.ix_(syms, syms)].astype(">i2")
            lines.append(f"submat {len(syms)} {corner.tobytes().hex()}")
            lines[3] = f"scoring {g} {max(0, int(corner.max()))} {min(0, int(corner.min()))} 1 {go} {ge}"
            full = np.zeros((256, 256), dtype=bool)
            full[:len(syms), :len(syms)] = label[np.ix_(syms, syms)]
            label = full
        if self.lut:
            words = np.packbits(label, axis=1, bitorder="little").reshape(-1).view("<u4")
            lines.append("lut " + "".join(f"{int(x):08x}" for x in words))
        if self.dev:
            d = self.dev
            lines += [f"resident1 {hx(d['seq1'])}", f"resident2 {hx(d['seq2'])}", f"bounds {d['max_m']} {d['max_n']}",
                      f"ops_bytes {d['ops_bytes']}"]
            lines += [f"dpair {a} {m} {b} {n} {k} {o}" for a, m, b, n, k, o in d["pairs"]]
        else:
            lines += [f"pair {hx(a)} {hx(b)} {k}" for (a, b), k in zip(pairs, self.diags)]
        return "\n".join(lines + ["end"]) + "\n"


def parse(path):
    """{case name: {"launch": [(v, first, count)], "list": [...], "ws": n, "res": {p: tuple}, "ops": {p: bytes},
    "rec": {p: (variant, words, unwritten)}, "tail": n, "poison": "SAME"}}"""
    out, cur = {}, None
    for line in open(path):
        f = line.split()
        if f[0] == "case":
            cur = out.setdefault(f[1], {"launch": [], "list": [], "res": {}, "ops": {}, "rec": {}, "done": False})
        elif f[0] == "launch":
            cur["launch"].append(tuple(int(x) for x in f[1:]))
        elif f[0] == "list":
            cur["list"].append(tuple(int(x) for x in f[1:]))
        elif f[0] == "res":
            cur["res"][int(f[1])] = tuple(int(x) for x in f[2:])
        elif f[0] == "ops":
            cur["ops"][int(f[1])] = b"" if f[2] == "-" else f[2].encode()
        elif f[0] == "rec":
            cur["rec"][int(f[1])] = tuple(int(x) for x in f[2:])
        elif f[0] == "opsmask":
            cur["opsmask"] = "" if f[1] == "-" else f[1]
        elif f[0] in ("ws", "tail"):
            cur[f[0]] = int(f[1])
        elif f[0] == "poison":
            cur["poison"] = f[1]
        elif f[0] == "end":
            cur["done"] = True
    return out


def run_driver(emu, cases, tag, expect_failure=False):
    """The cases through the driver, RUNNERS processes side by side; {case name: parsed output}.  A sanitizer
    report, a shim abort or a driver complaint ends a process with a non-zero status: the test fails with its text."""
    chunks = [cases[k::RUNNERS] for k in range(RUNNERS) if cases[k::RUNNERS]]
    procs = []
    for k, chunk in enumerate(chunks):
        cin, cout = os.path.join(emu["dir"], f"{tag}_{k}.cases"), os.path.join(emu["dir"], f"{tag}_{k}.out")
        with open(cin, "w") as f:
            f.write("".join(c.text() for c in chunk))
        procs.append((subprocess.Popen([emu["driver"], cin, cout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), cout))
    got, failures = {}, []
    for proc, cout in procs:
        _, err = proc.communicate()
        if proc.returncode != 0:
            failures.append((proc.returncode, err[-3000:]))
        elif os.path.exists(cout):
            got.update(parse(cout))
    if expect_failure:
        return failures
    assert not failures, failures
    assert all(got[c.name]["done"] for c in cases)
    return got


@functools.lru_cache(maxsize=None)
def model(family, algo, args, a, b, k, w, x, fe, lut):
    """(score, end_i, end_j, start_i, start_j, ops, flags) of one pair, from the family's Python model."""
    table = PURINE if lut else None
    if family == "extend":
        r = extend_model(algo, args, a, b, w, x, table)
        return r[:6] + (DROPPED if r[6] else 0,)
    if family in ("seeded", "seeded_dev"):
        return tuple(seeded_model(algo, args, a, b, k, w, fe, table)) + (0,)
    if family == "ends_free":
        return tuple(ends_free_model(algo, args, a, b, w, fe, table)) + (0,)
    r = banded_affine_model(algo, args, a, b, w, table) if affine(algo) else banded_model(algo, args, a, b, w, table)
    return tuple(r) + (0,)


def expected(c, p):
    a, b = c.pairs[p]
    if c.submat is not None:
        return matrix_model(c.algo, c.args, c.submat_key, a, b, c.w, c.lut)
    return model(c.family, c.algo, c.args, a, b, c.diags[p], c.w, c.xdrop, c.fe, c.lut)


def geometry(c, p):
    """(lo', hi', tb, tend) of pair p as its family clips the band."""
    m, n = len(c.pairs[p][0]), len(c.pairs[p][1])
    if c.family in ("corridor", "ends_free"):
        d = n - m
        lo, hi = max(min(d, 0) - c.w, -m), min(max(d, 0) + c.w, n)
        return lo, hi, (-lo) & ~1, m + n - lo
    k = 0 if c.family == "extend" else c.diags[p]
    lo, hi = seeded_band(m, n, k, c.w)
    return (lo, hi) + tuple(seeded_steps(m, n, k, c.w))


def check(c, got, models=True):
    """One case's output: the poison runs agree, every record word of every pair that ran to its end was written,
    nothing outside the pairs' ranges changed, and every result and op is the model's."""
    g = got[c.name]
    assert g["poison"] == "SAME", (c.name, "the two poison runs differ: a walk read a word the call had not written")
    assert g["tail"] == 0, (c.name, "record words outside every pair's range changed")
    for p in range(len(c.pairs)):
        res = g["res"][p]
        where = (c.name, c.family, c.algo, c.args, c.w, c.xdrop, c.fe, p, len(c.pairs[p][0]), len(c.pairs[p][1]))
        if not c.notb:
            v, words, unwritten = g["rec"][p]
            if not res[6] & DROPPED:
                assert unwritten == 0, where + (v, words, unwritten, "record words never written")
        if not models:
            continue
        want = expected(c, p)
        if c.notb:
            assert res == want[:3] + (-1, -1, 0, want[6], 0), where + (res, want)
        else:
            assert res == want[:5] + (len(want[5]), want[6], 0), where + (res, want[:5], len(want[5]))
            assert g["ops"][p] == want[5], where
    return g


def run_and_check(emu, cases, tag):
    got = run_driver(emu, cases, tag)
    for c in cases:
        check(c, got)
    return got


def launched_variant(g, p_entry=0):
    return g["launch"][p_entry][0]


# ------------------------------------------------------------------------------------- 0. the shim itself
def test_shim_selftest(emu):
    out = subprocess.run([emu["selftest"]], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]
    for what, message in (("shfl-exited", "__shfl_xor reads a lane that has exited"),
                          ("first-exited", "readfirstlane reads lane 0, which has exited"), ("dpp-control", "update_dpp: only controls")):
        out = subprocess.run([emu["selftest"], what], capture_output=True, text=True)
        assert out.returncode != 0 and message in out.stderr and "not refused" not in out.stdout, (what, out.returncode, out.stderr[-500:])


# --------------------------------------------------------------------- 1. the open fault's case, by name
FAULT_W, FAULT_ARGS = 1023, WIDE_SCORINGS[GG][0]


def test_the_open_fault_case(emu):
    """GlobalGotoh, w = 1023 (16 cells per lane), (2, -1, 1, -1), the clipped 40 x 1073 pair
    of variant_pairs(1023) whose best cell is the sweep's last -- as one launch of three pairs and alone, with every
    xdrop of the issue.  The full pairs' ops come from the model once (xdrop off: under this scoring nothing falls)."""
    pairs = variant_pairs(FAULT_W)
    assert FAULT_ARGS == (2, -1, 1, -1, True) and [(len(a), len(b)) for a, b in pairs] == [(1223, 1223), (1223, 1222), (40, 1073)]
    a, b = pairs[2]
    lo, hi, tend = extend_band(len(a), len(b), FAULT_W)
    assert (lo, hi, hi - lo + 1, tend) == (-40, 1023, 1064, 1143) and variant_of(hi - lo + 1) == 6
    want = model("extend", GG, FAULT_ARGS, a, b, 0, FAULT_W, OFF, 0, False)
    assert want[:5] == (1103, 40, 1063, 0, 0) and want[1] + want[2] - lo == tend   # the end cell is the last step's
    for x in (0, 1, 5, INT_MAX):   # every step rises: no checkpoint sees a fall
        assert extend_fill_np(GG, FAULT_ARGS, a, b, FAULT_W, x)[:4] == (1103, 40, 1063, False)
    cases = [Case("extend", GG, FAULT_ARGS, FAULT_W, [pairs[2]], xdrop=x, name="fault_alone") for x in (OFF, 0, 1, 5, INT_MAX)]
    cases += [Case("extend", GG, FAULT_ARGS, FAULT_W, [pairs[2]], xdrop=OFF, notb=True, name="fault_score")]
    three = [Case("extend", GG, FAULT_ARGS, FAULT_W, pairs, xdrop=x, name="fault_three") for x in (OFF, 0, INT_MAX)]
    got = run_driver(emu, cases + three, "fault")
    for c in cases:
        g = check(c, got, models=False)
        assert g["launch"] == [(6, 0, 1)] and (c.notb or g["rec"][0] == (6, 141312, 0))
        res = g["res"][0]
        if c.notb:
            assert res == (1103, 40, 1063, -1, -1, 0, 0, 0)
        else:
            assert res == want[:5] + (1103, 0, 0) and g["ops"][0] == want[5]
    for c in three:
        g = check(c, got, models=False)
        assert g["launch"] == [(6, 0, 3)]
        for p in range(3):
            x, y = pairs[p]
            sc, ei, ej, drop, _ = extend_fill_np(GG, FAULT_ARGS, x, y, FAULT_W, c.xdrop)
            assert not drop and g["res"][p][:3] == (sc, ei, ej) and g["res"][p][3:5] == (0, 0) and g["res"][p][6:] == (0, 0)
        assert g["res"][2] == want[:5] + (1103, 0, 0) and g["ops"][2] == want[5]
    c = three[0]   # ops of the two full pairs: the model, once
    for p in (0, 1):
        w2 = expected(c, p)
        assert got[c.name]["res"][p] == w2[:5] + (len(w2[5]), 0, 0) and got[c.name]["ops"][p] == w2[5]


def test_the_batch_of_section_2_19(emu):
    """The w = 1025 batch that ended the device-resident extension calls: 12 related pairs whose clipped bands hold
    32 ... 1025 diagonals, xdrop 30, GlobalGotoh -- through the host-planned extension call, which is the code in
    the tree.  The 1025-diagonal pair runs at 16 cells per lane; its band is clipped and it runs to its last step."""
    rng = np.random.default_rng(1025)
    pairs = []
    for d in (32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025):
        m = min(40, d - 8)   # clipped on the Seq1 side: min(w, m) + min(w, n) + 1 = m + (d - m - 1) + 1
        a = seq(rng, ACGT, m)
        pairs.append((a, (edited(rng, a, 0.05) + seq(rng, ACGT, d))[:d - m - 1]))
    diagonals = [extend_band(len(a), len(b), 1025)[1] - extend_band(len(a), len(b), 1025)[0] + 1 for a, b in pairs]
    assert diagonals == [32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025]
    assert {variant_of(d) for d in diagonals} == {0, 1, 2, 3, 4, 5, 6}
    args = (-4, -1, 1, -3)
    cases = [Case("extend", GG, args, 1025, pairs, xdrop=30, merge=merge, name="batch_2_19") for merge in (False, True)]
    cases += [Case("extend", GG, FAULT_ARGS, 1025, pairs, xdrop=30, merge=False, name="batch_2_19_rising")]
    wide = expected(cases[2], 11)
    assert wide[1] + wide[2] + min(1025, len(pairs[11][0])) == extend_band(len(pairs[11][0]), len(pairs[11][1]), 1025)[2]
    got = run_and_check(emu, cases, "b219")
    assert sorted(v for v, _, _ in got[cases[0].name]["launch"]) == [0, 1, 2, 3, 4, 5, 6]
    assert len(got[cases[1].name]["launch"]) < 7   # merged: some pairs run one variant wider than their own


# ---------------------------------------------------------- 2. both sides of every variant's capacity
def clipped_pair(rng, m, n):
    a = seq(rng, ACGT, m)
    return a, (edited(rng, a, 0.05) + seq(rng, ACGT, n))[:n]


def capacity_diagonals(algo):
    """Per variant: its capacity 2RL, and one diagonal more than the next narrower variant holds."""
    top = 7 if affine(algo) else 8
    out = []
    for v in range(top):
        R, L = VARIANTS[v]
        out.append((v, 2 * R * L))
        if v:
            out.append((v, 2 * VARIANTS[v - 1][0] * VARIANTS[v - 1][1] + 1))
    return out


CAPACITY_SCORING = {NW: (-2, 1, -3), SW: (-2, 2, -3), GG: (-4, -1, 1, -3), LG: (-3, -1, 2, -1)}


def capacity_case(family, algo, v, diagonals, seed):
    """The shortest clipped pair (m = min(40, .) < w < n) whose band holds `diagonals` diagonals in this family."""
    rng = np.random.default_rng(seed)
    m = min(40, max(1, diagonals // 2 - 1))
    if family in ("corridor", "ends_free"):   # lo' = -m, hi' = n: diagonals = m + n + 1, inside the corridor of w
        n = diagonals - m - 1
        w = n   # (n - m + w >= n and w >= m: both clips are the matrix's)
        fe, k = (sa.SA_FREE_SEQ2_END if family == "ends_free" else 0), 0
    else:                                      # lo' = -m, hi' = w: diagonals = m + w + 1
        w = diagonals - m - 1
        n = w + 50
        fe, k = (sa.SA_FREE_SEQ2_END if family == "seeded" else 0), 0
    pair = clipped_pair(rng, m, n)
    c = Case(family, algo, CAPACITY_SCORING[algo], w, [pair], diags=[k], xdrop=OFF, fe=fe, merge=False, name=f"cap_{family}_{algo}_{v}_{diagonals}")
    lo, hi, tb, tend = geometry(c, 0)
    assert hi - lo + 1 == diagonals and variant_of(diagonals) == v, (family, algo, v, diagonals, lo, hi)
    return c


@pytest.mark.parametrize("family,algo", [(f, a) for f in ("extend", "seeded", "ends_free") for a in (NW, GG)] +
                         [("corridor", a) for a in (NW, SW, GG, LG)])
def test_both_sides_of_every_capacity(emu, family, algo):
    cases = [capacity_case(family, algo, v, d, 100 * v + d) for v, d in capacity_diagonals(algo)]
    assert {VARIANTS[variant_of(geometry(c, 0)[1] - geometry(c, 0)[0] + 1)][0] for c in cases} == \
        ({1, 2, 4, 8, 16} if affine(algo) else {1, 2, 4, 8, 16, 32})
    cases += [Case(c.family, c.algo, c.args, c.w, c.pairs, diags=c.diags, fe=c.fe, merge=False, notb=True, name=c.name + "_score")
              for c in cases[::3]]
    got = run_and_check(emu, cases, f"cap_{family}_{algo}")
    for c in cases:
        lo, hi, _, _ = geometry(c, 0)
        assert got[c.name]["launch"] == [(variant_of(hi - lo + 1), 0, 1)]


# ------------------------------------------ 3. clipped pairs whose best cell is the sweep's last cell
RISING = {NW: (1, 1, -1), GG: (2, -1, 1, -1, True)}         # every step rises (gap > 0)
ORDINARY = {NW: (-2, 1, -3), GG: (-4, -1, 1, -3)}


def last_cell_pairs(v, seed):
    """A pair clipped on the Seq1 side (m < w < n) at variant v's capacity, and its transpose."""
    R, L = VARIANTS[v]
    w = 2 * R * L - 41
    a, b = clipped_pair(np.random.default_rng(seed), 40, w + 50)
    return w, [(a, b), (b, a)]


@pytest.mark.parametrize("algo", [NW, GG])
def test_clipped_pairs_that_end_in_the_last_cell(emu, algo):
    """The conditions of the open fault, for every 64-lane variant: under the rising scoring the end cell is the last
    cell of the sweep (asserted on the model), so the walk starts in the records of step tend; under the ordinary one
    it lies early.  xdrop off, 0 and 2^31 - 1; the pair and its transpose in one launch and each alone."""
    cases = []
    for v in range(4, 7 if algo == GG else 8):
        w, pairs = last_cell_pairs(v, 40 + v)
        for a, b in pairs:
            lo, hi, tend = extend_band(len(a), len(b), w)
            assert hi - lo + 1 == 2 * VARIANTS[v][0] * VARIANTS[v][1] and min(len(a), len(b)) < w < max(len(a), len(b))
            r = model("extend", algo, RISING[algo], a, b, 0, w, OFF, 0, False)
            assert r[1] + r[2] - lo == tend and r[3:5] == (0, 0), (v, r[:5], tend)
            o = model("extend", algo, ORDINARY[algo], a, b, 0, w, OFF, 0, False)
            assert o[1] + o[2] - lo < tend
        for args in (RISING[algo], ORDINARY[algo]):
            for x in (OFF, 0, INT_MAX):
                cases.append(Case("extend", algo, args, w, pairs, xdrop=x, merge=False, name=f"last_{algo}_{v}"))
            if args == RISING[algo]:
                cases += [Case("extend", algo, args, w, [p], xdrop=OFF, merge=False, name=f"last_alone_{algo}_{v}") for p in pairs]
        # the same cells through the seeded call (diagonal 0, both ends free): its end cell is on the border
        cases.append(Case("seeded", algo, RISING[algo], w, pairs, fe=sa.SA_FREE_SEQ1_END | sa.SA_FREE_SEQ2_END, merge=False, name=f"last_seeded_{algo}_{v}"))
    got = run_and_check(emu, cases, f"last_{algo}")
    for c in cases:
        assert all(v == variant_of(geometry(c, 0)[1] - geometry(c, 0)[0] + 1) for v, _, _ in got[c.name]["launch"])


# ----------------------------------------------------------------------------------- 4. mixed waves
@pytest.mark.parametrize("algo", [NW, GG])
def test_mixed_waves(emu, algo):
    """Waves of 4, 2 and 1 pairs with idle lane groups; the w = 12 batch (m < w pairs, transposes, tend = 14, 15, 0,
    1 mod 16 in shared waves); a batch in which pairs of one wave stop at different checkpoints and one runs on."""
    args = PHASE_SCORING[algo]
    phase = phase_batch()
    for ph, shape in PHASE_PAIRS.items():
        assert extend_band(*shape, PHASE_W)[2] % XDROP_PERIOD == ph
    cases = [Case("extend", algo, args, PHASE_W, phase, xdrop=x, lut=lut, name="phase") for x in (10, OFF) for lut in (False, True)]
    four = mixed_batch()
    assert len(four) % 4 == 3   # the last wave has an idle lane group
    cases += [Case("extend", algo, args, w, four, xdrop=10, name="four") for w in (8, 15)]
    cases += [Case("extend", algo, args, 8, four[:k], xdrop=10, name="idle") for k in (1, 2, 5)]
    seven = mixed_seven()
    for w, per_wave in ((100, 2), (200, 1)):
        full = [(a, b) for a, b in seven if a]
        assert {64 // VARIANTS[variant_of(extend_band(len(a), len(b), w)[1] - extend_band(len(a), len(b), w)[0] + 1)][1] for a, b in full} == {per_wave}
        cases.append(Case("extend", algo, args, w, seven, xdrop=10, merge=False, name=f"seven_{per_wave}"))
    # one wave of four: its pairs stop at different checkpoints, one runs to its end
    div, isl, rel = drop_inputs()
    wave = [div[0], rel[0], isl[0], div[1]]
    stops = [extend_model(algo, args, *wave[p], 8, 10)[7] for p in launch_order(wave)]
    assert None in stops and len({s for s in stops if s is not None}) >= 2, stops
    cases.append(Case("extend", algo, args, 8, wave, xdrop=10, name="one_wave"))
    four_at_8 = cases[4]
    got = run_and_check(emu, cases, f"mixed_{algo}")
    assert got[cases[-1].name]["launch"] == [(0, 0, 4)]   # 17 diagonals: four pairs of 16 lanes in one wave
    # a stopped pair leaves record words unwritten, and the walk did not read them (the poison runs agree)
    g = got[four_at_8.name]
    assert any(g["res"][p][6] & DROPPED and g["rec"][p][2] > 0 for p in range(len(four)))


# ------------------------------------------------------------------ 5. seeded: flags and diagonals
@pytest.mark.parametrize("algo", [NW, GG])
def test_seeded_flag_sets_and_diagonals(emu, algo):
    """All 16 flag sets on legal_batch's ragged pairs (w in {0, 1, 3, 8}), and seed diagonals at -m, n, 0 and +-1 round
    n - m for the flag sets under which each is legal."""
    from test_gpu_banded_seeded import SCORINGS
    cases = []
    for fe in range(16):
        for n_w, w in enumerate((0, 1, 3, 8)):
            args = SCORINGS[algo][(fe + n_w) % 3]
            if w == 0 and not scoring_fields(args)[5]:
                args = SCORINGS[algo][0]
            pairs, diags = legal_batch(1000 * fe + w, w, fe, 16)
            cases.append(Case("seeded", algo, args, w, pairs, diags=diags, fe=fe, lut=bool(fe & 1), name=f"flags_{fe}_{w}"))
    rng = np.random.default_rng(5)
    a, b = seq(rng, ACGT, 23), seq(rng, ACGT, 31)
    seen = set()
    for w in (1, 3):
        for fe in range(16):
            pairs, diags = [], []
            for x, y in ((a, b), (b, a), (a, a)):
                m, n = len(x), len(y)
                for k in (-m, n, 0, n - m - 1, n - m, n - m + 1):
                    if -m <= k <= n and seeded_legal(m, n, k, w, fe) == (True, True):
                        pairs.append((x, y))
                        diags.append(k)
                        seen.add((k == -m, k == n, k == 0, k - (n - m)))
            if pairs:
                cases.append(Case("seeded", algo, SCORINGS[algo][0], w, pairs, diags=diags, fe=fe, name=f"diag_{fe}_{w}"))
    assert {s[3] for s in seen} >= {-1, 0, 1} and any(s[0] for s in seen) and any(s[1] for s in seen) and any(s[2] for s in seen)
    run_and_check(emu, cases, f"seeded_{algo}")


# ----------------------------------------------------- 6. corridor and ends-free families, merge on and off
@pytest.mark.parametrize("family,algo", [("corridor", a) for a in (NW, SW, GG, LG)] + [("ends_free", a) for a in (NW, GG)])
def test_ragged_batches(emu, family, algo):
    """About 16 ragged pairs of at most 80 symbols (empty ones included: SW and LocalGotoh on an empty pair) at
    w in {0, 1, 3, 8}, byte equality and the purine table, align and score call; one batch over several variants with
    band_group's merge on and off, so that pairs launched one variant wider than their own are covered."""
    args = CAPACITY_SCORING[algo]
    pairs = regime_batch(algo)   # 16 pairs: empty shapes, ragged ones, related heads with unrelated tails, m < 8
    assert len(pairs) == 16 and all(len(a) <= 80 and len(b) <= 80 for a, b in pairs) and pairs[0] == (b"", b"")
    cases = []
    for n_w, w in enumerate((0, 1, 3, 8)):
        fe = [0, 5, 10, 15][n_w] if family == "ends_free" else 0
        cases.append(Case(family, algo, args, w, pairs, fe=fe, lut=bool(n_w & 1), name=f"ragged_{w}"))
        cases.append(Case(family, algo, args, w, pairs, fe=fe, notb=True, name=f"ragged_score_{w}"))
    rng = np.random.default_rng(9)
    mixed = []
    for s in (12, 20, 40, 70, 100, 9, 33):   # 25 ... 201 diagonals at w >= s: variants 0 ... 3
        a = seq(rng, ACGT, s)
        mixed.append((a, edited(rng, a, 0.1)[:s + 3]))
    for merge in (False, True):
        cases.append(Case(family, algo, args, 128, mixed, fe=15 if family == "ends_free" else 0, merge=merge, name=f"merge_{int(merge)}"))
    got = run_and_check(emu, cases, f"ragged_{family}_{algo}")
    off, on = got[cases[-2].name], got[cases[-1].name]
    assert len(on["launch"]) < len(off["launch"]) and len(off["launch"]) >= 3
    own = {p: variant_of(geometry(cases[-1], p)[1] - geometry(cases[-1], p)[0] + 1) for p in range(len(mixed))}
    assert any(on["rec"][p][0] == own[p] + 1 for p in own) and all(off["rec"][p][0] == own[p] for p in own)


# ------------------------------------------------------------------------------ 7. the planted faults
def test_a_record_buffer_one_word_short_is_reported(emu):
    """The sanitized driver must see what it is there for: the faulting shape with records one word short of
    band_affine_rec_words ends in an address-sanitizer report, not in an answer."""
    pair = variant_pairs(FAULT_W)[2]
    for algo, args in ((GG, FAULT_ARGS), (NW, RISING[NW])):
        failures = run_driver(emu, [Case("extend", algo, args, FAULT_W, [pair], short_rec=1, name="short")], "short", expect_failure=True)
        assert len(failures) == 1 and "AddressSanitizer: heap-buffer-overflow" in failures[0][1], failures


@pytest.mark.parametrize("algo", [NW, GG])
def test_a_walk_with_the_neighbouring_variant_is_caught(emu, algo):
    """A walk told the next narrower (or wider) variant's R and L reads other words than the fill wrote: the poison
    comparison, the model comparison or the sanitizer must say so."""
    w, pairs = last_cell_pairs(5, 45)
    for shift in (-1, 1):
        c = Case("extend", algo, RISING[algo], w, pairs[:1], walk_shift=shift, merge=False, name=f"shift_{shift}")
        failures = run_driver(emu, [c], f"shift_{algo}", expect_failure=True)
        if failures:
            continue   # a sanitizer report
        got = parse(os.path.join(emu["dir"], f"shift_{algo}_0.out"))
        want = expected(c, 0)
        g = got[c.name]
        assert g["poison"] == "DIFFER" or g["res"][0] != want[:5] + (len(want[5]), want[6], 0) or g["ops"][0] != want[5], shift


# ----------------------------------------------------------- 8. the device-planned seeded calls
def bound_words(max_m, max_n, w, aff):
    """band_plan_bound_seeded (sa_band_plan.h) restated: the record words the host provisions per pair."""
    diagonals = min(2 * w + 1, max_m + max_n + 1)
    steps = min(max_m + max_n, 2 * max_m + 2 * w, 2 * max_n + 2 * w) + 2
    R, L = VARIANTS[variant_of(diagonals)]
    per_word = (8 if aff else 16) // R
    return -(-steps // per_word) * L if per_word else steps * (R // (8 if aff else 16)) * L


def dev_case(algo, args, b, w, fe, max_m, max_n, lut=False, chunk=None, notb=False, name="dev"):
    """A device-planned call on a Batch of tests/test_gpu_banded_seeded_device.py.  chunk: the pairs per chunk, set
    through the workspace budget as a caller would (sa_api_banded_device.hip: an 8 KiB head, 512 bytes of alignment,
    then per pair the bound's records and 17 words of plan)."""
    dev = {"seq1": b.seq1.tobytes(), "seq2": b.seq2.tobytes(), "max_m": max_m, "max_n": max_n, "ops_bytes": b.ops_bytes,
           "pairs": [tuple(int(x) for x in t) for t in zip(b.start1, b.len1, b.start2, b.len2, b.diag, b.ops_off)]}
    budget = None
    if chunk:
        per_pair = (0 if notb else bound_words(max_m, max_n, w, affine(algo))) + 17
        budget = 4 * 2048 + 512 + 4 * per_pair * chunk + 3
    pairs = []
    for a, m, s, n, _, _ in dev["pairs"]:   # (a refused pair's slice may lie outside its buffer: no model runs on it)
        inside = a + m <= len(dev["seq1"]) and s + n <= len(dev["seq2"])
        pairs.append((dev["seq1"][a:a + m], dev["seq2"][s:s + n]) if inside else (b"", b""))
    return Case("seeded_dev", algo, args, w, pairs, diags=[int(k) for k in b.diag], fe=fe, lut=lut, budget=budget, dev=dev,
                notb=notb, name=name)


def host_twin(c):
    return Case("seeded", c.algo, c.args, c.w, c.pairs, diags=c.diags, fe=c.fe, lut=c.lut, merge=False, notb=c.notb, name=c.name + "_host")


def same_as_host(got, c, h, pairs=None):
    for p in (range(len(c.pairs)) if pairs is None else pairs):
        assert got[c.name]["res"][p] == got[h.name]["res"][p], (c.name, p, got[c.name]["res"][p], got[h.name]["res"][p])
        if not c.notb:
            assert got[c.name]["ops"][p] == got[h.name]["ops"][p], (c.name, p)


def untouched_ops(got, c, refused=()):
    """The ops buffer's bytes outside the ops the results count are what they were before the call."""
    g = got[c.name]
    written = np.zeros(c.dev["ops_bytes"], dtype=bool)
    for p, t in enumerate(c.dev["pairs"]):
        if p not in refused:
            written[t[5]:t[5] + g["res"][p][5]] = True
    mask = np.frombuffer(g["opsmask"].encode(), dtype=np.uint8) == ord("1")
    assert written.any() and not (mask & ~written).any(), (c.name, "a byte outside the pairs' ops was written")


@pytest.mark.parametrize("algo", [NW, GG])
def test_device_planned_flag_sets_and_chunks(emu, algo):
    """All 16 flag sets on the host call's own layout, as one chunk and in chunks of one and of five pairs: the planned
    results are the host-planned call's, byte for byte, and the model's."""
    from test_gpu_banded_seeded_device import SCORINGS, Batch
    cases, twins = [], []
    for fe in range(16):
        w = (0, 1, 3, 8)[fe % 4]
        args = SCORINGS[algo][fe % 3]
        if w == 0 and not scoring_fields(args)[5]:
            args = SCORINGS[algo][0]
        pairs, diags = legal_batch(1000 * fe + w, w, fe, 16)
        b = Batch.packed(pairs, diags)
        chunk = (None, 1, 5)[fe % 3]
        cases.append(dev_case(algo, args, b, w, fe, 40, 40, lut=bool(fe & 2), chunk=chunk, name=f"dev_flags_{fe}"))
        twins.append(host_twin(cases[-1]))
        if fe % 5 == 0:
            cases.append(dev_case(algo, args, b, w, fe, 40, 40, chunk=chunk, notb=True, name=f"dev_score_{fe}"))
            twins.append(host_twin(cases[-1]))
    got = run_and_check(emu, cases + twins, f"devflags_{algo}")
    for c, h in zip(cases, twins):
        same_as_host(got, c, h)
        chunk = (None, 1, 5)[c.fe % 3]
        starts = sorted({t[0] for t in got[c.name]["list"]})
        assert starts == (list(range(0, len(c.pairs), chunk)) if chunk else [0]), (c.name, starts)
        assert sum(t[2] for t in got[c.name]["list"]) == len(c.pairs)   # every pair is in exactly one list
        if not c.notb:
            untouched_ops(got, c)


@pytest.mark.parametrize("algo", [NW, GG])
def test_device_planned_variants(emu, algo):
    """Every variant on both sides of its capacity in one call (test_gpu_banded_seeded_device.variant_batch), the
    clipped 40 x 1073 pair at 16 cells per lane among them: the host-planned call's bytes, and the model's for the
    pairs of at most 64 symbols and the clipped one."""
    from test_gpu_banded_seeded_device import S2E, SCORINGS, variant_batch
    sizes = (15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512) if algo == NW else (15, 16, 31, 32, 63, 64, 127, 128, 255, 256)
    w = 1023
    b = variant_batch(sizes, True, 31 * w + len(sizes), upload=False)
    c = dev_case(algo, SCORINGS[algo][0], b, w, S2E, max(sizes), 1073, name="dev_variants")
    h = host_twin(c)
    used = {variant_of(2 * int(m) + 1 if m == n else int(m) + w + 1) for m, n in zip(b.len1, b.len2)}
    assert used == {0, 1, 2, 3, 4, 5, 6}   # (GlobalGotoh: every variant it has)
    got = run_driver(emu, [c, h], f"devvar_{algo}")
    small = [p for p in range(b.n) if int(b.len1[p]) <= 64 or int(b.len2[p]) == 1073]
    for case in (c, h):
        g = check(case, got, models=False)
        for p in small:
            want = expected(case, p)
            assert g["res"][p] == want[:5] + (len(want[5]), 0, 0) and g["ops"][p] == want[5], (case.name, p)
    same_as_host(got, c, h)
    untouched_ops(got, c)
    assert {t[1] for t in got[c.name]["list"] if t[2]} == used


@pytest.mark.parametrize("algo", [NW, GG])
def test_device_planned_refusals(emu, algo):
    """The planner's refusals among valid neighbours: the refused pairs get the zero result with their one flag, enter
    no list and leave their ops region alone; the others are the host-planned call's."""
    from test_gpu_banded_seeded_device import SCORINGS, refusal_batch
    b, flags, align_only = refusal_batch(upload=False)
    args = SCORINGS[algo][0]
    c = dev_case(algo, args, b, 3, 0, 40, 40, name="dev_refusals")
    s = dev_case(algo, args, b, 3, 0, 40, 40, notb=True, name="dev_refusals_score")
    good = [p for p in range(b.n) if p not in flags]
    h = Case("seeded", algo, args, 3, [c.pairs[p] for p in good], diags=[c.diags[p] for p in good], merge=False, name="dev_refusals_host")
    got = run_driver(emu, [c, s, h], f"devref_{algo}")
    check(h, got)
    for case in (c, s):
        g = got[case.name]
        assert g["poison"] == "SAME" and g["tail"] == 0
        listed = sorted(p for t in g["list"] for p in t[3:])
        refused = [p for p in flags if not (case.notb and p in align_only)]
        assert listed == [p for p in range(b.n) if p not in refused]
        for p in range(b.n):
            if p in refused:
                assert g["res"][p] == (0, 0, 0, 0, 0, 0, flags[p], 0), (case.name, p, g["res"][p])
            elif p in good:
                want = got[h.name]["res"][good.index(p)]
                assert g["res"][p] == (want[:3] + (-1, -1, 0, 0, 0) if case.notb else want), (case.name, p)
                if not case.notb:
                    assert g["ops"][p] == got[h.name]["ops"][good.index(p)] and g["rec"][p][2] == 0
    untouched_ops(got, c, refused=list(flags))


# ------------------------------------------------------------------------------ 9. the matrix calls
MATRIX_TABLES = {}


@functools.lru_cache(maxsize=None)
def matrix_model(algo, args, key, a, b, w, lut):
    rows = MATRIX_TABLES[key].tolist()
    gaps = (args[0], args[1]) if affine(algo) else args[0]
    return tuple(banded_matrix_model(algo, gaps, rows, a, b, w, PURINE.reshape(256, 256).tolist() if lut else None)) + (0,)


@pytest.mark.parametrize("algo", [SW, NW, LG, GG])
def test_matrix_calls(emu, algo):
    """The fills with a substitution table in LDS (sa_banded_sub.hip, sa_banded_affine_sub.hip): 16 ragged pairs at
    w in {0, 1, 3, 8} over alphabets of K = 3 and K = 19 used symbols (odd: the dense table ends in half a word, which
    the host pads), with and without a label table, and a clipped pair at 8 cells per lane."""
    from test_gpu_banded_matrix import alphabet, random_table, redraw, scoring
    args = scoring(algo)
    cases = []
    for k in (3, 20):
        MATRIX_TABLES[k] = random_table(40 + k)
        alph = alphabet(k)[:19] if k == 20 else alphabet(k)
        pairs = redraw(regime_batch(algo), alph, 7 + k)
        assert len(set(b"".join(a + b for a, b in pairs))) == len(alph) and len(alph) % 2 == 1
        for n_w, w in enumerate((0, 1, 3, 8)):
            c = Case("corridor", algo, args, w, pairs, lut=bool(n_w & 1), submat=MATRIX_TABLES[k], notb=(n_w == 2), name=f"matrix_{k}_{w}")
            c.submat_key = k
            cases.append(c)
    rng = np.random.default_rng(77)
    a = seq(rng, alphabet(3), 40)
    wide = Case("corridor", algo, args, 500, [(a, a + seq(rng, alphabet(3), 460))], submat=MATRIX_TABLES[3], merge=False, name="matrix_wide")
    wide.submat_key = 3
    lo, hi, _, _ = geometry(wide, 0)
    assert VARIANTS[variant_of(hi - lo + 1)] == (8, 64)
    got = run_and_check(emu, cases + [wide], f"matrix_{algo}")
    assert got[wide.name]["launch"] == [(5, 0, 1)]


# ------------------------------------------------------ 10. square pairs: the sweep's interior steps
@pytest.mark.parametrize("family,algo", [("extend", NW), ("extend", GG), ("seeded", NW), ("seeded", GG), ("ends_free", NW),
                                         ("ends_free", GG), ("corridor", NW), ("corridor", SW), ("corridor", GG), ("corridor", LG)])
def test_square_pairs_take_the_interior_steps(emu, family, algo):
    """A clipped 40 x n pair has a border or an outside cell in every step, so the capacity cases above run the
    EDGE instantiation of step() only.  Pairs m = n = s + 100 with w = s hold 2s + 1 diagonals -- one more than the
    next narrower variant -- and sweep 200 steps through the other instantiation, whose stores are separate calls.
    s = 128 and 256 for every family; s = 512 (16 cells per lane) for the affine kernels and s = 512 and 1024 (32 cells
    per lane) for the linear template's two sweeps of their own (corridor NW, extension NW)."""
    sizes = [128, 256]
    if (family, algo) in (("corridor", NW), ("extend", NW)):
        sizes += [512, 1024]
    elif affine(algo) and family != "ends_free":
        sizes += [512]
    cases = []
    for s in sizes:
        rng = np.random.default_rng(s + algo)
        a = seq(rng, ACGT, s + 100)
        b = (edited(rng, a, 0.05) + seq(rng, ACGT, 40))[:s + 100]
        fe = sa.SA_FREE_SEQ2_END if family in ("seeded", "ends_free") else 0
        c = Case(family, algo, CAPACITY_SCORING[algo], s, [(a, b)], fe=fe, xdrop=OFF, merge=False, name=f"square_{s}")
        lo, hi, tb, tend = geometry(c, 0)
        assert hi - lo + 1 == 2 * s + 1 and VARIANTS[variant_of(2 * s + 1)] == (s // 32, 64)
        first, last = max(hi, -lo) - lo, min(2 * len(a) + lo, 2 * len(b) - hi) - lo   # steps without border or outside cells
        assert last - first == 200
        cases.append(c)
    got = run_and_check(emu, cases, f"square_{family}_{algo}")
    for c, s in zip(cases, sizes):
        assert got[c.name]["launch"] == [(variant_of(2 * s + 1), 0, 1)]
