"""GPU parity on scorings outside gap < 0 < match, mismatch < 0 (util.REGIME_LINEAR / REGIME_AFFINE).

The C ABI takes any int32 scoring, and the kernel-selection rules of sa_api.hip (t16_mode,
t16_mode_affine, keyed_ok) and sa_dc.h (dc16_plan) admit match <= 0, mismatch >= 0, mismatch = match,
gap = 0 and their corner values to the 16-bit kernels.  Every test here is bit-exact against the
oracle (pinned to the unmodified reference on the same scorings: tests/golden/regimes.jsonl,
test_oracle_golden.py::test_oracle_regimes) -- score, end cell, start cell, op stream and flags --
and asserts the kernel or plan it meant to reach, so that a fallback cannot make it pass.
"""
import os

import numpy as np
import pytest

import seqalib_amd as sa
from test_gpu_banded import banded_model, pair_ops, ragged_pairs
from test_gpu_parity import check_golden
from util import (ALGOS, LG_HACK_SIZES, ORACLE_RESULT_DTYPE, REGIME_AFFINE, REGIME_DIVERGING, REGIME_LINEAR,
                  golden_sequences, load_regimes, oracle_align, oracle_batch, pack_bytes, scoring_fields)

pytestmark = pytest.mark.gpu
BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py)

SW, NW, LG, GG, HB, MM = 0, 1, 2, 3, 4, 5
INT32 = (sa.SA_KERNEL_INT32,)
T16 = (sa.SA_KERNEL_T16, sa.SA_KERNEL_T16_ENDCELL)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def ident(s):
    return "_".join(str(int(x)) for x in s)


# ------------------------------------------------------------------ which kernel family runs
# By scoring, from the rules in sa_api.hip; the shape-dependent parts are functions of the batch's
# (max_m, max_n) below.
# t16_mode: match and mismatch in -32..31, mismatch <= match, gap in -4096..0 (SW: < 0);
# !AllowMismatch runs with mismatch' = 2 * gap - 1.
LIN_T16 = {(-1, 0, -1), (-1, -1, -2), (-1, 1, 0), (-1, 1, 1), (-1, 2, 1), (-2, 2, 2), (-3, 31, -32), (-4096, 31, -32),
           (-1, 0, -1, False), (-1, -1, -2, False)}
LIN_T16_GAP0 = {(0, 1, -1), (0, 1, 0), (0, 0, 0), (0, 3, 3), (0, 1), (0, 1, -1, False)}   # NW only
# t16_mode_affine: match and mismatch in -16..15, mismatch <= match, gap_open in -2048..0,
# gap_extend in -512..-1; !AllowMismatch runs with mismatch' = 2 * (gap_open + gap_extend) - 1.
# (-3, -1, 2, 2), (0, -2, 3, 1) and (-3, -5, 1, -1) pass every one of these: mismatch = match and
# 0 < mismatch < match are admitted (the rule refuses only mismatch > match), and so are
# gap_open = 0 and gap_extend = -5.
AFF_T16 = {(-3, -1, 0, -1, True), (-3, -1, 1, 0, True), (-3, -1, 1, 1, True), (-3, -1, -1, -2, True),
           (-3, -1, 15, -16, True), (-2048, -512, 15, -16, True), (-3, -1, 0, -1, False), (0, -1, 1, -1, False),
           (-3, -1, 2, 2, True), (0, -2, 3, 1, True), (-3, -5, 1, -1, True)}


def eff_mismatch(algo, args):
    g, ma, mi, go, ge, allow = scoring_fields(args)
    if allow:
        return mi
    return 2 * (go + ge) - 1 if algo in (LG, GG) else 2 * g - 1


def nw_window_fits(args, m, n):
    """t16_mode, NW: the range of H over the matrix (upper: the best diagonals plus the gaps that
    |i - j| forces, or the all-gap path; lower: the all-mismatch diagonal or the all-gap path, and
    one candidate below it) must fit 2^14 values: 4 * (H - delta) + tag in int16."""
    g, ma, _, _, _, _ = scoring_fields(args)
    mi = eff_mismatch(NW, args)
    k = min(m, n)
    pts = [(0, 0), (m, 0), (0, n), (k, k), (m, n), (k, n), (m, k)]
    hi = max(max(min(i, j) * ma + abs(i - j) * g, (i + j) * g) for i, j in pts)
    lo = min(max(min(i, j) * mi + abs(i - j) * g, (i + j) * g) for i, j in pts) + min(mi, g, 0)
    delta = (hi + lo) >> 1
    return 4 * (hi - delta) + 3 <= 32767 and 4 * (lo - delta) >= -32768


def keyed_fits(algo, args, m, n):
    """keyed_ok: the 16-bit (score, column) keys of the local modes hold match * min(m, n) when no
    substitution or gap term is positive, else (sum of the magnitudes) * (m + n); below 65,536."""
    g, ma, mi, go, ge, allow = scoring_fields(args)
    aff = algo == LG
    nonpos = (not allow or mi <= 0) and ((ge <= 0 and go + ge <= 0) if aff else g <= 0)
    if nonpos:
        return max(ma, 0) * min(m, n) < 65536
    return (abs(ma) + abs(mi) + abs(g) + abs(go) + abs(ge)) * (m + n) < 65536


def gg_window_fits(args, m, n, many):
    """t16_mode_affine, GlobalGotoh: match >= 0, the reference's -10000 Ix / Iy border wins nowhere,
    and the affine path bounds fit 2^13 values around an offset (8 * (V - delta) + 3 bits in int16)
    -- or, on the many-pairs plans, the window sits at the low end and at least typical pairs (half
    the best diagonal) stay below its cap, the others re-running in int32."""
    _, ma, _, go, ge, _ = scoring_fields(args)
    mi = eff_mismatch(GG, args)
    goe = go + ge
    if ma < 0 or go + max(m, n) * ge + goe <= -10000 + ge:
        return False
    k = min(m, n)
    gapc = lambda L: go + L * ge if L > 0 else 0
    pts = [(0, 0), (m, 0), (0, n), (k, k), (m, n), (k, n), (m, k)]
    hi = max(min(i, j) * ma + gapc(abs(i - j)) for i, j in pts)
    lo = min(max(min(i, j) * mi + go + abs(i - j) * ge, 2 * go + (i + j) * ge) for i, j in pts)
    cand_lo = lo + min(mi, goe + ge, 0)
    floor_ext = -32768 + 8 * -ge + 16 + 8 * ge + 1
    delta = (hi + cand_lo) >> 1
    if 8 * (hi - delta) + 7 <= 32767 and 8 * (cand_lo - delta) > floor_ext:
        return True
    if not many:   # t16_candidate: a band of the few-pairs band plan cannot leave its pair alone
        return False
    delta = cand_lo + 4100
    while 8 * (cand_lo - delta) <= floor_ext:
        delta -= 1
    return delta + (32767 - 7) // 8 >= max(ma, 0) * k // 2


def expected_kernels(algo, args, m, n, many=True):
    """The kernel family a DNA batch of at most m x n takes under the scoring (many: >= 1,024 pairs,
    or a few-pairs batch that does not take the band plan)."""
    if algo == SW:
        return T16 if args in LIN_T16 and keyed_fits(SW, args, m, n) else INT32
    if algo == NW:
        return T16 if (args in LIN_T16 or args in LIN_T16_GAP0) and nw_window_fits(args, m, n) else INT32
    if algo == LG:
        return T16 if args in AFF_T16 and keyed_fits(LG, args, m, n) else INT32
    return T16 if args in AFF_T16 and gg_window_fits(args, m, n, many) else INT32


# ----------------------------------------------------------------------------- running, comparing
def run(engine, algo, args, batch, env=None):
    """(results, ops, last_plan_ex) of sa_align_batch under the environment settings env."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        res, ops = engine.align_packed(algo, sa.ScoringSystem(*args), *batch)
        plan = engine.last_plan_ex()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return res.copy(), ops.copy(), plan


_ORACLE = {}
_DIVERGED = {}   # per oracle key: the pairs on which the oracle's walk found no move (rc == -3)


def oracle_pairwise(algo, args, batch):
    """oracle_batch's arrays from one oracle_align per pair, which also tells the pairs with rc == -3
    (oracle_batch reports one status for the whole batch)."""
    s1, o1, s2, o2 = batch
    n = len(o1) - 1
    res = np.zeros(n, dtype=ORACLE_RESULT_DTYPE)
    ops = np.zeros(int(o1[-1] + o2[-1]) + n + 1, dtype=np.uint8)
    div = []
    for p in range(n):
        o = oracle_align(algo, args, s1[int(o1[p]):int(o1[p + 1])].tobytes(), s2[int(o2[p]):int(o2[p + 1])].tobytes())
        assert o["rc"] in (0, -3), (algo, args, p, o["rc"])
        if o["rc"] == -3:
            div.append(p)
        res[p] = (o["score"], o["end_i"], o["end_j"], o["start_i"], o["start_j"], len(o["ops"]), 0)
        off = int(o1[p] + o2[p]) + p
        ops[off:off + len(o["ops"])] = np.frombuffer(o["ops"], dtype=np.uint8)
    return res, ops, div


def oracle(name, algo, args, batch):
    """The oracle's results and op streams of a named batch, computed once and read-only."""
    key = (name, algo, args)
    if key not in _ORACLE:
        if (algo, args) == REGIME_DIVERGING:
            res, ops, _DIVERGED[key] = oracle_pairwise(algo, args, batch)
        else:
            res, ops = oracle_batch(algo, args, *batch)
        res.setflags(write=False)
        ops.setflags(write=False)
        _ORACLE[key] = (res, ops)
    return _ORACLE[key]


def op_bytes(nops, ops, o1, o2):
    """The op streams of all pairs, concatenated (pair p's nops[p] bytes from o1[p] + o2[p] + p)."""
    n = len(nops)
    nops = nops.astype(np.int64)
    starts = o1[:n].astype(np.int64) + o2[:n].astype(np.int64) + np.arange(n)
    first = np.concatenate([[0], np.cumsum(nops)[:-1]])
    return ops[np.repeat(starts - first, nops) + np.arange(int(nops.sum()))]


def assert_exact(got, exp, batch, what, exempt=()):
    """Every field and op stream of got (results, ops, ...) equals the oracle's; flags are 0.  Pairs in
    `exempt` (the oracle's walk found no move) are compared on score and end cell alone."""
    res, ops = got[0], got[1]
    eres, eops = exp
    o1, o2 = batch[1], batch[3]
    keep = np.ones(len(res), dtype=bool)
    keep[list(exempt)] = False
    shape = lambda p: (int(p), int(o1[p + 1] - o1[p]), int(o2[p + 1] - o2[p]))
    for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops"):
        ok = res[f].astype(np.int64) == eres[f].astype(np.int64)
        if f in ("start_i", "start_j", "nops"):
            ok |= ~keep
        bad = np.nonzero(~ok)[0]
        assert len(bad) == 0, (what, f, [(shape(p), int(res[f][p]), int(eres[f][p])) for p in bad[:5]])
    bad = np.nonzero(res["flags"] != np.where(keep, 0, sa.SA_FLAG_DIVERGED))[0]
    assert len(bad) == 0, (what, "flags", [(shape(p), int(res["flags"][p])) for p in bad[:5]])
    nops = np.where(keep, eres["nops"], 0)
    a, b = op_bytes(nops, ops, o1, o2), op_bytes(nops, eops, o1, o2)
    if not np.array_equal(a, b):
        ends = np.cumsum(nops.astype(np.int64))
        p = int(np.searchsorted(ends, int(np.nonzero(a != b)[0][0]), side="right"))
        raise AssertionError((what, "op stream", shape(p)))


def check(engine, name, algo, args, batch, kernels, env=None, what=None):
    got = run(engine, algo, args, batch, env)
    assert got[2][0] in kernels, (what or name, algo, args, env, got[2])
    exp = oracle(name, algo, args, batch)
    assert_exact(got, exp, batch, (what or name, algo, args, env), _DIVERGED.get((name, algo, args), ()))
    return got


def check_score(engine, name, algo, args, batch, kernels):
    """sa_score_batch: score and end cell against the oracle, and the record-free contract fields."""
    res = engine.score_packed(algo, sa.ScoringSystem(*args), *batch).copy()
    plan = engine.last_plan_ex()
    assert plan[0] in kernels, (name, algo, args, plan)
    assert plan[3] in (sa.SA_RECORDS_NONE, sa.SA_RECORDS_SCORE_ONLY, sa.SA_RECORDS_TAGS), plan
    assert engine.last_timings()[1] == 0   # no traceback ran
    exp = oracle(name, algo, args, batch)[0]
    for f in ("score", "end_i", "end_j"):
        bad = np.nonzero(res[f].astype(np.int64) != exp[f].astype(np.int64))[0]
        assert len(bad) == 0, (name, algo, args, f, [(int(p), int(res[f][p]), int(exp[f][p])) for p in bad[:5]])
    assert (res["start_i"] == -1).all() and (res["start_j"] == -1).all()
    assert (res["nops"] == 0).all() and (res["reserved"] == 0).all() and (res["flags"] == 0).all()
    return res


def bounds(batch):
    return int(np.diff(batch[1]).max()), int(np.diff(batch[3]).max())


def no_hack(pairs):
    """No pair of a LocalGotoh size-hack shape (SALocalGotoh.h:484-488: parity unpinned there)."""
    assert not any((len(a), len(b)) in LG_HACK_SIZES for a, b in pairs)
    return pairs


@pytest.fixture(autouse=True)
def _f16_cell_on(request):
    """A launch that flags many pairs turns the f16 cell off for the context (sa_api.hip); every
    test here starts, and leaves the session's engine, with it on."""
    if "engine" not in request.fixturenames:
        yield
        return
    engine = request.getfixturevalue("engine")
    engine.test_hook(sa.SA_HOOK_F16, 0)
    yield
    engine.test_hook(sa.SA_HOOK_F16, 0)


# ----------------------------------------------------------------------------------- a. golden
REG = load_regimes()


@pytest.mark.parametrize("tiny", ["0", "1"], ids=["batch", "small-call"])
def test_golden_regimes(engine, monkeypatch, tiny):
    """The reference's own vectors on the batch kernels and on the small-call kernel; on a record
    the reference was not run on (its walk does not end) the engine reports SA_FLAG_DIVERGED and the
    oracle's score and end cell."""
    monkeypatch.setenv("SEQALIB_TINY", tiny)
    groups = {}
    for e in REG:
        groups.setdefault((e["algo"], tuple(e["scoring"])), []).append(e)
    n = nd = 0
    for (algo, args), es in groups.items():
        n += check_golden(engine, [e for e in es if not e.get("diverged")])
        if ALGOS[algo] <= GG:
            kern = engine.last_plan()[0]
            assert (kern == sa.SA_KERNEL_TINY) == (tiny == "1"), (algo, args, kern)
        div = [e for e in es if e.get("diverged")]
        if div:
            pairs = [golden_sequences(e) for e in div]
            for (a, b), r in zip(pairs, engine.align(ALGOS[algo], sa.ScoringSystem(*args), pairs)):
                o = oracle_align(ALGOS[algo], args, a, b)
                assert o["rc"] == -3 and r.flags == sa.SA_FLAG_DIVERGED, (algo, args, len(a), len(b))
                assert (r.score, r.end_i, r.end_j) == (o["score"], o["end_i"], o["end_j"])
                nd += 1
    assert n > 2500 and nd > 0 and n + nd == len(REG)


@pytest.mark.parametrize("algo", [SW, NW, LG, GG])
def test_small_call_kernel_all_regimes(engine, monkeypatch, algo):
    """The small-call kernel (one launch per host call of <= 64 short pairs) up to its shape limits
    (256 rows, 1,024 columns, 32,768 cells), every scoring."""
    from test_gpu_tiny import small_pairs as tiny_pairs
    monkeypatch.setenv("SEQALIB_TINY", "1")
    pairs = [p for p in tiny_pairs(50 + algo, 64) if (len(p[0]), len(p[1])) not in LG_HACK_SIZES]
    batch = pack_bytes(pairs)
    assert bounds(batch)[0] > 200 and bounds(batch)[1] > 900
    for args in (REGIME_LINEAR if algo <= NW else REGIME_AFFINE):
        check(engine, f"tiny{algo}", algo, args, batch, (sa.SA_KERNEL_TINY,))


# ------------------------------------------------------------------------ b. many-pairs plans
def many_pairs(long):
    """1,030 DNA pairs of 100..300 symbols, odd ones mutated relatives and even ones unrelated, and
    fourteen edge shapes; with
    `long`, a 4,200 x 3,100 random pair (three bands at R = 32), a 2,100-long related pair, a
    periodic pair and an all-mismatch 2,500 x 2,000 pair (test_endcell_replay_vs_oracle's shape)."""
    pairs = []
    for k in range(1030):
        m, n = 100 + (k * 37) % 201, 100 + (k * 53) % 201
        if k % 2:
            a = sa.synth_dna(300_000 + 2 * k, 110 + (k * 37) % 171)
            b = sa.synth_mutate(a, k)[:300]
        else:
            a, b = sa.synth_dna(300_000 + 2 * k, m), sa.synth_dna(300_001 + 2 * k, n)
        pairs.append((a, b))
    # edge shapes: empty sides, single symbols, lane-block boundaries; homopolymers (all one score),
    # periodic and identical pairs (tied maxima in every row and chunk)
    d = lambda k, n: sa.synth_dna(310_000 + k, n)
    pairs[20:29] = [(b"", d(0, 5)), (d(1, 5), b""), (b"", b""), (d(2, 1), d(3, 300)), (d(4, 300), d(5, 1)), (b"G", b"G"),
                    (d(6, 63), d(7, 64)), (d(8, 64), d(9, 63)), (d(10, 65), d(11, 65))]
    pairs[30:35] = [(b"A" * 70, b"C" * 50), (b"A" * 40, b"A" * 37), (b"AC" * 40, b"CA" * 45), (d(12, 97), d(12, 97)),
                    (b"ACGT" * 16, b"ACGT" * 15)]
    if long:
        pairs[7] = (sa.synth_dna(1, 4200), sa.synth_dna(2, 3100))
        pairs[11] = (sa.synth_dna(3, 2100), sa.synth_mutate(sa.synth_dna(3, 2100), 9))
        pairs[13] = (b"ACGT" * 1050, b"ACGT" * 700)
        pairs[17] = (b"A" * 2500, b"C" * 2000)
    return no_hack(pairs)


@pytest.fixture(scope="module")
def many():
    return {"long": pack_bytes(many_pairs(True)), "short": pack_bytes(many_pairs(False))}


def many_cases():
    """(algorithm, scoring, batch): every scoring on the batch with the long pairs, and again on the
    short batch where the long pairs alone send it to the int32 kernel."""
    out = []
    for algo in (SW, NW, LG, GG):
        for args in (REGIME_LINEAR if algo <= NW else REGIME_AFFINE):
            out.append((algo, args, "long"))
            if expected_kernels(algo, args, 4200, 3100) != expected_kernels(algo, args, 300, 300):
                out.append((algo, args, "short"))
    return out


# What the rules give at 4,200 x 3,100 and at 300 x 300, written out (the functions above restate
# the rules; these sets pin what they must come to for the scorings of this module).
T16_LONG = {SW: LIN_T16 - {(-3, 31, -32), (-4096, 31, -32)},   # keyed_ok: 31 * 3,100 >= 65,536
            NW: (LIN_T16 | LIN_T16_GAP0) - {(-3, 31, -32), (-4096, 31, -32)},   # NW window: (31 + 32) * 3,100
            LG: AFF_T16,
            GG: {(-3, -1, 0, -1, True), (-3, -1, 1, 0, True), (-3, -1, 1, 1, True), (-3, -1, 0, -1, False),
                 (-3, -1, 2, 2, True)}}
T16_SHORT = {SW: LIN_T16, NW: (LIN_T16 | LIN_T16_GAP0) - {(-4096, 31, -32)}, LG: AFF_T16,
             # match < 0: int32; gap_open -2048: the -10000 border rule
             GG: AFF_T16 - {(-3, -1, -1, -2, True), (-2048, -512, 15, -16, True)}}


def test_expected_kernel_tables():
    for algo in (SW, NW, LG, GG):
        for args in (REGIME_LINEAR if algo <= NW else REGIME_AFFINE):
            assert (expected_kernels(algo, args, 4200, 3100) == T16) == (args in T16_LONG[algo]), (algo, args)
            assert (expected_kernels(algo, args, 300, 300) == T16) == (args in T16_SHORT[algo]), (algo, args)
            # the engine's own answer for a four-symbol batch (no GPU work)
            for (m, n), tab in (((4200, 3100), T16_LONG), ((300, 300), T16_SHORT)):
                k = sa.plan_query_ex(algo, sa.ScoringSystem(*args), m, n, 1030)[0]
                assert (k in T16) == (args in tab[algo]), (algo, args, m, n, k)
            for m, n in ((700, 700), (2600, 2600), (1998, 40), (40, 1999)):   # few pairs
                k = sa.plan_query_ex(algo, sa.ScoringSystem(*args), m, n, 50)[0]
                assert (k in T16) == (expected_kernels(algo, args, m, n, False) == T16), (algo, args, m, n, k)


SW_CELLS = [{"SEQALIB_SO2_F16": "0"}, {"SEQALIB_SO2_F16": "5"}, {"SEQALIB_SO2": "0"}, {"SEQALIB_SO": "0"},
            {"SEQALIB_CMAX": "0"}]
OTHER_CELLS = [{"SEQALIB_SO": "0"}, {"SEQALIB_T16": "0"}]


@pytest.mark.parametrize("algo,args,size", many_cases(), ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_many_pairs_plans(engine, many, algo, args, size):
    """>= 1,024 pairs, one wave per pair (or two): the default kernel, then -- where that is a 16-bit
    kernel -- the other cells and record kinds of the same fill: SW with the 16-bit integer cell and
    the 5-op f16 cell in place of the 4-op scaled-f16 one, one pair per wave, tagged records and
    per-cell keys; NW and Gotoh with tagged records and on the int32 kernel.  All equal the oracle,
    hence each other."""
    batch = many[size]
    m, n = bounds(batch)
    kernels = expected_kernels(algo, args, m, n)
    got = check(engine, size, algo, args, batch, kernels)
    if kernels == T16:
        if size == "long" and algo in (SW, NW):
            assert got[2][1:3] == (32, 1), got[2]
        for env in (SW_CELLS if algo == SW else OTHER_CELLS):
            check(engine, size, algo, args, batch, INT32 if env.get("SEQALIB_T16") == "0" else T16, env)


# ------------------------------------------------------------------- e. score-only calls (of b)
@pytest.mark.parametrize("algo,args,size", many_cases(), ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_many_pairs_score_calls(engine, many, algo, args, size):
    batch = many[size]
    check_score(engine, size, algo, args, batch, expected_kernels(algo, args, *bounds(batch)))


# ------------------------------------------------------------------------------ c. thresholds
def rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def with_pairs(first):
    """The short many-pairs batch with its first pairs replaced."""
    pairs = list(first) + many_pairs(False)[len(first):]
    return pack_bytes(no_hack(pairs))


def test_f16_cell_threshold_positive_mismatch(engine):
    """(-2, 2, 2): every pair of equal length L scores 2 L whatever its symbols.  L = 990 and 1,000
    stay within the f16 cell's 2,000; 1,010 and 1,100 pass it and re-run in int32.  Exact either
    way, against the integer cell too, and four flagged pairs of 1,030 leave the cell on."""
    rng = np.random.default_rng(3)
    lengths = [990, 1000, 1010, 1100]
    batch = with_pairs([(rnd(rng, L), rnd(rng, L)) for L in lengths])
    args = (-2, 2, 2)
    got = check(engine, "f16", SW, args, batch, T16)
    assert got[2][1] in (16, 32) and got[2][3] == sa.SA_RECORDS_SCORE_ONLY   # two pairs per wave
    assert [int(s) for s in got[0]["score"][:4]] == [2 * L for L in lengths]
    check(engine, "f16", SW, args, batch, T16, {"SEQALIB_SO2_F16": "0"})
    check(engine, "f16", SW, args, batch, T16)
    assert engine.test_hook(sa.SA_HOOK_F16, 2) == 0
    check_score(engine, "f16", SW, args, batch, T16)


@pytest.mark.parametrize("args", [(-3, 31, -32), (-4096, 31, -32)], ids=ident)
def test_t16_sw_retry_at_match_31(engine, args):
    """Identical pairs of 270 (8,370 > 8191 - 31: re-run on int32) and 250 (7,750: not)."""
    rng = np.random.default_rng(5)
    a, b = rnd(rng, 270), rnd(rng, 250)
    batch = with_pairs([(a, a), (b, b)])
    got = check(engine, "m31", SW, args, batch, T16)
    assert [int(s) for s in got[0]["score"][:2]] == [31 * 270, 31 * 250]
    check_score(engine, "m31", SW, args, batch, T16)
    check(engine, "m31", NW, args, batch, expected_kernels(NW, args, *bounds(batch)))


def test_t16_local_gotoh_retry_at_match_15(engine):
    """(-3, -1, 15, -16): identical pairs of 270 (4,050) and 280 (4,200) around 4095 - 15."""
    rng = np.random.default_rng(6)
    a, b = rnd(rng, 270), rnd(rng, 280)
    batch = with_pairs([(a, a), (b, b)])
    args = (-3, -1, 15, -16, True)
    got = check(engine, "m15", LG, args, batch, T16)
    assert [int(s) for s in got[0]["score"][:2]] == [4050, 4200]
    check_score(engine, "m15", LG, args, batch, T16)
    check(engine, "m15", GG, args, batch, expected_kernels(GG, args, *bounds(batch)))


def small_pairs(rng, count, top):
    pairs = []
    for k in range(count):
        m, n = int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))
        if (m, n) in LG_HACK_SIZES:
            n += 1 if n < top else -1
        a = rnd(rng, m)
        pairs.append((a, (a + rnd(rng, n))[:n] if k % 2 else rnd(rng, n)))
    return pairs


@pytest.mark.parametrize("algo,args", [(SW, (-700, 1000, -900)), (LG, (-6000, -5000, 1000, -900, True))],
                         ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("top", [65, 66])
@pytest.mark.parametrize("count", [5, 1030])
def test_keyed_bound_large_match(engine, algo, args, top, count):
    """keyed_ok's match * min(m, n) < 65,536 with match 1,000: batches whose longest pair is an
    identical pair of 65 (keys hold 65,000) and of 66 (they do not), few pairs and many."""
    rng = np.random.default_rng(100 * top + count)
    a = rnd(rng, top)
    batch = pack_bytes(no_hack([(a, a)] + small_pairs(rng, count - 1, top)))
    assert keyed_fits(algo, args, *bounds(batch)) == (top == 65)
    got = check(engine, f"key{top}x{count}", algo, args, batch, INT32)
    assert int(got[0]["score"][0]) == 1000 * top
    check_score(engine, f"key{top}x{count}", algo, args, batch, INT32)


@pytest.mark.parametrize("args,long_m", [((-1, 2, 1), 16300), ((-1, 2, 1), 16301), ((1, 1, -1), 21745), ((1, 1, -1), 21746)],
                         ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_keyed_bound_positive_terms(engine, args, long_m):
    """keyed_ok with a positive mismatch or gap: (|match| + |mismatch| + |gap|) * (m + n) < 65,536.
    One long thin pair puts the batch on either side of it: 4 * (16,300 + 83) = 65,532 and
    3 * (21,745 + 100) = 65,535 keep the keys, one symbol more does not.  (-1, 2, 1) leaves the
    16-bit kernel with them; (1, 1, -1) is on the int32 kernel on both sides."""
    n = 83 if args == (-1, 2, 1) else 100
    base = many_pairs(False)
    pairs = [(a[:n], b[:n]) for a, b in base]
    pairs[7] = (sa.synth_dna(7, long_m), sa.synth_mutate(sa.synth_dna(7, long_m), 3)[4000:4000 + n])
    batch = pack_bytes(no_hack(pairs))
    assert bounds(batch) == (long_m, n)
    keyed = keyed_fits(SW, args, long_m, n)
    assert keyed == (long_m in (16300, 21745))
    kernels = T16 if args == (-1, 2, 1) and keyed else INT32
    name = f"pos{long_m}"
    check(engine, name, SW, args, batch, kernels)
    check_score(engine, name, SW, args, batch, kernels)


def thin_pairs(longest):
    return [(sa.synth_dna(11, longest), sa.synth_dna(12, 40)), (sa.synth_dna(13, 40), sa.synth_dna(14, longest))]


@pytest.mark.parametrize("longest", [1000, 1998, 1999, 2100])
def test_global_gotoh_border_rule(engine, longest):
    """GlobalGotoh (-3, -5, 1, -1): the reference's -10000 Ix / Iy border wins a cell once
    GO + max(m, n) GE + GOE <= -10000 + GE, i.e. from a longest side of 1,999 (never at 1,998, always
    at 2,100), and such shapes must run the int32 kernel, which keeps the border.  At 1,998 the border
    rule of t16_mode_affine admits the shape, but its window rule does not (the border column alone
    spans 9,993), so only the 1,000-long shape runs the 16-bit kernel.  Tall and wide, one call each
    and both in one call, align and score calls."""
    args = (-3, -5, 1, -1, True)
    pairs = thin_pairs(longest)
    for name, sub in (("tall", pairs[:1]), ("wide", pairs[1:]), ("both", pairs)):
        batch = pack_bytes(sub)
        m, n = bounds(batch)
        kernels = expected_kernels(GG, args, m, n)
        assert (kernels == T16) == (longest == 1000)
        check(engine, f"border{longest}{name}", GG, args, batch, kernels)
        check_score(engine, f"border{longest}{name}", GG, args, batch, kernels)


@pytest.mark.parametrize("allow", [True, False])
def test_gotoh_huge_gap_terms(engine, allow):
    """(-6000, -5000, 1, -1): gap terms past the 16-bit rules and past the -10000 border, 300 x 280."""
    args = (-6000, -5000, 1, -1, allow)
    a = sa.synth_dna(21, 300)
    batch = pack_bytes([(a, sa.synth_mutate(a, 2)[:280]), (sa.synth_dna(22, 300), sa.synth_dna(23, 280))])
    for algo in (LG, GG):
        check(engine, "huge", algo, args, batch, INT32)
        check_score(engine, "huge", algo, args, batch, INT32)


# ------------------------------------------------------------------ d. few pairs, forced plans
def few_batch():
    a, b = sa.synth_dna(31, 2600), sa.synth_dna(33, 1030)
    pairs = [(a, sa.synth_mutate(a, 5)[:2300]), (b, sa.synth_dna(34, 120))]
    return pack_bytes(pairs + [(y, x) for x, y in pairs])


FEW = [(SW, (-1, 1, 1), T16), (NW, (-1, 1, 1), T16), (SW, (-1, 0, -1), T16), (NW, (-1, 0, -1), T16), (NW, (0, 1, 0), T16),
       (SW, (1, 1, -1), INT32), (NW, (1, 1, -1), INT32), (LG, (-3, -1, 1, 1, True), T16), (GG, (-3, -1, 1, 1, True), T16),
       (LG, (-3, 0, 1, -1, True), INT32), (GG, (-3, 0, 1, -1, True), INT32)]
SETTINGS = [None] + [("SEQALIB_PLAN", p) for p in ("1,0", "4,0", "8,1", "16,1", "8,3", "16,16")] + \
           [("SEQALIB_SPLIT", "0")] + [("SEQALIB_TB", t) for t in ("lane", "wave", "seg")]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "default" if s is None else "=".join(s))
def test_few_pairs_forced_plans(engine, setting):
    """Two long pairs and their transposes: the multi-workgroup band plan (default; R forced to 1
    and 4), the single-workgroup plans, and the three traceback walks."""
    batch = few_batch()
    env = dict([setting]) if setting else {}
    for algo, args, kernels in FEW:
        got = check(engine, "few", algo, args, batch, kernels, env)
        plan = got[2]
        if setting and setting[0] == "SEQALIB_PLAN":
            r, w = (int(x) for x in setting[1].split(","))
            bands = -(-bounds(batch)[0] // (64 * r))   # make_plan: never more waves than bands
            assert plan[1:3] == (r, min(w, bands)), (algo, args, plan)
        elif setting and setting[0] == "SEQALIB_SPLIT":
            assert plan[2] > 0, (algo, args, plan)
        else:
            assert plan[2] == 0, (algo, args, plan)   # the band plan


@pytest.mark.parametrize("algo", [LG, GG])
def test_few_pairs_ragged_affine(engine, algo):
    """Every affine scoring on a ragged batch of few pairs (every edge length up to 700; the band
    plan with its default R): the 16-bit affine kernel where the rules admit it, int32 elsewhere.
    (The linear scorings on the same plan: test_whole_matrix_band_equals_full_path.)"""
    from test_gpu_submat import drop_hack_sizes
    pairs = drop_hack_sizes(algo, ragged_pairs(11, ACGT)[::2])
    batch = pack_bytes(pairs)
    m, n = bounds(batch)
    ran = set()
    for args in REGIME_AFFINE:
        kernels = expected_kernels(algo, args, m, n, False)
        got = check(engine, f"half{algo}", algo, args, batch, kernels)
        assert got[2][2] == 0, got[2]   # the band plan
        ran.add(kernels)
    assert ran == {T16, INT32}


# ---------------------------------------------------------------------- f. banded and matrix calls
@pytest.fixture(scope="module")
def ragged_dna():
    return ragged_pairs(11, ACGT)   # test_gpu_banded.py's batch


@pytest.mark.parametrize("algo", [NW, SW])
@pytest.mark.parametrize("args", REGIME_LINEAR, ids=ident)
def test_whole_matrix_band_equals_full_path(engine, ragged_dna, algo, args):
    batch = pack_bytes(ragged_dna)
    o1, o2 = batch[1], batch[3]
    sc = sa.ScoringSystem(*args)
    full = check(engine, "ragged", algo, args, batch, expected_kernels(algo, args, *bounds(batch)))
    band, bops = engine.align_banded_packed(algo, sc, *batch, 4096)
    assert engine.last_plan_ex()[0] == sa.SA_KERNEL_BANDED
    for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops", "flags", "reserved"):
        assert np.array_equal(full[0][f], band[f]), (algo, args, f)
    assert_exact((band, bops), oracle("ragged", algo, args, batch), batch, ("band", algo, args))
    score = engine.score_banded_packed(algo, sc, *batch, 4096)
    for f in ("score", "end_i", "end_j"):
        assert np.array_equal(score[f], band[f]), (algo, args, f)
    assert (score["start_i"] == -1).all() and (score["start_j"] == -1).all() and (score["nops"] == 0).all()
    assert (score["flags"] == 0).all() and (score["reserved"] == 0).all()


def narrow_pairs():
    rng = np.random.default_rng(8)
    pairs = [(b"", b""), (b"A", b""), (b"", b"CA"), (b"A", b"A")]
    for m, n in ((7, 9), (33, 31), (64, 70), (80, 80), (75, 12)):
        a = rnd(rng, m)
        b = bytearray((a + rnd(rng, n))[:n])
        for p in rng.integers(0, n, n // 5):
            b[p] = ACGT[rng.integers(0, 4)]
        pairs.append((a, bytes(b)))
    return pairs


@pytest.mark.parametrize("algo", [NW, SW])
@pytest.mark.parametrize("args", [(-1, 1, 1), (-1, 0, -1), (0, 1, 0), (1, 1, -1), (-1, 1, 2)], ids=ident)
def test_narrow_band_matches_model(engine, algo, args):
    pairs = narrow_pairs()
    batch = pack_bytes(pairs)
    for w in (0, 1, 3, 32, 65):
        res, ops = engine.align_banded_packed(algo, sa.ScoringSystem(*args), *batch, w)
        assert engine.last_plan_ex()[0] == sa.SA_KERNEL_BANDED
        score = engine.score_banded_packed(algo, sa.ScoringSystem(*args), *batch, w)
        for p, (a, b) in enumerate(pairs):
            want = banded_model(algo, args, a, b, w)
            r = res[p]
            got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
                   pair_ops(res, ops, batch[1], batch[3], p))
            assert got == want, (algo, args, w, p, len(a), len(b))
            assert int(r["flags"]) == 0 and int(r["reserved"]) == 0
            assert (int(score["score"][p]), int(score["end_i"][p]), int(score["end_j"][p])) == want[:3], (algo, args, w, p)


def matrix_scorings(algo):
    """Matrix calls score every cell from the table (allow_mismatch = 1) with int16 entries."""
    return [s for s in (REGIME_LINEAR if algo <= NW else REGIME_AFFINE)
            if scoring_fields(s)[5] and (algo, s) != REGIME_DIVERGING]


@pytest.mark.parametrize("algo", [SW, NW, LG, GG])
def test_degenerate_table_equals_align_batch(engine, monkeypatch, algo):
    """sa_align_batch_matrix with table[a][b] = (a == b ? match : mismatch) equals sa_align_batch on
    the int32 kernel, field for field and op for op, and the oracle, for every regime scoring that
    allows mismatches."""
    from test_gpu_submat import compare_with_align_batch, drop_hack_sizes
    monkeypatch.setenv("SEQALIB_T16", "0")
    pairs = drop_hack_sizes(algo, ragged_pairs(11, ACGT)[::3])
    batch = pack_bytes(pairs)
    for args in matrix_scorings(algo):
        compare_with_align_batch(engine, algo, args, pairs)
        check(engine, f"third{algo}", algo, args, batch, INT32)


def test_matrix_call_rejects_wrapping_scoring(engine):
    """(m + n + 1) * max(|gap terms|, max |S|) >= 2^29: SA_ERR_UNSUPPORTED (include/seqalib_hip.h)."""
    pairs = [(b"ACGT" * 8, b"ACGA" * 8)]
    tab = np.where(np.eye(256, dtype=bool), 1, -1).astype(np.int16)
    with pytest.raises(sa.SeqalibError, match="unsupported"):
        engine.align_matrix_packed(SW, sa.ScoringSystem(-(2 ** 29) // 64, 1, -1), *pack_bytes(pairs), tab, None)


# --------------------------------------------------------------------------- g. linear space
def dc_pairs(count, top, seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(count):
        m = int(rng.integers(0, top)) if k % 4 else int(rng.integers(0, 4))
        n = int(rng.integers(0, top)) if k % 5 else int(rng.integers(0, 4))
        a = sa.synth_dna(70_000 + 2 * k, m)
        pairs.append((a, sa.synth_mutate(a, k)[:n] if k % 2 else sa.synth_dna(70_001 + 2 * k, n)))
    return pairs


@pytest.fixture(scope="module")
def dc_batches():
    """big: 40 pairs up to 900 long and one 2,048 x 2,048 pair; small: 40 pairs up to 200 long, where
    the value range of match 127 still fits the 16-bit sweeps."""
    return {"big": pack_bytes(dc_pairs(40, 900, 19) + [(sa.synth_dna(5, 2048), sa.synth_dna(6, 2048))]),
            "small": pack_bytes(dc_pairs(40, 200, 20) + [(sa.synth_dna(7, 200), sa.synth_dna(8, 200))])}


@pytest.mark.parametrize("size", ["big", "small"])
@pytest.mark.parametrize("algo,args", [(HB, s) for s in REGIME_LINEAR] + [(MM, s) for s in REGIME_AFFINE],
                         ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_linear_space_vs_oracle(engine, dc_batches, algo, args, size):
    """Hirschberg / Myers-Miller by default (the 16-bit sweeps where dc16_plan, sa_dc.h, admits the
    scoring -- match 0..127, mismatch -128..match, gap terms <= 0 -- and the batch's value range: match
    127 fits at 200 x 200, not at 2,048 x 2,048) and with SEQALIB_DC16=0 (every sweep on int32): both
    equal the oracle.  No call reports which sweep ran, so none is asserted."""
    batch = dc_batches[size]
    exp = oracle("dc" + size, algo, args, batch)
    for env in ({}, {"SEQALIB_DC16": "0"}):
        assert_exact(run(engine, algo, args, batch, env), exp, batch, ("dc", size, algo, args, env))


# ------------------------------------------------------------------------------ h. divergence
def diverging_pairs():
    rng = np.random.default_rng(23)
    pairs = [(b"ACGT", b"ACGT"), (b"A" * 40, b"A" * 37), (b"A" * 33, b"C" * 35), (b"AC" * 20, b"CA" * 17)]
    while len(pairs) < 60:
        k = len(pairs)
        m, n = int(rng.integers(1, 200 if k % 8 else 420)), int(rng.integers(1, 160))   # a few pairs of two bands
        a = rnd(rng, m)
        pairs.append((a, sa.synth_mutate(a, k)[:n] if k % 2 else rnd(rng, n)))
    return no_hack([p for p in pairs if p[1]])


DIVERGE_WALKS = [{"SEQALIB_TB": "lane"}, {"SEQALIB_TB": "wave"}, {"SEQALIB_TB": "seg"}, {"SEQALIB_TINY": "1"},
                 {"SEQALIB_PLAN": "4,1"}, {}]


def test_divergence(engine):
    """LocalGotoh (-3, 1, 1, -1): with gap_extend > 0 the reference's walk can reach a cell none of
    its branches leaves.  The oracle decides which pairs (rc == -3); exactly those carry
    SA_FLAG_DIVERGED, with the oracle's score and end cell, on every walk kernel; every other pair
    is exact; the score call never flags."""
    algo, args = REGIME_DIVERGING
    pairs = diverging_pairs()
    batch = pack_bytes(pairs)
    ora = [oracle_align(algo, args, a, b) for a, b in pairs]
    div = [p for p, o in enumerate(ora) if o["rc"] == -3]
    assert all(o["rc"] in (0, -3) for o in ora) and 0 < len(div) < len(pairs)
    small = [p for p, (a, b) in enumerate(pairs) if len(a) <= 256 and len(a) * len(b) <= 32768]   # small-call limits
    assert set(div) & set(small) and len(small) < len(pairs)
    for env in DIVERGE_WALKS:
        tiny = env.get("SEQALIB_TINY") == "1"
        idx = small if tiny else list(range(len(pairs)))
        sub = pack_bytes([pairs[p] for p in idx])
        res, ops, plan = run(engine, algo, args, sub, env)
        assert plan[0] == (sa.SA_KERNEL_TINY if tiny else sa.SA_KERNEL_INT32), (env, plan)
        if env.get("SEQALIB_TB") == "seg" or not env:
            assert plan[2] == 0, (env, plan)   # the band plan, whose fills the segmented walk follows
        for q, p in enumerate(idx):
            o, r = ora[p], res[q]
            where = (env, p, len(pairs[p][0]), len(pairs[p][1]))
            assert (int(r["score"]), int(r["end_i"]), int(r["end_j"])) == (o["score"], o["end_i"], o["end_j"]), where
            assert int(r["flags"]) == (sa.SA_FLAG_DIVERGED if p in div else 0), where
            if p not in div:
                assert (int(r["start_i"]), int(r["start_j"]), pair_ops(res, ops, sub[1], sub[3], q)) == \
                       (o["start_i"], o["start_j"], o["ops"]), where
    score = engine.score_packed(algo, sa.ScoringSystem(*args), *batch)
    assert engine.last_plan_ex()[0] == sa.SA_KERNEL_INT32
    assert [(int(r["score"]), int(r["end_i"]), int(r["end_j"])) for r in score] == \
           [(o["score"], o["end_i"], o["end_j"]) for o in ora]
    assert (score["flags"] == 0).all() and (score["nops"] == 0).all() and (score["start_i"] == -1).all()
