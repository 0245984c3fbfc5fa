"""Banded X-drop extension (sa_align_batch_banded_extend, sa_score_batch_banded_extend) on the GPU.

Small shapes are compared field by field and op by op with tests/extend_model.py, a plain-dict restatement
of the header's contract that tests/test_extend_model.py pins on the CPU; the wide variants with its numpy
fill for score, end cell and flag, and for their ops with the existing seeded call on the GPU through the
header's equivalence (a).  The drop tests assert on the model what their inputs are meant to do (stop
early with the unstopped score, stop early with a lower one, not stop), so they cannot pass vacuously.
"""
import functools

import numpy as np
import pytest

import seqalib_amd as sa
from extend_model import extend_band, extend_fill_np, extend_model
from test_gpu_banded import ACGT, pair_ops, seq
from util import named_lut, pack_bytes, scoring_fields

pytestmark = pytest.mark.gpu

NW, HB, GG = sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH
OFF, DROPPED = sa.SA_XDROP_OFF, sa.SA_FLAG_DROPPED
# per algorithm: the issue's scoring, one outside gap < 0 < match, one without mismatches
SCORINGS = {NW: [(-2, 1, -3), (0, 1, -1), (-1, 2, -1, False)],
            GG: [(-4, -1, 1, -3), (0, 0, 1, -1), (-3, -1, 2, -1, False)]}
PURINE = named_lut("purine")
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals


def cells_per_lane(diagonals):
    return next(R for R, L in VARIANTS if diagonals <= 2 * R * L)


def run_align(engine, algo, args, pairs, w, xdrop, lut=None):
    s1, o1, s2, o2 = pack_bytes(pairs)
    res, ops = engine.align_banded_extend_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, w, xdrop, lut)
    return res, ops, o1, o2


def run_score(engine, algo, args, pairs, w, xdrop, lut=None):
    return engine.score_banded_extend_packed(algo, sa.ScoringSystem(*args), *pack_bytes(pairs), w, xdrop, lut)


@functools.lru_cache(maxsize=None)
def model(algo, args, a, b, w, xdrop, lut=False):
    """extend_model, computed once per input (several tests share pairs)."""
    return extend_model(algo, args, a, b, w, xdrop, PURINE if lut else None)


def check_model(engine, algo, args, pairs, w, xdrop, lut=False):
    """Align and score call against the model: every field, op and the flag exact, the score contract kept."""
    table = PURINE if lut else None
    res, ops, o1, o2 = run_align(engine, algo, args, pairs, w, xdrop, table)
    score = run_score(engine, algo, args, pairs, w, xdrop, table)
    for p, (a, b) in enumerate(pairs):
        want = model(algo, args, a, b, w, xdrop, lut)
        r = res[p]
        got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
               pair_ops(res, ops, o1, o2, p))
        where = (algo, args, w, xdrop, p, len(a), len(b))
        assert got == want[:6], where
        assert int(r["flags"]) == (DROPPED if want[6] else 0) and int(r["reserved"]) == 0, where
        s = score[p]
        assert (int(s["score"]), int(s["end_i"]), int(s["end_j"])) == want[:3], where
        assert (int(s["start_i"]), int(s["start_j"]), int(s["nops"]), int(s["reserved"])) == (-1, -1, 0, 0), where
        assert int(s["flags"]) == (DROPPED if want[6] else 0), where
    return res, ops


# ---------------------------------------------------------------------------- the inputs
def edited(rng, a, rate):
    """A copy of `a` with about `rate` of its symbols edited: half substituted, a quarter each inserted before
    and deleted."""
    b = bytearray()
    for ch in a:
        r = rng.random()
        if r < rate / 2:
            b.append(int(ACGT[(list(ACGT).index(ch) + 1 + rng.integers(0, 3)) % 4]))
        elif r < 3 * rate / 4:
            b.append(int(ACGT[rng.integers(0, 4)]))
            b.append(ch)
        elif r < rate:
            continue
        else:
            b.append(ch)
    return bytes(b)


def diverging(rng, head=48, tail=200):
    """A related head (4 % edits), then unrelated symbols."""
    a = seq(rng, ACGT, head)
    return a + seq(rng, ACGT, tail), edited(rng, a, 0.04) + seq(rng, ACGT, tail)


def island(rng):
    """30 related symbols, 40 unrelated ones, 150 related ones."""
    a1, a3 = seq(rng, ACGT, 30), seq(rng, ACGT, 150)
    return a1 + seq(rng, ACGT, 40) + a3, edited(rng, a1, 0.04) + seq(rng, ACGT, 40) + edited(rng, a3, 0.04)


def related_throughout(rng, n=200):
    a = seq(rng, ACGT, n)
    return a, edited(rng, a, 0.08)


def steps_swept(m, n, w, stop):
    tend = extend_band(m, n, w)[2]
    return (stop + 1) / (tend + 1)


# ---------------------------------------------------------------------------- 1. model parity
def ragged_batch(seed, count=19):
    rng = np.random.default_rng(seed)
    pairs = [(b"", b""), (b"A", b""), (b"", b"AB")]
    while len(pairs) < count:
        a = seq(rng, ACGT, int(rng.integers(0, 41)))
        n = int(rng.integers(0, 41))
        # a related prefix and an unrelated rest, so that small xdrops stop some pairs and not others
        k = int(rng.integers(0, min(len(a), n) + 1))
        pairs.append((a, edited(rng, a[:k], 0.1)[:n] + seq(rng, ACGT, max(0, n - k))))
    return pairs


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("w", [0, 1, 3, 8])
def test_ragged_batches_match_the_model(engine, algo, w):
    stopped = 0
    for n_s, args in enumerate(SCORINGS[algo]):
        if w == 0 and not scoring_fields(args)[5]:   # one diagonal needs allow_mismatch: the contract's status
            with pytest.raises(sa.SeqalibError):
                run_score(engine, algo, args, [(b"ACGT", b"ACGT")], 0, 5)
            continue
        pairs = ragged_batch(100 * w + n_s)
        assert all(len(a) <= 40 and len(b) <= 40 for a, b in pairs)
        for xdrop in (OFF, 0, 2, 5, 1000):
            check_model(engine, algo, args, pairs, w, xdrop)
            check_model(engine, algo, args, pairs, w, xdrop, lut=True)
            stopped += sum(model(algo, args, a, b, w, xdrop)[6] for a, b in pairs)
    assert stopped > 0 or w == 0


def test_hirschberg_means_nw(engine):
    pairs = ragged_batch(5)
    a, aops = run_align(engine, HB, (-2, 1, -3), pairs, 3, 2)[:2]
    b, bops = run_align(engine, NW, (-2, 1, -3), pairs, 3, 2)[:2]
    assert a.tobytes() == b.tobytes() and aops.tobytes() == bops.tobytes()
    assert (a["flags"] == DROPPED).any()


# ---------------------------------------------------------------------------- 2. every variant
def variant_pairs(w):
    """(m = n = w + 200) related throughout, the same shape diverging after 60 symbols, and a shape clipped on
    the Seq1 side (m < w < n)."""
    rng = np.random.default_rng(w)
    n = w + 200
    a = seq(rng, ACGT, n)
    full = (a, (edited(rng, a, 0.05) + seq(rng, ACGT, 40))[:n])
    div = diverging(rng, 60, n - 60)
    m = min(40, w - 5)
    c = seq(rng, ACGT, m)
    clipped = (c, edited(rng, c, 0.05) + seq(rng, ACGT, w + 50 - m))
    return [full, (div[0][:n], div[1][:n]), clipped]


@pytest.mark.parametrize("algo,w", [(NW, w) for w in (15, 31, 63, 127, 255, 511, 1023, 2047)] +
                         [(GG, w) for w in (15, 31, 63, 127, 255, 511, 1023)])
def test_every_variant(engine, algo, w):
    args = (-2, 1, -3) if algo == NW else (-4, -1, 1, -3)
    pairs = variant_pairs(w)
    (a, b), _, (c, d) = pairs
    assert len(a) == len(b) == w + 200 and len(c) < w < len(d)
    assert sa.banded_extend_plan_query(algo, len(a), len(b), w)[0] == cells_per_lane(2 * w + 1)
    s1, o1, s2, o2 = pack_bytes(pairs)
    dropped = 0
    for xdrop in (OFF, 10):
        res, ops = engine.align_banded_extend_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, w, xdrop)
        assert engine.last_plan_ex()[1] == cells_per_lane(2 * w + 1)
        score = engine.score_banded_extend_packed(algo, sa.ScoringSystem(*args), s1, o1, s2, o2, w, xdrop)
        want = [extend_fill_np(algo, args, x, y, w, xdrop) for x, y in pairs]
        for p, (sc, ei, ej, drop, _) in enumerate(want):
            for r in (res[p], score[p]):
                assert (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["flags"])) == (sc, ei, ej, DROPPED if drop else 0), (w, xdrop, p)
            assert (int(res[p]["start_i"]), int(res[p]["start_j"])) == (0, 0)
            dropped += drop
        # equivalence (a): the seeded call on the prefixes that end in the end cell
        prefixes = [(x[:int(r["end_i"])], y[:int(r["end_j"])]) for (x, y), r in zip(pairs, res)]
        p1, q1, p2, q2 = pack_bytes(prefixes)
        sres, sops = engine.align_banded_seeded_packed(algo, sa.ScoringSystem(*args), p1, q1, p2, q2, [0] * len(pairs), w, 0)
        for p in range(len(pairs)):
            for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops"):
                assert int(res[p][f]) == int(sres[p][f]), (w, xdrop, p, f)
            assert pair_ops(res, ops, o1, o2, p) == pair_ops(sres, sops, q1, q2, p), (w, xdrop, p)
    assert dropped >= 1   # (the diverging pair stops under xdrop = 10)


# ---------------------------------------------------------------------------- 3. the drop fires
@functools.lru_cache(maxsize=None)
def drop_inputs():
    rng = np.random.default_rng(78)
    return ([diverging(rng) for _ in range(6)], [island(rng) for _ in range(6)], [related_throughout(rng) for _ in range(6)])


@pytest.mark.parametrize("algo", [NW, GG])
def test_diverging_pairs_stop_early_with_the_unstopped_score(engine, algo):
    args = SCORINGS[algo][0]
    pairs = drop_inputs()[0]
    for a, b in pairs:
        got, off = model(algo, args, a, b, 8, 10), model(algo, args, a, b, 8, OFF)
        assert got[6] and steps_swept(len(a), len(b), 8, got[7]) < 0.45
        assert got[0] == off[0] > 20
    res, _ = check_model(engine, algo, args, pairs, 8, 10)
    assert (res["flags"] == DROPPED).all()
    check_model(engine, algo, args, pairs, 8, OFF)


@pytest.mark.parametrize("algo", [NW, GG])
def test_island_pairs_stop_below_the_unstopped_score(engine, algo):
    args = SCORINGS[algo][0]
    pairs = drop_inputs()[1]
    for a, b in pairs:
        got, off = model(algo, args, a, b, 8, 10), model(algo, args, a, b, 8, OFF)
        assert got[6] and got[0] < off[0]
    res, _ = check_model(engine, algo, args, pairs, 8, 10)
    off, _ = check_model(engine, algo, args, pairs, 8, OFF)
    assert (res["flags"] == DROPPED).all() and (off["flags"] == 0).all() and (res["score"] < off["score"]).all()


@pytest.mark.parametrize("algo", [NW, GG])
def test_related_pairs_do_not_stop(engine, algo):
    args = SCORINGS[algo][0]
    pairs = drop_inputs()[2]
    for a, b in pairs:
        assert not model(algo, args, a, b, 8, 20)[6]
        assert model(algo, args, a, b, 8, 20)[:6] == model(algo, args, a, b, 8, OFF)[:6]
    res, _ = check_model(engine, algo, args, pairs, 8, 20)
    assert (res["flags"] == 0).all()


# ---------------------------------------------------------------------------- 4. the threshold
@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("w", [8, 7])
def test_threshold(engine, algo, w):
    """xdrop = best - recent - 1 at the stopping checkpoint stops there, xdrop = best - recent does not; also
    with one symbol put before both sequences, and with a band whose lo' has the other parity (w = 7)."""
    args = SCORINGS[algo][0]
    a, b = drop_inputs()[0][0]
    for x, y in ((a, b), (b"G" + a, b"G" + b)):
        trace = []
        stop = extend_model(algo, args, x, y, w, 10, trace=trace)[7]
        t, best, recent = trace[-1]
        g = best - recent
        assert stop == t and g > 10
        assert model(algo, args, x, y, w, g - 1)[7] == t
        after = model(algo, args, x, y, w, g)[7]
        assert after is None or after > t
        check_model(engine, algo, args, [(x, y)], w, g - 1)
        check_model(engine, algo, args, [(x, y)], w, g)


# ---------------------------------------------------------------------------- 5. - 7. mixed waves
@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Diverging, island, related and empty pairs interleaved, four pairs per wave, 23 pairs: neighbours of a
    stopped pair in every lane group, and a last wave that is not full."""
    div, isl, rel = drop_inputs()
    empty = [(b"", b""), (b"ACGT", b""), (b"", b"ACGTA"), (b"", b""), (b"C", b"C"), (b"", b"")]
    pairs = [kind[k] for k in range(6) for kind in (div, isl, rel, empty)][:23]
    assert len(pairs) % 4 == 3
    return pairs


@pytest.mark.parametrize("algo", [NW, GG])
@pytest.mark.parametrize("w", [8, 15])
def test_mixed_waves(engine, algo, w):
    pairs = mixed_batch()
    assert all(sa.banded_extend_plan_query(algo, len(a), len(b), w)[1] == 4 for a, b in pairs)
    flags = [model(algo, SCORINGS[algo][0], a, b, w, 10)[6] for a, b in pairs]
    assert any(flags[k] and not flags[k + 1] for k in range(22)) and any(not flags[k] and flags[k + 1] for k in range(22))
    check_model(engine, algo, SCORINGS[algo][0], pairs, w, 10)
    check_model(engine, algo, SCORINGS[algo][0], pairs, w, 10, lut=True)


@pytest.mark.parametrize("algo", [NW, GG])
def test_stale_workspace(engine, algo):
    """Every record word the walk reads was written by this call: stopped pairs leave words unwritten."""
    pairs = mixed_batch()
    for value in (0xFFFFFFFF, 0x55555555, 0):
        engine.test_hook(sa.SA_HOOK_POISON_WS, value)
        check_model(engine, algo, SCORINGS[algo][0], pairs, 8, 10)


@pytest.mark.parametrize("algo", [NW, GG])
def test_workspace_limit_splits_the_launch(engine, algo):
    pairs = mixed_batch()
    want, wops = check_model(engine, algo, SCORINGS[algo][0], pairs, 8, 10)
    launches = engine.last_timings()[2]   # (the score call's, which splits nothing)
    largest = max(sa.banded_extend_plan_query(algo, len(a), len(b), 8)[2] for a, b in pairs)
    try:
        engine.set_workspace_limit(3 * largest)
        got, gops, _, _ = run_align(engine, algo, SCORINGS[algo][0], pairs, 8, 10)
        assert engine.last_timings()[2] >= 4 > launches
    finally:
        engine.set_workspace_limit(0)
    assert want.tobytes() == got.tobytes() and wops.tobytes() == gops.tobytes()


@pytest.mark.parametrize("algo", [NW, GG])
def test_capacity_and_workspace_statuses(engine, algo):
    """The two status codes that need a context: an ops buffer one byte short is SA_ERR_CAPACITY, a workspace
    limit below one pair's records SA_ERR_NOMEM; the exact capacity and the exact limit are accepted."""
    import ctypes as C
    pairs = mixed_batch()
    s1, o1, s2, o2 = pack_bytes(pairs)
    sc = sa.ScoringSystem(*SCORINGS[algo][0])._c()
    need = int(o1[-1] + o2[-1]) + len(pairs)
    res = np.zeros(len(pairs), dtype=sa.RESULT_DTYPE)
    ops = np.zeros(need, dtype=np.uint8)

    def align(cap):
        return engine.L.sa_align_batch_banded_extend(engine.h, algo, C.byref(sc), s1.ctypes.data, o1.ctypes.data, s2.ctypes.data,
                                                     o2.ctypes.data, len(pairs), None, 8, 10, res.ctypes.data, ops.ctypes.data, cap)

    assert align(need - 1) == -4 and b"ops buffer" in engine.L.sa_last_error(engine.h)   # SA_ERR_CAPACITY
    assert align(0) == -4
    assert align(need) == 0
    want = res.copy()
    largest = max(sa.banded_extend_plan_query(algo, len(a), len(b), 8)[2] for a, b in pairs)
    try:
        engine.set_workspace_limit(largest - 4)
        assert align(need) == -3 and b"workspace limit" in engine.L.sa_last_error(engine.h)   # SA_ERR_NOMEM
        engine.set_workspace_limit(largest)
        assert align(need) == 0 and res.tobytes() == want.tobytes()
        assert engine.L.sa_score_batch_banded_extend(engine.h, algo, C.byref(sc), s1.ctypes.data, o1.ctypes.data, s2.ctypes.data,
                                                     o2.ctypes.data, len(pairs), None, 8, 10, res.ctypes.data) == 0   # (no records)
    finally:
        engine.set_workspace_limit(0)
    for p, (a, b) in enumerate(pairs):
        assert int(want[p]["score"]) == model(algo, SCORINGS[algo][0], a, b, 8, 10)[0]


# ---------------------------------------------------------------------------- plan, classes
@pytest.mark.parametrize("algo,records", [(NW, sa.SA_RECORDS_BAND2), (HB, sa.SA_RECORDS_BAND2), (GG, sa.SA_RECORDS_BAND4)])
def test_plan_and_timings(engine, algo, records):
    pairs = mixed_batch()
    run_align(engine, algo, SCORINGS[GG if algo == GG else NW][0], pairs, 8, 10)
    kernel, _, waves, rec = engine.last_plan_ex()
    assert (kernel, waves, rec) == (sa.SA_KERNEL_BANDED, 1, records)
    assert engine.last_timings()[2] >= 1
    run_score(engine, algo, SCORINGS[GG if algo == GG else NW][0], pairs, 8, 10)
    kernel, _, waves, rec = engine.last_plan_ex()
    assert (kernel, waves, rec) == (sa.SA_KERNEL_BANDED, 1, sa.SA_RECORDS_NONE)
    assert engine.last_timings()[1] == 0


def test_python_classes(engine):
    div, isl, _ = drop_inputs()
    pairs = [(a.decode(), b.decode()) for a, b in (div[0], isl[0])] + [("ACGT", ""), ("", "")]
    for cls, algo, args in [(sa.NeedlemanWunschSA, NW, (-2, 1, -3)), (sa.HirschbergSA, NW, (-2, 1, -3)),
                            (sa.GlobalGotohSA, GG, (-4, -1, 1, -3))]:
        al = cls(sa.ScoringSystem(*args))
        want = [model(algo, args, a.encode(), b.encode(), 8, 10) for a, b in pairs]
        assert al.getExtensionScores(pairs, 8, 10) == [x[0] for x in want]
        assert al.getExtensionEndCells(pairs, 8, 10) == [x[1:3] for x in want]
        assert al.getExtensionDropped(pairs, 8, 10) == [x[6] for x in want] == [True, True, False, False]
        out = al.getExtensionAlignments(pairs, 8, 10)
        for (a, b), x, seqs in zip(pairs, want, out):
            row1 = "".join(str(e.first) for e in seqs)
            row2 = "".join(str(e.second) for e in seqs)
            assert row1.replace("-", "") == a and row2.replace("-", "") == b      # the tails are printed
            assert sum(e.is_match for e in seqs) == x[5].count(b"M")
        one = al.getExtensionAlignment(pairs[0][0], pairs[0][1], 8, 10)
        assert [(e.first, e.second) for e in one] == [(e.first, e.second) for e in out[0]]
