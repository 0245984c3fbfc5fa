"""GPU: the score-only calls (sa_score_batch*, Engine.score*): scores and end cells with no
traceback.  Every comparison is exact equality of (score, end_i, end_j) against sa_align_batch on
the same context and against the oracle, plus the contract fields of a score result: start =
(-1, -1), nops = 0, reserved = 0 and only the allowed flag bits."""
import numpy as np
import pytest

import seqalib_amd as sa
from seqalib_amd.multi import MultiEngine
from util import named_lut, oracle_align, oracle_align_matrix, oracle_batch, oracle_sw_scores, pack_bytes

pytestmark = pytest.mark.gpu

BATCH_KERNELS = True   # small host calls stay on the batch kernels (conftest.py); test 6 sets it back

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ALGOS = [sa.SA_SW, sa.SA_NW, sa.SA_LOCAL_GOTOH, sa.SA_GLOBAL_GOTOH]
CLASSES = {sa.SA_SW: sa.SmithWatermanSA, sa.SA_NW: sa.NeedlemanWunschSA, sa.SA_LOCAL_GOTOH: sa.LocalGotohSA,
           sa.SA_GLOBAL_GOTOH: sa.GlobalGotohSA}
AFFINE = {sa.SA_SW: (-1, 1, -1), sa.SA_NW: (-1, 2, -1), sa.SA_LOCAL_GOTOH: (-3, -1, 1, -1, True),
          sa.SA_GLOBAL_GOTOH: (-3, -1, 1, -1, True)}
HACK_SIZES = [(314, 288), (60, 57), (61, 58)]   # SALocalGotoh.h:484-488
# every band edge 64 R of R in {2, 4, 8, 16}, the 32-step chunk edge, and their neighbours
EDGE_LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047,
                2049]


def scorings(algo):
    """The class default, (-2, 2, -3) and the 2-argument !AllowMismatch form; the affine classes
    also with affine terms set (the 3- and 2-argument forms leave them 0)."""
    out = [CLASSES[algo].getDefaultScoring().args(), (-2, 2, -3), (-1, 2)]
    if algo >= sa.SA_LOCAL_GOTOH:
        out += [(-3, -1, 1, -1, True), (-3, -1, 1, -1, False)]
    return out


def seq(rng, alphabet, n):
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


def ragged_pairs(seed, alphabet, extra=34):
    """~100 pairs: every edge length in m and in n against random lengths <= 700 and against each
    other, then random pairs."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k, L in enumerate(EDGE_LENGTHS):
        pairs.append((seq(rng, alphabet, L), seq(rng, alphabet, int(rng.integers(0, 701)))))
        pairs.append((seq(rng, alphabet, int(rng.integers(0, 701))), seq(rng, alphabet, L)))
        pairs.append((seq(rng, alphabet, L), seq(rng, alphabet, EDGE_LENGTHS[-1 - k])))
    for _ in range(extra):
        a = seq(rng, alphabet, int(rng.integers(1, 701)))
        b = bytearray(a)   # related pairs: local maxima away from the corner
        for p in rng.integers(0, len(b), len(b) // 5):
            b[p] = alphabet[rng.integers(0, len(alphabet))]
        pairs.append((a, bytes(b[: int(rng.integers(1, len(b) + 1))])))
    return pairs


def triple(res):
    return [(int(r["score"]), int(r["end_i"]), int(r["end_j"])) for r in res]


def check_contract(res, allowed=0):
    assert (res["start_i"] == -1).all() and (res["start_j"] == -1).all()
    assert (res["nops"] == 0).all() and (res["reserved"] == 0).all()
    assert (res["flags"] & ~np.uint32(allowed) == 0).all(), sorted(set(int(f) for f in res["flags"]))


def check_batch(engine, algo, args, pairs, lut=None, oracle=True, records=None):
    """score_packed == align_packed == oracle on (score, end_i, end_j); returns the score results."""
    sc = sa.ScoringSystem(*args)
    batch = pack_bytes(pairs)
    got = engine.score_packed(algo, sc, *batch, lut=lut).copy()
    plan = engine.last_plan_ex()
    tb_ms = engine.last_timings()[1]
    ref, _ = engine.align_packed(algo, sc, *batch, lut=lut)
    hack = sa.SA_FLAG_SIZE_HACK if algo == sa.SA_LOCAL_GOTOH else 0
    check_contract(got, hack)
    assert triple(got) == triple(ref), (algo, args)
    assert ((got["flags"] & hack) == (ref["flags"] & hack)).all()
    assert tb_ms == 0
    if records is not None:
        assert plan[3] == records, plan
    if oracle:
        if lut is None:
            exp, _ = oracle_batch(algo, args, *batch)
            exp = triple(exp)
        else:
            exp = []
            for a, b in pairs:
                o = oracle_align(algo, args, a, b, lut)
                exp.append((o["score"], o["end_i"], o["end_j"]))
        for p, (a, b) in enumerate(pairs):
            if hack and (len(a), len(b)) in HACK_SIZES:   # reported as NW, flag set
                o = oracle_align(sa.SA_NW, args, a, b, lut)
                exp[p] = (o["score"], o["end_i"], o["end_j"])
                assert got["flags"][p] & hack
        assert triple(got) == exp, (algo, args)
    return got


# ------------------------------------------------------------------ 1. int32 path, all algorithms
@pytest.mark.parametrize("algo", ALGOS)
def test_int32_ragged_batch(engine, algo):
    pairs = ragged_pairs(11 + algo, AA)
    ms = {len(a) for a, _ in pairs}
    ns = {len(b) for _, b in pairs}
    assert set(EDGE_LENGTHS) <= ms and set(EDGE_LENGTHS) <= ns
    for args in scorings(algo):
        check_batch(engine, algo, args, pairs, records=sa.SA_RECORDS_NONE)


# ------------------------------------------------------------------ 2. LUT and bitmaps
@pytest.mark.parametrize("algo", ALGOS)
def test_lut_nwild(engine, algo):
    pairs = ragged_pairs(31 + algo, np.frombuffer(b"ACGTN", dtype=np.uint8), extra=10)
    check_batch(engine, algo, AFFINE[algo], pairs, lut=named_lut("nwild"), records=sa.SA_RECORDS_NONE)


def int_pairs(seed, extra=10, lengths=EDGE_LENGTHS):
    """ragged_pairs' shapes over integers above 256 (300 .. 699): every edge length in m and in n."""
    rng = np.random.default_rng(seed)
    ints = lambda n: rng.integers(300, 700, n).astype(np.int64)
    pairs = []
    for k, L in enumerate(lengths):
        pairs.append((ints(L), ints(int(rng.integers(0, 701)))))
        pairs.append((ints(int(rng.integers(0, 701))), ints(L)))
        pairs.append((ints(L), ints(lengths[-1 - k])))
    for _ in range(extra):
        pairs.append((ints(int(rng.integers(1, 701))), ints(int(rng.integers(1, 701)))))
    return pairs


def mod7_bitmaps(pairs):
    """The sa_*_batch_bits input of integer pairs under match(x, y) = (x - y) % 7 == 0, packed with
    numpy (row-major, ceil(n / 32) words per row, bit j % 32 of word j / 32), and the m x n match
    matrices the oracle takes."""
    n_p = len(pairs)
    off1 = np.zeros(n_p + 1, dtype=np.uint64)
    off2 = np.zeros(n_p + 1, dtype=np.uint64)
    bits_off = np.zeros(n_p + 1, dtype=np.uint64)
    words, mats = [], []
    for p, (a, b) in enumerate(pairs):
        m, n = len(a), len(b)
        wn = (n + 31) // 32
        mt = (np.subtract.outer(a, b) % 7 == 0).astype(np.uint8).reshape(m, n)
        mats.append(mt)
        row = np.zeros((m, 4 * wn), dtype=np.uint8)
        if m and n:
            packed = np.packbits(mt, axis=1, bitorder="little")
            row[:, :packed.shape[1]] = packed
        words.append(row.reshape(-1).view("<u4"))
        off1[p + 1] = off1[p] + m
        off2[p + 1] = off2[p] + n
        bits_off[p + 1] = bits_off[p] + m * wn
    bits = np.ascontiguousarray(np.concatenate(words + [np.zeros(1, dtype="<u4")]), dtype=np.uint32)
    return off1, off2, bits, bits_off, mats


def check_bits(engine, algo, args, pairs, oracle_idx=None, records=sa.SA_RECORDS_NONE):
    """score_bits == align_bits == the matrix oracle on (score, end_i, end_j)."""
    sc = sa.ScoringSystem(*args)
    off1, off2, bits, bits_off, mats = mod7_bitmaps(pairs)
    got = engine.score_bits(algo, sc, off1, off2, bits, bits_off).copy()
    plan = engine.last_plan_ex()
    assert plan[3] == records, plan
    assert engine.last_timings()[1] == 0
    ref, _ = engine.align_bits(algo, sc, off1, off2, bits, bits_off)
    hack = sa.SA_FLAG_SIZE_HACK if algo == sa.SA_LOCAL_GOTOH else 0
    check_contract(got, hack)
    assert triple(got) == triple(ref), (algo, args)
    t = triple(got)
    for p in (range(len(pairs)) if oracle_idx is None else oracle_idx):
        is_hack = hack and mats[p].shape in HACK_SIZES
        o = oracle_align_matrix(sa.SA_NW if is_hack else algo, args, mats[p])
        assert t[p] == (o["score"], o["end_i"], o["end_j"]), (algo, args, p, mats[p].shape)
    return got, plan


@pytest.mark.parametrize("algo", ALGOS)
def test_bitmaps_generic_symbols(engine, algo):
    """The shapes of test 1 over integers above 256 with a non-equality predicate, through
    score_bits.  The bitmaps are packed with numpy; one small batch also goes through
    match_bitmaps and score_generic with the predicate as a Python function."""
    pairs = int_pairs(51 + algo)
    ms = {len(a) for a, _ in pairs}
    ns = {len(b) for _, b in pairs}
    assert set(EDGE_LENGTHS) <= ms and set(EDGE_LENGTHS) <= ns
    got, _ = check_bits(engine, algo, AFFINE[algo], pairs)
    if algo < sa.SA_LOCAL_GOTOH:
        check_bits(engine, algo, (-1, 2), pairs)   # !AllowMismatch
    # the Python predicate path on the small pairs: the same bitmaps, the same results
    match = lambda x, y: (x - y) % 7 == 0
    small = [p for p in range(len(pairs)) if len(pairs[p][0]) * len(pairs[p][1]) <= 20000][:12]
    lists = [([int(x) for x in pairs[p][0]], [int(x) for x in pairs[p][1]]) for p in small]
    o1, o2, b, bo = sa.match_bitmaps(lists, match)
    e1, e2, eb, ebo, _ = mod7_bitmaps([pairs[p] for p in small])
    assert (o1 == e1).all() and (o2 == e2).all() and (bo == ebo).all() and (b[:int(bo[-1])] == eb[:int(ebo[-1])]).all()
    gen = engine.score_generic(algo, sa.ScoringSystem(*AFFINE[algo]), lists, match)
    assert [(r.score, r.end_i, r.end_j, r.start_i, r.start_j, r.ops) for r in gen] == \
        [triple(got)[p] + (-1, -1, b"") for p in small]


# ------------------------------------------------------------------ 3. plans
@pytest.mark.parametrize("alphabet", [ACGT, AA], ids=["dna", "aa"])
def test_few_long_pairs(engine, alphabet):
    rng = np.random.default_rng(71)
    a = seq(rng, alphabet, 4096)
    b = bytearray(a)
    for p in rng.integers(0, 4096, 600):
        b[p] = alphabet[rng.integers(0, len(alphabet))]
    b = bytes(b)
    sw = (-1, 1, -1)
    got = check_batch(engine, sa.SA_SW, sw, [(a, b)], oracle=False)
    exp = oracle_sw_scores(sw, *pack_bytes([(a, b)]))
    assert triple(got) == [tuple(int(x) for x in exp[0])]
    check_batch(engine, sa.SA_LOCAL_GOTOH, (-3, -1, 1, -1, True), [(a[:2048], b)])


def test_many_pairs_one_wave(engine):
    rng = np.random.default_rng(72)
    pairs = [(seq(rng, AA, 300), seq(rng, AA, 300)) for _ in range(1100)]
    sc = sa.ScoringSystem(-1, 1, -1)
    batch = pack_bytes(pairs)
    got = engine.score_packed(sa.SA_SW, sc, *batch).copy()
    k, R, W, rec = engine.last_plan_ex()
    assert (k, W, rec) == (sa.SA_KERNEL_INT32, 1, sa.SA_RECORDS_NONE)
    ref, _ = engine.align_packed(sa.SA_SW, sc, *batch)
    check_contract(got)
    assert triple(got) == triple(ref)
    assert triple(got) == [tuple(int(x) for x in r) for r in oracle_sw_scores((-1, 1, -1), *batch)]


@pytest.mark.parametrize("algo", ALGOS)
def test_band_pipeline_plan(engine, algo, monkeypatch):
    """SEQALIB_SPLIT=0: a few long pairs take the multi-wave band pipeline (W > 1)."""
    monkeypatch.setenv("SEQALIB_SPLIT", "0")
    rng = np.random.default_rng(73 + algo)
    pairs = [(seq(rng, AA, 2049), seq(rng, AA, 1500)), (seq(rng, AA, 700), seq(rng, AA, 2049))]
    sc = sa.ScoringSystem(*AFFINE[algo])
    engine.score_packed(algo, sc, *pack_bytes(pairs))
    k, R, W, rec = engine.last_plan_ex()
    assert W > 1 and rec == sa.SA_RECORDS_NONE, (k, R, W, rec)
    check_batch(engine, algo, AFFINE[algo], pairs, records=sa.SA_RECORDS_NONE)
    # the LUT and bitmap flavours of the same plan
    acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
    npairs = [(seq(rng, acgtn, 2049), seq(rng, acgtn, 1500)), (seq(rng, acgtn, 700), seq(rng, acgtn, 2049))]
    check_batch(engine, algo, AFFINE[algo], npairs, lut=named_lut("nwild"), records=sa.SA_RECORDS_NONE)
    assert engine.last_plan()[2] > 1
    ints = lambda n: rng.integers(300, 700, n).astype(np.int64)
    _, plan = check_bits(engine, algo, AFFINE[algo], [(ints(2049), ints(1500)), (ints(700), ints(2049))])
    assert plan[2] > 1, plan


@pytest.mark.parametrize("algo", ALGOS)
def test_many_pairs_lut_and_bitmaps(engine, algo):
    """One wave per pair (>= 1024 pairs) with a LUT and with bitmaps; 300 rows take R = 8, whose
    bitmap kernels have their own launch bound.  SW also with a scoring whose scores pass 16 bits
    (unkeyed maxima)."""
    rng = np.random.default_rng(171 + algo)
    acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
    pairs = [(seq(rng, acgtn, int(rng.integers(200, 301))), seq(rng, acgtn, int(rng.integers(1, 301)))) for _ in range(1100)]
    pairs[0] = (seq(rng, acgtn, 300), seq(rng, acgtn, 300))
    sc = sa.ScoringSystem(*AFFINE[algo])
    lut = named_lut("nwild")
    batch = pack_bytes(pairs)
    got = engine.score_packed(algo, sc, *batch, lut=lut).copy()
    k, R, W, rec = engine.last_plan_ex()
    assert (k, R, W, rec) == (sa.SA_KERNEL_INT32, 8, 1, sa.SA_RECORDS_NONE)
    ref, _ = engine.align_packed(algo, sc, *batch, lut=lut)
    check_contract(got, sa.SA_FLAG_SIZE_HACK if algo == sa.SA_LOCAL_GOTOH else 0)
    assert triple(got) == triple(ref)
    for p in range(0, 1100, 50):
        if (len(pairs[p][0]), len(pairs[p][1])) in HACK_SIZES:
            continue
        o = oracle_align(algo, AFFINE[algo], pairs[p][0], pairs[p][1], lut)
        assert triple(got)[p] == (o["score"], o["end_i"], o["end_j"]), p
    ints = lambda n: rng.integers(300, 700, n).astype(np.int64)
    ipairs = [(ints(int(rng.integers(200, 301))), ints(int(rng.integers(1, 301)))) for _ in range(1100)]
    ipairs[0] = (ints(300), ints(300))
    for args in [AFFINE[algo]] + ([(-1, 300, -1)] if algo == sa.SA_SW else []):
        _, plan = check_bits(engine, algo, args, ipairs, oracle_idx=range(0, 1100, 50))
        assert plan[:3] == (sa.SA_KERNEL_INT32, 8, 1), plan


def test_wave_cap_of_the_record_free_plan(engine, monkeypatch):
    """SEQALIB_SPLIT=0, one pair of more than 8 bands of 1,024 rows: the align plan runs 9 waves, the
    record-free plan is capped at 8 (its R = 16 kernels are bounded to 8 waves)."""
    monkeypatch.setenv("SEQALIB_SPLIT", "0")
    rng = np.random.default_rng(181)
    for algo in (sa.SA_SW, sa.SA_LOCAL_GOTOH):
        pairs = [(seq(rng, AA, 8300), seq(rng, AA, 700))]
        sc = sa.ScoringSystem(*AFFINE[algo])
        batch = pack_bytes(pairs)
        engine.score_packed(algo, sc, *batch)
        assert engine.last_plan_ex()[1:] == (16, 8, sa.SA_RECORDS_NONE)
        engine.align_packed(algo, sc, *batch)
        assert engine.last_plan_ex()[1:3] == (16, 9)
        check_batch(engine, algo, AFFINE[algo], pairs, records=sa.SA_RECORDS_NONE)


# ------------------------------------------------------------------ 4. DNA fast paths keep their guards
def f16_batch():
    rng = np.random.default_rng(5)
    lengths = [1990, 1993, 1994, 1999, 2005, 2040, 2047, 2048, 2049, 2100, 2500, 3000]
    pairs = []
    for p in range(1100):
        if p < len(lengths):
            a = seq(rng, ACGT, lengths[p])
            pairs.append((a, a))
        else:
            pairs.append((seq(rng, ACGT, int(rng.integers(1, 1401))), seq(rng, ACGT, int(rng.integers(1, 1401)))))
    return lengths, pairs


def test_dna_f16_guard_and_rerun(engine):
    lengths, pairs = f16_batch()
    batch = pack_bytes(pairs)
    sw = sa.ScoringSystem(-1, 1, -1)
    engine.test_hook(sa.SA_HOOK_F16, 0)
    got = engine.score_packed(sa.SA_SW, sw, *batch).copy()
    plan = engine.last_plan_ex()
    assert engine.last_timings()[1] == 0
    engine.score_packed(sa.SA_SW, sw, *batch)   # (the policy reads a launch's count at the next call)
    state_score = engine.test_hook(sa.SA_HOOK_F16, 2)
    engine.test_hook(sa.SA_HOOK_F16, 0)
    ref, _ = engine.align_packed(sa.SA_SW, sw, *batch)
    assert engine.last_plan_ex() == plan   # the same fills: the mode only skips the walks
    assert plan[0] != sa.SA_KERNEL_INT32 and plan[3] != sa.SA_RECORDS_NONE
    engine.align_packed(sa.SA_SW, sw, *batch)
    state_align = engine.test_hook(sa.SA_HOOK_F16, 2)
    assert state_score == state_align
    check_contract(got)
    assert (got["flags"] == 0).all()
    assert [int(x) for x in got["score"][:len(lengths)]] == lengths   # the int32 re-run happened
    assert triple(got) == triple(ref)
    idx = list(range(len(lengths))) + [500, 1099]
    exp = oracle_sw_scores((-1, 1, -1), *pack_bytes([pairs[p] for p in idx]))
    assert [triple(got)[p] for p in idx] == [tuple(int(x) for x in r) for r in exp]


def test_dna_nw_same_batch(engine):
    lengths, pairs = f16_batch()
    batch = pack_bytes(pairs)
    nw = sa.ScoringSystem(-1, 2, -1)
    got = engine.score_packed(sa.SA_NW, nw, *batch).copy()
    assert engine.last_plan_ex()[0] == sa.SA_KERNEL_T16
    ref, _ = engine.align_packed(sa.SA_NW, nw, *batch)
    check_contract(got)
    assert triple(got) == triple(ref)
    idx = list(range(len(lengths))) + [500, 1099]
    exp, _ = oracle_batch(sa.SA_NW, (-1, 2, -1), *pack_bytes([pairs[p] for p in idx]))
    assert [triple(got)[p] for p in idx] == triple(exp)


# ------------------------------------------------------------------ 5. workspace
def test_workspace_limit_between_plans(engine):
    rng = np.random.default_rng(91)
    pair = [(seq(rng, AA, 2048), seq(rng, AA, 2048))]
    batch = pack_bytes(pair)
    args = (-1, 1, -1)
    sc = sa.ScoringSystem(*args)
    ws_score = sa.score_plan_query(sa.SA_SW, sc, 2048, 2048, 1, nsym=20)[3]
    ws_align = sa.plan_query_ex(sa.SA_SW, sc, 2048, 2048, 1, nsym=20)[3]
    assert ws_score < ws_align
    try:
        engine.set_workspace_limit((ws_score + ws_align) // 2)
        with pytest.raises(sa.SeqalibError, match="out of memory"):
            engine.align_packed(sa.SA_SW, sc, *batch)
        got = engine.score_packed(sa.SA_SW, sc, *batch).copy()
        assert engine.last_plan_ex()[3] == sa.SA_RECORDS_NONE
    finally:
        engine.set_workspace_limit(0)
    check_contract(got)
    assert triple(got) == [tuple(int(x) for x in oracle_sw_scores(args, *batch)[0])]


# ------------------------------------------------------------------ 6. small-call kernel
@pytest.mark.parametrize("algo", ALGOS)
def test_small_call_kernel(engine, algo, monkeypatch):
    monkeypatch.delenv("SEQALIB_TINY", raising=False)
    rng = np.random.default_rng(101 + algo)
    # (60, 57) and (61, 58): the two LocalGotoh hack sizes the small-call kernel takes
    shapes = [(11, 8), (60, 57), (61, 58), (0, 5), (7, 0), (0, 0), (256, 128), (32, 1024), (64, 65), (1, 1), (255, 100),
              (65, 500)]
    while len(shapes) < 64:
        m = int(rng.integers(1, 257))
        shapes.append((m, int(rng.integers(1, min(1024, 32768 // m) + 1))))
    pairs = [(seq(rng, AA, m), seq(rng, AA, n)) for m, n in shapes]
    for count in (1, 5, 64):
        for args in (AFFINE[algo], (-1, 2)):
            sub = pairs[:count]
            sc = sa.ScoringSystem(*args)
            engine.score_packed(algo, sc, *pack_bytes(sub))
            plan = engine.last_plan_ex()
            assert plan[0] == sa.SA_KERNEL_TINY and plan[3] == sa.SA_RECORDS_NONE, plan
            assert engine.last_timings() == (0.0, 0.0, 0)
            check_batch(engine, algo, args, sub)
    # the third hack size is beyond the small-call kernel (m = 314): same call shape, batch kernels
    big = [(seq(rng, AA, 314), seq(rng, AA, 288))] + pairs[1:3]
    got = check_batch(engine, algo, AFFINE[algo], big)
    if algo == sa.SA_LOCAL_GOTOH:
        assert (got["flags"] == sa.SA_FLAG_SIZE_HACK).all()
    res = engine.score(algo, sa.ScoringSystem(*AFFINE[algo]), pairs[:3])
    assert all(r.ops == b"" and r.start_i == -1 and r.start_j == -1 for r in res)


# ------------------------------------------------------------------ 7. device API and pipeline
def test_device_api_pipelined_with_align_calls(engine):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    rng = np.random.default_rng(111)
    sets = []
    for alphabet, long_pair in ((ACGT, None), (AA, 7)):
        pairs = [(seq(rng, alphabet, 512), seq(rng, alphabet, 512)) for _ in range(256)]
        if long_pair is not None:   # longer than the max_m the calls pass: SA_FLAG_BAD_SHAPE
            pairs[long_pair] = (seq(rng, alphabet, 600), seq(rng, alphabet, 512))
        h = pack_bytes(pairs)
        sets.append((h, [t(x) for x in h], long_pair))
    sc = sa.ScoringSystem(-1, 1, -1)
    stream = torch.cuda.current_stream().cuda_stream

    def run_calls(pipelined):
        outs = []
        for k in range(6):
            h, d, long_pair = sets[(k // 2) % 2]
            score = k % 2 == 0
            res = torch.zeros(256 * 32, dtype=torch.uint8, device=dev)
            ops = None if score else torch.zeros(len(h[0]) + len(h[2]) + 256, dtype=torch.uint8, device=dev)
            if score:
                engine.score_device(sa.SA_SW, sc, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 256,
                                    512, 512, res.data_ptr(), stream)
            else:
                engine.align_device(sa.SA_SW, sc, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 256,
                                    512, 512, res.data_ptr(), ops.data_ptr(), stream)
            if not pipelined:
                torch.cuda.synchronize()
            outs.append((score, long_pair, h, res, ops))
        return outs

    serial = run_calls(False)
    engine.set_pipeline(True)
    try:
        piped = run_calls(True)
        engine.wait()
    finally:
        engine.set_pipeline(False)
    torch.cuda.synchronize()
    as_res = lambda x: np.frombuffer(x.cpu().numpy().tobytes(), dtype=sa.RESULT_DTYPE)
    for (score, long_pair, h, res_s, ops_s), (_, _, _, res_p, ops_p) in zip(serial, piped):
        a, b = as_res(res_s), as_res(res_p)
        assert a.tobytes() == b.tobytes()
        if not score:
            assert ops_s.cpu().numpy().tobytes() == ops_p.cpu().numpy().tobytes()
            continue
        check_contract(b, sa.SA_FLAG_BAD_SHAPE)
        ok = np.ones(256, dtype=bool)
        if long_pair is not None:
            assert b["flags"][long_pair] == sa.SA_FLAG_BAD_SHAPE
            ok[long_pair] = False
        assert (b["flags"][ok] == 0).all()
        exp = oracle_sw_scores((-1, 1, -1), *h)
        assert [triple(b)[p] for p in np.nonzero(ok)[0]] == [tuple(int(x) for x in exp[p]) for p in np.nonzero(ok)[0]]
    # the align calls of the same inputs agree with the score calls on (score, end cell) and the flag
    for k in (0, 2):
        a, b = as_res(piped[k][3]), as_res(piped[k + 1][3])
        assert triple(a) == triple(b) and (a["flags"] == b["flags"]).all()


# ------------------------------------------------------------------ 8. poisoned workspace
@pytest.mark.parametrize("alphabet", [ACGT, AA], ids=["dna", "aa"])
def test_poisoned_workspace(engine, alphabet):
    rng = np.random.default_rng(121)
    pairs = [(seq(rng, alphabet, int(rng.integers(1, 900))), seq(rng, alphabet, int(rng.integers(1, 900))))
             for _ in range(1100)]
    batch = pack_bytes(pairs)
    sc = sa.ScoringSystem(-1, 1, -1)
    engine.score_packed(sa.SA_SW, sc, *batch)   # (the workspace of this shape exists)
    engine.test_hook(sa.SA_HOOK_POISON_WS, 0xDEADBEEF)
    got = engine.score_packed(sa.SA_SW, sc, *batch).copy()
    check_contract(got)
    assert triple(got) == [tuple(int(x) for x in r) for r in oracle_sw_scores((-1, 1, -1), *batch)]
    engine.test_hook(sa.SA_HOOK_POISON_WS, 0x7F7F7F7F)
    nw = engine.score_packed(sa.SA_NW, sa.ScoringSystem(-1, 2, -1), *batch).copy()
    check_contract(nw)
    exp, _ = oracle_batch(sa.SA_NW, (-1, 2, -1), *batch)
    assert triple(nw) == triple(exp)


# ------------------------------------------------------------------ 9. multi handle
def test_multi_handle_matches_single_context(engine):
    pairs = ragged_pairs(131, AA, extra=134)[:200]
    assert len(pairs) == 200
    batch = pack_bytes(pairs)
    multi = MultiEngine([0, 0])
    try:
        for algo in ALGOS:
            sc = sa.ScoringSystem(*AFFINE[algo])
            one = engine.score_packed(algo, sc, *batch).copy()
            two = multi.score_packed(algo, sc, *batch)
            assert one.tobytes() == two.tobytes()
    finally:
        multi.close()


# ------------------------------------------------------------------ aligner classes and the algorithms beyond the four
def test_aligner_classes_get_scores(engine):
    rng = np.random.default_rng(141)
    pairs = [(seq(rng, AA, int(rng.integers(1, 400))), seq(rng, AA, int(rng.integers(1, 400)))) for _ in range(9)]
    for cls in (sa.SmithWatermanSA, sa.NeedlemanWunschSA, sa.LocalGotohSA, sa.GlobalGotohSA, sa.HirschbergSA):
        al = cls()
        scores = al.getScores(pairs)
        each = []
        cells = []
        one = cls()
        for a, b in pairs:
            one.getAlignment(a, b)
            each.append(one.getScore())
            cells.append((one.last.end_i, one.last.end_j))
        assert scores == each, cls.__name__
        assert al.getScore() == scores[-1]
        if cls in (sa.SmithWatermanSA, sa.LocalGotohSA):
            assert al.getEndCells(pairs) == cells
    with pytest.raises(sa.SeqalibError, match="unsupported"):
        engine.score(sa.SA_MYERS_MILLER, sa.ScoringSystem(-3, -1, 1, -1), pairs)
