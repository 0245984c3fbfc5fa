"""Device-resident seeded banded NW / GlobalGotoh (sa_align_batch_banded_seeded_device,
sa_score_batch_banded_seeded_device) on the GPU.

The inputs are torch tensors: two resident byte buffers and per-pair descriptors (start and length per side, seed
diagonal, ops offset).  The references are the host-buffer call (sa_align_batch_banded_seeded) on the materialised
slices, byte for byte, and tests/seeded_model.py.  The input builders are those of test_gpu_banded_seeded.py.

The test ids carry the algorithm (nw, gg) and the GlobalGotoh cases with 64 lanes per pair live in functions of
their own (gg64), so that `-k nw`, `-k "gg and not gg64"` and `-k gg64` run the three groups apart.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import seqalib_amd as sa
from seeded_model import seeded_legal, seeded_model
from test_gpu_banded import ACGT, related, seq
from test_gpu_banded_seeded import legal_batch
from test_gpu_ends_free import edited
from util import named_lut, pack_bytes, scoring_fields

pytestmark = pytest.mark.gpu

NW, HB, GG = sa.SA_NW, sa.SA_HIRSCHBERG, sa.SA_GLOBAL_GOTOH
ALGOS = [pytest.param(NW, id="nw"), pytest.param(GG, id="gg")]
SCORINGS = {NW: [(-1, 1, -1), (-1, 2), (1, -1, -2)],
            GG: [(-3, -1, 1, -1), (-3, -1, 2, -1, False), (2, -1, -1, -2)]}
S1B, S1E, S2B, S2E = sa.SA_FREE_SEQ1_BEGIN, sa.SA_FREE_SEQ1_END, sa.SA_FREE_SEQ2_BEGIN, sa.SA_FREE_SEQ2_END
FIT = S2B | S2E
PURINE = named_lut("purine")
VARIANTS = [(1, 16), (2, 16), (4, 16), (4, 32), (4, 64), (8, 64), (16, 64), (32, 64)]   # (R, L): 2 R L diagonals
FILL = 0xEE   # what the ops buffer holds before a call


def dev(a):
    """A numpy array as a device tensor of the same bytes (torch has no unsigned 32 / 64-bit arithmetic types)."""
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


class Batch:
    """Descriptors of one call, on the host (numpy) and, after upload(), on the device."""

    def __init__(self, seq1, start1, len1, seq2, start2, len2, diag, ops_off, ops_bytes):
        self.seq1 = np.frombuffer(bytes(seq1) + b"\0", dtype=np.uint8)[:-1].copy()
        self.seq2 = np.frombuffer(bytes(seq2) + b"\0", dtype=np.uint8)[:-1].copy()
        self.start1 = np.asarray(start1, dtype=np.uint64)
        self.start2 = np.asarray(start2, dtype=np.uint64)
        self.len1 = np.asarray(len1, dtype=np.uint32)
        self.len2 = np.asarray(len2, dtype=np.uint32)
        self.diag = np.asarray(diag, dtype=np.int32)
        self.ops_off = np.asarray(ops_off, dtype=np.uint64)
        self.ops_bytes = int(ops_bytes)
        self.n = len(self.diag)
        self.seq1_bytes, self.seq2_bytes = len(self.seq1), len(self.seq2)

    @classmethod
    def packed(cls, pairs, diags):
        """The host call's own layout: start = off[p], ops_off = off1[p] + off2[p] + p."""
        s1, o1, s2, o2 = pack_bytes(pairs)
        p = np.arange(len(pairs), dtype=np.uint64)
        return cls(s1.tobytes(), o1[:-1], np.diff(o1), s2.tobytes(), o2[:-1], np.diff(o2), diags, o1[:-1] + o2[:-1] + p,
                   int(o1[-1] + o2[-1]) + len(pairs))

    def pairs(self):
        return [(self.seq1[int(a):int(a) + int(m)].tobytes(), self.seq2[int(b):int(b) + int(n)].tobytes())
                for a, m, b, n in zip(self.start1, self.len1, self.start2, self.len2)]

    def upload(self):
        # (an empty buffer still gets an address: one spare byte)
        self.d = {k: dev(getattr(self, k)) for k in ("start1", "len1", "start2", "len2", "diag", "ops_off")}
        self.d["seq1"] = dev(np.append(self.seq1, np.uint8(0)))
        self.d["seq2"] = dev(np.append(self.seq2, np.uint8(0)))
        return self


def device_call(engine, algo, args, b, w, fe, max_m, max_n, lut=None, score=False, stream=0, sync=True, out=None):
    """One device call on uploaded descriptors: (results, the whole ops buffer) as numpy arrays (sync), or the two
    output tensors.  out: the output tensors, filled by the caller."""
    d = b.d
    d_res = out[0] if out else torch.full((max(b.n, 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ops = out[1] if out else torch.full((max(b.ops_bytes, 1),), FILL, dtype=torch.uint8, device="cuda")
    d_lut = dev(lut.reshape(65536)) if lut is not None else None
    sc = sa.ScoringSystem(*args)
    common = (algo, sc, d["seq1"].data_ptr(), b.seq1_bytes, d["start1"].data_ptr(), d["len1"].data_ptr(), d["seq2"].data_ptr(),
              b.seq2_bytes, d["start2"].data_ptr(), d["len2"].data_ptr(), b.n, max_m, max_n, d["diag"].data_ptr(), w, fe)
    lut_ptr = d_lut.data_ptr() if d_lut is not None else 0
    if stream == 0:
        torch.cuda.synchronize()   # the fills above ran on torch's stream, the call runs on the context's
    if score:
        engine.score_banded_seeded_device(*common, d_res.data_ptr(), stream, lut_ptr)
    else:
        engine.align_banded_seeded_device(*common, d_res.data_ptr(), d_ops.data_ptr(), d["ops_off"].data_ptr(), b.ops_bytes,
                                          stream, lut_ptr)
    if not sync:
        return d_res, d_ops, d_lut
    engine.wait()
    torch.cuda.synchronize()
    return d_res.cpu().numpy()[:b.n * 32].view(sa.RESULT_DTYPE), d_ops.cpu().numpy()[:b.ops_bytes]


def host_call(engine, algo, args, pairs, diags, w, fe, lut=None, score=False):
    s1, o1, s2, o2 = pack_bytes(pairs)
    sc = sa.ScoringSystem(*args)
    if score:
        return engine.score_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diags, w, fe, lut), None, o1, o2
    res, ops = engine.align_banded_seeded_packed(algo, sc, s1, o1, s2, o2, diags, w, fe, lut)
    return res, ops, o1, o2


def assert_equals_host(engine, algo, args, b, w, fe, max_m, max_n, lut=None, model=()):
    """Align and score call of batch b against the host call on its materialised slices: every result byte and
    every op, and nothing written outside the ops.  model: pairs also checked against tests/seeded_model.py."""
    pairs, diags = b.pairs(), [int(k) for k in b.diag]
    keep = list(range(b.n))
    want, wops, o1, o2 = host_call(engine, algo, args, [pairs[p] for p in keep], [diags[p] for p in keep], w, fe, lut)
    wscore = host_call(engine, algo, args, [pairs[p] for p in keep], [diags[p] for p in keep], w, fe, lut, score=True)[0]
    res, ops = device_call(engine, algo, args, b, w, fe, max_m, max_n, lut)
    score = device_call(engine, algo, args, b, w, fe, max_m, max_n, lut, score=True)[0]
    written = np.zeros(b.ops_bytes, dtype=bool)
    for q, p in enumerate(keep):
        assert res[p].tobytes() == want[q].tobytes(), (algo, args, w, fe, p, res[p], want[q])
        assert score[p].tobytes() == wscore[q].tobytes(), (algo, args, w, fe, p, score[p], wscore[q])
        nops, oo, ho = int(want[q]["nops"]), int(b.ops_off[p]), int(o1[q] + o2[q]) + q
        assert ops[oo:oo + nops].tobytes() == wops[ho:ho + nops].tobytes(), (algo, args, w, fe, p)
        written[oo:oo + nops] = True
    assert (ops[~written] == FILL).all(), "a byte outside the pairs' ops was written"
    for p in model:
        a, s = pairs[p]
        m = seeded_model(algo, args, a, s, diags[p], w, fe, lut)
        r = res[p]
        oo = int(b.ops_off[p])
        got = (int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
               ops[oo:oo + int(r["nops"])].tobytes())
        assert got == m, (algo, args, w, fe, p, len(a), len(s), diags[p])
    return res, ops, score


# ------------------------------------------------------------------------- 1. equals the host call
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("fe", range(16))
def test_equals_the_host_call(engine, algo, fe):
    """16 ragged pairs, m, n <= 40, ("", "") included, in the host call's own layout; every flag set, w in
    {0, 1, 3, 8}, byte equality and the purine table.  Fails without the device calls."""
    for n_w, w in enumerate((0, 1, 3, 8)):
        args = SCORINGS[algo][(fe + n_w) % 3]
        if w == 0 and not scoring_fields(args)[5]:
            args = SCORINGS[algo][0]   # one diagonal needs allow_mismatch
        pairs, diags = legal_batch(1000 * fe + w, w, fe, 16)
        assert pairs[0] == (b"", b"")
        b = Batch.packed(pairs, diags).upload()
        model = range(b.n) if fe == FIT else ()
        assert_equals_host(engine, algo, args, b, w, fe, 40, 40, model=model)
        assert_equals_host(engine, algo, args, b, w, fe, 40, 40, PURINE, model=model)


def test_hirschberg_means_nw(engine):
    pairs, diags = legal_batch(5, 3, 15, 16)
    b = Batch.packed(pairs, diags).upload()
    h, hops = device_call(engine, HB, (-1, 1, -1), b, 3, 15, 40, 40)
    n, nops = device_call(engine, NW, (-1, 1, -1), b, 3, 15, 40, 40)
    assert h.tobytes() == n.tobytes() and hops.tobytes() == nops.tobytes()
    assert (n["nops"] > 0).any()


# ------------------------------------------------------------------------- 2. a resident reference
def contig_batch(seed=7):
    """One 4,096-symbol contig and 64 reads of 24-40 symbols cut from it and edited, each against the window
    contig[pos - 20 .. pos + len + 20), clipped.  The windows overlap and start unsorted, pairs 10 and 11 share one
    window, and the pairs' order in the reads buffer and the order of their ops regions are two more shuffles."""
    rng = np.random.default_rng(seed)
    contig = seq(rng, ACGT, 4096)
    pos = [int(x) for x in rng.integers(0, 4096 - 40, 64)]
    pos[0], pos[1] = 0, 4096 - 40          # both clips
    length = [int(x) for x in rng.integers(24, 41, 64)]
    length[1] = 40
    pos[11], length[11] = pos[10], length[10]
    reads = [edited(rng, contig[p:p + n]) for p, n in zip(pos, length)]
    wstart = [max(p - 20, 0) for p in pos]
    wend = [min(p + n + 20, 4096) for p, n in zip(pos, length)]
    diag = [p - s + int(rng.integers(-2, 3)) for p, s in zip(pos, wstart)]
    order = rng.permutation(64)            # the reads buffer holds the reads in this order
    start1 = np.zeros(64, dtype=np.uint64)
    at = 0
    for p in order:
        start1[p] = at
        at += len(reads[p])
    buf = b"".join(reads[p] for p in order)
    ops_order = rng.permutation(64)        # and the ops regions lie in this one, behind a guard region
    ops_off = np.zeros(64, dtype=np.uint64)
    at = 64
    for p in ops_order:
        ops_off[p] = at
        at += len(reads[p]) + (wend[p] - wstart[p]) + 1
    b = Batch(buf, start1, [len(r) for r in reads], contig, wstart, [e - s for s, e in zip(wstart, wend)], diag, ops_off, at + 64)
    assert sorted(wstart) != wstart and (b.start2[10], b.len2[10]) == (b.start2[11], b.len2[11])
    return b


@pytest.mark.parametrize("algo", ALGOS)
def test_resident_reference(engine, algo):
    b = contig_batch().upload()
    for (a, s), k in zip(b.pairs(), b.diag):
        assert seeded_legal(len(a), len(s), int(k), 8, FIT) == (True, True)
    res, _, _ = assert_equals_host(engine, algo, SCORINGS[algo][0], b, 8, FIT, 44, 84, model=range(b.n))
    assert (res["flags"] == 0).all() and (res["nops"] >= 20).all()
    assert_equals_host(engine, algo, SCORINGS[algo][0], b, 8, FIT, 44, 84, PURINE)


# ------------------------------------------------------------------------- 3. every variant in one call
def cells_per_lane(diagonals):
    return next(R for R, L in VARIANTS if diagonals <= 2 * R * L)


def variant_batch(sizes, clipped, seed, upload=True):
    """Pairs m = n = s seeded at diagonal 0 (with w >= s the clipped band holds 2s + 1 diagonals), five pairs of
    3 x 3 -- the narrowest variant, one wave with idle groups -- and, when asked for, the clipped pair 40 x 1073."""
    rng = np.random.default_rng(seed)
    pairs = []
    for s in list(sizes) + [3] * 5:
        a = seq(rng, ACGT, s)
        pairs.append((a, related(rng, ACGT, a, s)))
    if clipped:
        a = seq(rng, ACGT, 40)
        pairs.append((a, edited(rng, a) + seq(rng, ACGT, 1073)))
        pairs[-1] = (a, pairs[-1][1][:1073])
    order = [int(x) for x in np.random.default_rng(seed + 1).permutation(len(pairs))]   # the variants interleaved
    b = Batch.packed([pairs[p] for p in order], [0] * len(pairs))
    return b.upload() if upload else b   # (tests/test_banded_emu.py runs the same batch without a device)


def check_variants(engine, monkeypatch, algo, sizes, clipped, w, top):
    monkeypatch.setenv("SEQALIB_BAND_MERGE", "0")   # the host call with every pair in its narrowest variant, as here
    b = variant_batch(sizes, clipped, 31 * w + len(sizes))
    used = {cells_per_lane(2 * int(m) + 1 if m == n else int(m) + w + 1) for m, n in zip(b.len1, b.len2)}
    max_n = max(top, 1073 if clipped else 0)
    bound = cells_per_lane(min(2 * w + 1, top + max_n + 1))
    assert sa.banded_seeded_device_plan_query(algo, top, max_n, w)[0] == bound
    small = [p for p in range(b.n) if int(b.len1[p]) <= 64 or int(b.len2[p]) == 1073]
    fe = S2E   # the clipped pair's flag; the square pairs hold (0, 0) and (m, n), legal under every set
    assert_equals_host(engine, algo, SCORINGS[algo][0], b, w, fe, top, max_n, model=small)
    assert engine.last_plan_ex()[:3] == (sa.SA_KERNEL_BANDED, bound, 1)
    return used


def test_every_variant_in_one_call_nw(engine, monkeypatch):
    sizes = (15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512)
    used = check_variants(engine, monkeypatch, NW, sizes, True, 1023, 512)
    assert used == {1, 2, 4, 8, 16}                 # (4 cells per lane: three variants, 16 / 32 / 64 lanes)
    used = check_variants(engine, monkeypatch, NW, (1024, 2047), False, 2047, 2047)
    assert used == {1, 32}                          # the six variants between them are launched and find no pair


def test_every_variant_up_to_32_lanes_gg(engine, monkeypatch):
    # s = 127: 255 diagonals, the 32-lane variant; the three wider ones up to the bound's are launched and empty
    check_variants(engine, monkeypatch, GG, (15, 16, 31, 32, 63, 64, 127), False, 1023, 512)


def test_gg64_lanes_per_pair(engine, monkeypatch):
    """GlobalGotoh with 64 lanes per pair: 4, 8 and 16 cells per lane, and the clipped 40 x 1073 pair (1064
    diagonals, 16 cells per lane) whose cells the host seeded call is on record walking correctly."""
    used = check_variants(engine, monkeypatch, GG, (128, 255, 256, 511, 512), True, 1023, 512)
    assert used == {1, 4, 8, 16}


# ------------------------------------------------------------------------- 4. refusals among valid pairs
def refusal_batch(upload=True):
    """Valid pairs (legal under free_ends = 0 at w = 3) with one pair for each refusal between them.
    Returns the batch, {pair: flag} for the align call, and the pairs only the align call refuses."""
    pairs, diags = legal_batch(11, 3, 0, 12)
    rng = np.random.default_rng(12)
    a41, b41 = seq(rng, ACGT, 41), seq(rng, ACGT, 41)
    bad = [((a41, a41[:38]), 0, "len1 > max_m"), ((b41[:39], b41), 0, "len2 > max_n"),
           ((a41[:10], a41[:12]), 0, "start1 + len1 past seq1_bytes"), ((a41[:10], a41[:12]), 0, "start1 wraps"),
           ((a41[:10], a41[:12]), 0, "start2 + len2 past seq2_bytes"), ((a41[:20], a41[:20]), 0, "ops region past ops_bytes"),
           ((a41[:10], a41[:12]), -11, "diag = -m - 1"), ((a41[:10], a41[:12]), 13, "diag = n + 1"),
           ((a41[:5], a41[:30]), 20, "neither (0, 0) nor (m, n) in the band")]
    slots = [1, 3, 4, 6, 8, 9, 11, 14, 16]   # where the bad pairs go
    allp, alld, why = [], [], {}
    good = list(zip(pairs, diags))
    for p in range(len(good) + len(bad)):
        if p in slots:
            (pr, k, reason) = bad[slots.index(p)]
            why[p] = reason
        else:
            pr, k = good.pop(0)
        allp.append(pr)
        alld.append(k)
    b = Batch.packed(allp, alld)
    # guard regions round the ops: every region moves up by 64, and 64 more bytes follow the last
    b.ops_off = b.ops_off + np.uint64(64)
    b.ops_bytes += 128
    flags = {}
    for p, reason in why.items():
        flags[p] = sa.SA_FLAG_BAD_SHAPE
        if reason == "start1 + len1 past seq1_bytes":
            b.start1[p] = b.seq1_bytes - 9
        elif reason == "start1 wraps":
            b.start1[p] = 2 ** 64 - 5
        elif reason == "start2 + len2 past seq2_bytes":
            b.start2[p] = b.seq2_bytes - 11
        elif reason == "ops region past ops_bytes":
            b.ops_off[p] = b.ops_bytes - 40   # 20 + 20 + 1 bytes are needed
        elif not reason.startswith("len"):
            flags[p] = sa.SA_FLAG_BAD_BAND
    align_only = [p for p, r in why.items() if r.startswith("ops")]
    return (b.upload() if upload else b), flags, align_only


@pytest.mark.parametrize("algo", ALGOS)
def test_refusals_among_valid_pairs(engine, algo):
    b, flags, align_only = refusal_batch()
    args = SCORINGS[algo][0]
    pairs, diags = b.pairs(), [int(k) for k in b.diag]
    good = [p for p in range(b.n) if p not in flags]
    want, wops, o1, o2 = host_call(engine, algo, args, [pairs[p] for p in good], [diags[p] for p in good], 3, 0)
    res, ops = device_call(engine, algo, args, b, 3, 0, 40, 40)
    zero = np.zeros(1, dtype=sa.RESULT_DTYPE)[0]
    written = np.zeros(b.ops_bytes, dtype=bool)
    for p in range(b.n):
        if p in flags:
            exp = zero.copy()
            exp["flags"] = flags[p]
            assert res[p].tobytes() == exp.tobytes(), (p, res[p])
        else:
            q = good.index(p)
            assert res[p].tobytes() == want[q].tobytes(), (p, res[p], want[q])
            nops, oo, ho = int(want[q]["nops"]), int(b.ops_off[p]), int(o1[q] + o2[q]) + q
            assert ops[oo:oo + nops].tobytes() == wops[ho:ho + nops].tobytes(), p
            written[oo:oo + nops] = True
    assert written.any() and (ops[~written] == FILL).all()   # the guards and the refused pairs' regions included
    # the score call has no ops region to refuse: that pair runs, the others keep their flag
    sgood = sorted(good + align_only)
    swant = host_call(engine, algo, args, [pairs[p] for p in sgood], [diags[p] for p in sgood], 3, 0, score=True)[0]
    score = device_call(engine, algo, args, b, 3, 0, 40, 40, score=True)[0]
    for p in range(b.n):
        if p in sgood:
            assert score[p].tobytes() == swant[sgood.index(p)].tobytes(), (p, score[p])
        else:
            exp = zero.copy()
            exp["flags"] = flags[p]
            assert score[p].tobytes() == exp.tobytes(), (p, score[p])


# ------------------------------------------------------------------------- 5. stream and state
class OwnStream:
    """A non-default HIP stream made here and destroyed on the way out, with its own asynchronous copies.  torch
    never sees it -- no tensor is allocated on it and torch's stream pool is not touched -- so nothing refers to
    it once it is gone, and the test leaves the process's streams as it found them."""

    def __enter__(self):
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        self.hip = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
        self.hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip.hipStreamDestroy.argtypes = [C.c_void_p]
        handle = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(handle), 1) == 0   # hipStreamNonBlocking
        self.handle = handle.value
        return self

    def upload(self, dst, src):
        """dst (device tensor) <- src (pinned host tensor), asynchronously on this stream."""
        assert src.is_pinned() and dst.numel() * dst.element_size() == src.numel() * src.element_size()
        assert self.hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), 1, self.handle) == 0

    def synchronize(self):
        assert self.hip.hipStreamSynchronize(self.handle) == 0

    def __exit__(self, *exc):
        self.synchronize()
        assert self.hip.hipStreamDestroy(self.handle) == 0


@pytest.mark.parametrize("algo", ALGOS)
def test_stream_and_state(engine, algo):
    args = SCORINGS[algo][0]
    b = contig_batch(seed=9)
    want_res, want_ops = device_call(engine, algo, args, b.upload(), 8, FIT, 44, 84)
    args2 = SCORINGS[algo][2]   # the second call of the pair below: another scoring, width and flag set
    want2 = device_call(engine, algo, args2, b, 5, 15, 44, 84)
    assert want_res.tobytes() != want2[0].tobytes()
    # inputs copied asynchronously on a non-default stream, two calls enqueued behind them with no sync between
    host = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in
            {"start1": b.start1.view(np.int64), "len1": b.len1.view(np.int32), "start2": b.start2.view(np.int64),
             "len2": b.len2.view(np.int32), "diag": b.diag, "ops_off": b.ops_off.view(np.int64),
             "seq1": np.append(b.seq1, np.uint8(0)), "seq2": np.append(b.seq2, np.uint8(0))}.items()}
    b.d = {k: torch.zeros(v.shape, dtype=v.dtype, device="cuda") for k, v in host.items()}   # (zeros: every pair BAD_BAND or empty if a copy were skipped)
    outs = [(torch.full((b.n * 32,), 0xAB, dtype=torch.uint8, device="cuda"),
             torch.full((b.ops_bytes,), FILL, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()   # the buffers exist and are filled; from here on nothing waits
    with OwnStream() as st:
        for k, v in host.items():
            st.upload(b.d[k], v)
        device_call(engine, algo, args, b, 8, FIT, 44, 84, stream=st.handle, sync=False, out=outs[0])
        device_call(engine, algo, args2, b, 5, 15, 44, 84, stream=st.handle, sync=False, out=outs[1])
        st.synchronize()
    for (d_res, d_ops), (r, o) in zip(outs, ((want_res, want_ops), want2)):
        assert d_res.cpu().numpy()[:b.n * 32].tobytes() == r.tobytes()
        assert d_ops.cpu().numpy()[:b.ops_bytes].tobytes() == o.tobytes()
    # the same call twice, and after the workspace was poisoned
    again = device_call(engine, algo, args, b, 8, FIT, 44, 84)
    assert again[0].tobytes() == want_res.tobytes() and again[1].tobytes() == want_ops.tobytes()
    for poison in (0xFFFFFFFF, 0):
        engine.test_hook(sa.SA_HOOK_POISON_WS, poison)
        again = device_call(engine, algo, args, b, 8, FIT, 44, 84)
        assert again[0].tobytes() == want_res.tobytes() and again[1].tobytes() == want_ops.tobytes()
    # a call between two sa_align_batch_device calls leaves theirs right
    rng = np.random.default_rng(3)
    sw_pairs = []
    for _ in range(24):
        a = seq(rng, ACGT, int(rng.integers(20, 200)))
        sw_pairs.append((a, related(rng, ACGT, a, int(rng.integers(20, 200)))))
    s1, o1, s2, o2 = pack_bytes(sw_pairs)
    sw = sa.ScoringSystem(-1, 1, -1)
    ref_res, ref_ops = engine.align_packed(sa.SA_SW, sw, s1, o1, s2, o2)
    d = [dev(np.append(s1, np.uint8(0))), dev(o1), dev(np.append(s2, np.uint8(0))), dev(o2)]
    outs = []
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        d_res = torch.zeros(len(sw_pairs) * 32, dtype=torch.uint8, device="cuda")
        d_ops = torch.zeros(int(o1[-1] + o2[-1]) + len(sw_pairs), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()   # (the zeroing ran on torch's stream)
        engine.align_device(sa.SA_SW, sw, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(sw_pairs),
                            200, 200, d_res.data_ptr(), d_ops.data_ptr(), stream)
        outs.append((d_res, d_ops))
        if k == 0:
            mid = device_call(engine, algo, args, b, 8, FIT, 44, 84, stream=stream, sync=False)
    torch.cuda.synchronize()
    assert mid[0].cpu().numpy()[:b.n * 32].tobytes() == want_res.tobytes()
    assert mid[1].cpu().numpy()[:b.ops_bytes].tobytes() == want_ops.tobytes()
    for d_res, d_ops in outs:
        r = d_res.cpu().numpy().view(sa.RESULT_DTYPE)
        o = d_ops.cpu().numpy()
        for f in ("score", "end_i", "end_j", "start_i", "start_j", "nops"):
            assert np.array_equal(r[f], ref_res[f]), f
        for p in range(len(sw_pairs)):
            at = int(o1[p] + o2[p]) + p
            assert o[at:at + int(r["nops"][p])].tobytes() == ref_ops[at:at + int(r["nops"][p])].tobytes(), p


# ------------------------------------------------------------------------- 6. chunks
@pytest.mark.parametrize("algo,records", [pytest.param(NW, sa.SA_RECORDS_BAND2, id="nw"), pytest.param(GG, sa.SA_RECORDS_BAND4, id="gg")])
def test_chunks_under_a_workspace_limit(engine, algo, records):
    args = SCORINGS[algo][0]
    pairs, diags = legal_batch(21, 8, FIT, 16)
    b = Batch.packed(pairs, diags).upload()
    want_res, want_ops = device_call(engine, algo, args, b, 8, FIT, 40, 40)
    assert engine.last_timings()[2] == 1
    R, rec, plan = sa.banded_seeded_device_plan_query(algo, 40, 40, 8)
    assert engine.last_plan_ex() == (sa.SA_KERNEL_BANDED, R, 1, records) and R == cells_per_lane(17)
    fixed = 8192 + 512
    try:
        engine.set_workspace_limit(fixed + 6 * (rec + plan))   # six pairs per chunk: 6 + 6 + 4
        res, ops = device_call(engine, algo, args, b, 8, FIT, 40, 40)
        fill_ms, tb_ms, launches = engine.last_timings()
        assert launches == 3 and fill_ms > 0 and tb_ms > 0
        assert res.tobytes() == want_res.tobytes() and ops.tobytes() == want_ops.tobytes()
        engine.set_workspace_limit(fixed + rec + plan)         # one pair per chunk
        res, ops = device_call(engine, algo, args, b, 8, FIT, 40, 40)
        assert engine.last_timings()[2] == 16
        assert res.tobytes() == want_res.tobytes() and ops.tobytes() == want_ops.tobytes()
        engine.set_workspace_limit(fixed + rec + plan - 1)     # below one pair's provision
        with pytest.raises(sa.SeqalibError, match="workspace limit"):
            device_call(engine, algo, args, b, 8, FIT, 40, 40)
        # a score call provisions plans only
        engine.set_workspace_limit(fixed + 6 * plan)
        score = device_call(engine, algo, args, b, 8, FIT, 40, 40, score=True)[0]
        assert engine.last_timings()[1:] == (0, 3)
        assert engine.last_plan_ex() == (sa.SA_KERNEL_BANDED, R, 1, sa.SA_RECORDS_NONE)
        for f in ("score", "end_i", "end_j"):
            assert np.array_equal(score[f], want_res[f]), f
        engine.set_workspace_limit(fixed + plan - 1)
        with pytest.raises(sa.SeqalibError, match="workspace limit"):
            device_call(engine, algo, args, b, 8, FIT, 40, 40, score=True)
    finally:
        engine.set_workspace_limit(0)
