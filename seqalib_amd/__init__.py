"""seqalib_amd — MI355X (gfx950) pairwise sequence alignment behind the SeqALib API.

Python view of the engine in ``seqalib_amd/lib/libseqalib_hip.so`` (C ABI:
``include/seqalib_hip.h``).  The C++ drop-in for the reference's header-only API lives in
``include/seqalib/SequenceAlignment.h``; this module mirrors the same surface for tests, the
benchmark and Python users:

* :class:`ScoringSystem` — the three constructor overloads of the reference
  (``include/SequenceAlignment.h:92-118``), with the same "which fields are meaningful" rules.
* :class:`SmithWatermanSA`, :class:`NeedlemanWunschSA`, :class:`LocalGotohSA`,
  :class:`GlobalGotohSA` — ``getAlignment(seq1, seq2)`` returns an :class:`AlignedSequence`
  exactly like the reference's (``SASmithWaterman.h:358-366`` etc.); ``getAlignments`` aligns a
  batch in one GPU pass.
* :class:`Engine` — the batch C ABI (host or device-resident buffers), align calls and the
  score-only calls (``score*``: scores and end cells, no traceback); ``getScores`` / ``getEndCells``
  on the aligner classes.

There is no CPU fallback: if the HIP library is missing or no GPU is present, calls fail with
:class:`SeqalibError`.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "SA_SW", "SA_NW", "SA_LOCAL_GOTOH", "SA_GLOBAL_GOTOH", "ALGO_NAMES",
    "SeqalibError", "ScoringSystem", "Entry", "AlignedSequence", "PairResult", "Engine",
    "SmithWatermanSA", "NeedlemanWunschSA", "LocalGotohSA", "GlobalGotohSA", "HirschbergSA", "MyersMillerSA",
    "load_library", "library_path", "expand_ops", "synth_dna", "synth_mutate", "synth_dna_batch",
    "SA_FLAG_DIVERGED", "SA_FLAG_BAD_SHAPE", "SA_FLAG_SIZE_HACK", "SA_FLAG_TIMEOUT",
    "SA_RECORDS_NONE", "score_plan_query",
    "SA_FLAG_DROPPED", "SA_XDROP_OFF", "SA_XDROP_PERIOD", "banded_extend_plan_query",
    "SA_FLAG_BAD_BAND", "banded_seeded_device_plan_query",
]

SA_SW, SA_NW, SA_LOCAL_GOTOH, SA_GLOBAL_GOTOH, SA_HIRSCHBERG, SA_MYERS_MILLER = 0, 1, 2, 3, 4, 5
ALGO_NAMES = {SA_SW: "sw", SA_NW: "nw", SA_LOCAL_GOTOH: "local_gotoh", SA_GLOBAL_GOTOH: "global_gotoh",
              SA_HIRSCHBERG: "hirschberg", SA_MYERS_MILLER: "myers_miller"}
SA_FLAG_DIVERGED, SA_FLAG_BAD_SHAPE, SA_FLAG_SIZE_HACK, SA_FLAG_TIMEOUT = 1, 2, 4, 8
SA_KERNEL_INT32, SA_KERNEL_T16, SA_KERNEL_T16_ENDCELL, SA_KERNEL_TINY = 0, 1, 2, 3
SA_KERNEL_BANDED = 4    # banded calls (sa_align_batch_banded / sa_score_batch_banded)
SA_PIPELINE_DEPTH = 2   # pipelined device calls that may run at once (distinct output buffers)
SA_RECORDS_FLAGS, SA_RECORDS_TAGS, SA_RECORDS_SCORE_ONLY = 0, 1, 2
SA_RECORDS_NONE = 3   # score calls on the int32 / small-call kernels: nothing stored for a traceback
SA_RECORDS_BAND2 = 4  # banded align calls: 2 bits per in-band cell, laid out by anti-diagonal
SA_RECORDS_BAND4 = 5  # banded affine align calls: 4 bits per in-band cell
# free_ends of the ends-free banded calls (sa_align_batch_banded_ends_free): which unaligned heads / tails cost nothing
SA_FREE_SEQ1_BEGIN, SA_FREE_SEQ1_END, SA_FREE_SEQ2_BEGIN, SA_FREE_SEQ2_END = 1, 2, 4, 8
# the banded extension calls (sa_align_batch_banded_extend): the flag of a pair the X-drop rule stopped, the
# xdrop that never stops one, and the steps between two checkpoints
SA_FLAG_DROPPED = 32
SA_XDROP_OFF, SA_XDROP_PERIOD = -1, 16
# the device-resident seeded calls (sa_align_batch_banded_seeded_device): a pair whose seed diagonal misses its
# matrix or whose band holds no legal begin / end
SA_FLAG_BAD_BAND = 64
SA_HOOK_HAND_TAG, SA_HOOK_POISON_WS, SA_HOOK_F16 = 1, 2, 3   # sa_test_hook (tests only)
INT32_MIN = -(2 ** 31)

_HERE = os.path.dirname(os.path.abspath(__file__))


class SeqalibError(RuntimeError):
    pass


class _Scoring(C.Structure):
    _fields_ = [("gap", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32),
                ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("allow_mismatch", C.c_int32)]


class _Result(C.Structure):
    _fields_ = [("score", C.c_int32), ("end_i", C.c_int32), ("end_j", C.c_int32),
                ("start_i", C.c_int32), ("start_j", C.c_int32), ("nops", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


RESULT_DTYPE = np.dtype([("score", "<i4"), ("end_i", "<i4"), ("end_j", "<i4"), ("start_i", "<i4"),
                         ("start_j", "<i4"), ("nops", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert RESULT_DTYPE.itemsize == C.sizeof(_Result) == 32

_lib = None


def library_path() -> str:
    return os.environ.get("SEQALIB_HIP_LIB", os.path.join(_HERE, "lib", "libseqalib_hip.so"))


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (same soname as /opt/rocm's).  Two HIP
    runtimes in one process cannot both own the device, so when torch is installed we bind the
    engine to torch's copy (loaded RTLD_GLOBAL by path, without importing torch); a later
    ``import torch`` then maps the very same file.  SEQALIB_HIP_RUNTIME=system disables this."""
    if os.environ.get("SEQALIB_HIP_RUNTIME", "torch") != "torch":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)


def load_library():
    """Load libseqalib_hip.so (built in-tree by ``make`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise SeqalibError(f"HIP engine not built: {path} missing (run `make` or __graft_entry__.build())")
    _share_hip_runtime_with_torch()
    L = C.CDLL(path)
    vp, u8p, u64p, i32p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    L.sa_version.restype = C.c_int
    L.sa_device_count.argtypes = [i32p]
    L.sa_status_string.restype = C.c_char_p
    L.sa_status_string.argtypes = [C.c_int]
    L.sa_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.sa_destroy.argtypes = [vp]
    L.sa_destroy.restype = None
    L.sa_last_error.argtypes = [vp]
    L.sa_last_error.restype = C.c_char_p
    L.sa_set_workspace_limit.argtypes = [vp, C.c_uint64]
    L.sa_trim.argtypes = [vp]
    L.sa_align_batch.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp, vp,
                                 C.c_uint64]
    L.sa_multi_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.sa_multi_destroy.argtypes = [vp]
    L.sa_multi_destroy.restype = None
    L.sa_multi_last_error.argtypes = [vp]
    L.sa_multi_last_error.restype = C.c_char_p
    L.sa_multi_align_batch.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp, vp,
                                       C.c_uint64]
    L.sa_align_batch_bits.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, C.c_uint32, vp, vp, vp, vp,
                                      C.c_uint64]
    L.sa_align_batch_device.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32,
                                        C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sa_score_batch.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp]
    L.sa_multi_score_batch.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp]
    L.sa_score_batch_bits.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, C.c_uint32, vp, vp, vp]
    L.sa_score_batch_device.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32,
                                        C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sa_align_batch_banded.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32,
                                        vp, vp, C.c_uint64]
    L.sa_score_batch_banded.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32,
                                        vp]
    L.sa_banded_plan_query.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, i32p, i32p, u64p]
    L.sa_align_batch_banded_affine.argtypes = L.sa_align_batch_banded.argtypes
    L.sa_score_batch_banded_affine.argtypes = L.sa_score_batch_banded.argtypes
    L.sa_banded_affine_plan_query.argtypes = L.sa_banded_plan_query.argtypes
    L.sa_score_plan_query.argtypes = [C.c_int, C.POINTER(_Scoring), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                      i32p, i32p, i32p, u64p]
    L.sa_align_batch_matrix.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp,
                                        vp, vp, C.c_uint64]
    L.sa_score_batch_matrix.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.sa_matrix_plan_query.argtypes = [C.c_int, C.POINTER(_Scoring), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                       i32p, i32p, i32p, u64p]
    L.sa_align_batch_banded_matrix.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp,
                                               C.c_uint32, vp, vp, C.c_uint64]
    L.sa_score_batch_banded_matrix.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp,
                                               C.c_uint32, vp]
    L.sa_align_batch_banded_ends_free.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp,
                                                  C.c_uint32, C.c_uint32, vp, vp, C.c_uint64]
    L.sa_score_batch_banded_ends_free.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp,
                                                  C.c_uint32, C.c_uint32, vp]
    L.sa_align_batch_banded_seeded.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp,
                                               C.c_uint32, C.c_uint32, vp, vp, C.c_uint64]
    L.sa_score_batch_banded_seeded.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp, vp,
                                               C.c_uint32, C.c_uint32, vp]
    L.sa_banded_seeded_plan_query.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint32, C.c_uint32,
                                              i32p, i32p, u64p]
    L.sa_align_batch_banded_seeded_device.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, C.c_uint64, vp, vp, vp,
                                                      C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                                      C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, vp]
    L.sa_score_batch_banded_seeded_device.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, C.c_uint64, vp, vp, vp,
                                                      C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                                      C.c_uint32, C.c_uint32, vp, vp]
    L.sa_banded_seeded_device_plan_query.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, i32p, u64p, u64p]
    L.sa_align_batch_banded_extend.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp,
                                               C.c_uint32, C.c_int32, vp, vp, C.c_uint64]
    L.sa_score_batch_banded_extend.argtypes = [vp, C.c_int, C.POINTER(_Scoring), vp, vp, vp, vp, C.c_uint32, vp,
                                               C.c_uint32, C.c_int32, vp]
    L.sa_banded_extend_plan_query.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, i32p, i32p, u64p]
    L.sa_last_timings.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i32p]
    L.sa_last_kernel_timings.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.sa_plan_query.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, i32p, i32p, u64p, u64p]
    L.sa_plan_query_ex.argtypes = [C.c_int, C.POINTER(_Scoring), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                   i32p, i32p, i32p, u64p]
    L.sa_last_plan.argtypes = [vp, i32p, i32p, i32p]
    L.sa_last_plan_ex.argtypes = [vp, i32p, i32p, i32p, i32p]
    L.sa_set_pipeline.argtypes = [vp, C.c_int]
    L.sa_wait.argtypes = [vp]
    L.sa_test_hook.argtypes = [vp, C.c_int, C.c_uint64]
    L.sa_synth_dna.argtypes = [C.c_uint64, C.c_uint32, vp]
    L.sa_synth_mutate.argtypes = [vp, C.c_uint32, C.c_uint64, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.sa_synth_dna_batch.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_int]
    for fn in ("sa_set_workspace_limit", "sa_trim", "sa_align_batch", "sa_align_batch_bits", "sa_align_batch_device",
               "sa_multi_create", "sa_multi_align_batch", "sa_score_batch", "sa_score_batch_bits",
               "sa_score_batch_device", "sa_multi_score_batch", "sa_score_plan_query",
               "sa_last_timings", "sa_last_kernel_timings", "sa_last_plan", "sa_last_plan_ex", "sa_plan_query", "sa_plan_query_ex", "sa_synth_dna", "sa_synth_mutate", "sa_synth_dna_batch",
               "sa_align_batch_banded", "sa_score_batch_banded", "sa_banded_plan_query",
               "sa_align_batch_banded_affine", "sa_score_batch_banded_affine", "sa_banded_affine_plan_query",
               "sa_align_batch_matrix", "sa_score_batch_matrix", "sa_matrix_plan_query",
               "sa_align_batch_banded_matrix", "sa_score_batch_banded_matrix",
               "sa_align_batch_banded_ends_free", "sa_score_batch_banded_ends_free",
               "sa_align_batch_banded_seeded", "sa_score_batch_banded_seeded", "sa_banded_seeded_plan_query",
               "sa_align_batch_banded_extend", "sa_score_batch_banded_extend", "sa_banded_extend_plan_query",
               "sa_align_batch_banded_seeded_device", "sa_score_batch_banded_seeded_device",
               "sa_banded_seeded_device_plan_query",
               "sa_create", "sa_device_count", "sa_set_pipeline", "sa_wait", "sa_test_hook"):
        getattr(L, fn).restype = C.c_int
    if L.sa_version() != 1:
        raise SeqalibError("libseqalib_hip ABI version mismatch")
    _lib = L
    return L


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


# ----------------------------------------------------------------------------------- scoring
class ScoringSystem:
    """Mirror of the reference's ScoringSystem (include/SequenceAlignment.h:82-131).

    * ``ScoringSystem(gap, match)``                        -> Mismatch = INT_MIN, AllowMismatch = False
    * ``ScoringSystem(gap, match, mismatch[, allow: bool])``
    * ``ScoringSystem(gap_open, gap_extend, match, mismatch[, allow])`` — four ints pick this
      overload, as in C++.
    Fields the chosen overload leaves uninitialised in the reference are 0 here.
    """

    def __init__(self, *args):
        self.gap = self.match = self.mismatch = self.gap_open = self.gap_extend = 0
        self.allow_mismatch = True
        if len(args) == 2:
            self.gap, self.match = args
            self.mismatch, self.allow_mismatch = INT32_MIN, False
            self.nargs = 2
        elif len(args) == 3 or (len(args) == 4 and isinstance(args[3], bool)):
            self.gap, self.match, self.mismatch = args[:3]
            self.allow_mismatch = bool(args[3]) if len(args) == 4 else True
            self.nargs = len(args)
        elif len(args) in (4, 5):
            self.gap_open, self.gap_extend, self.match, self.mismatch = args[:4]
            self.allow_mismatch = bool(args[4]) if len(args) == 5 else True
            self.nargs = 5
        else:
            raise TypeError("ScoringSystem takes 2, 3, 4 or 5 arguments")

    def getAllowMismatch(self): return self.allow_mismatch
    def getMismatchPenalty(self): return self.mismatch
    def getGapPenalty(self): return self.gap
    def getMatchProfit(self): return self.match
    def getGapOpenPenalty(self): return self.gap_open
    def getGapExtendPenalty(self): return self.gap_extend

    def _c(self) -> _Scoring:
        return _Scoring(self.gap, self.match, self.mismatch, self.gap_open, self.gap_extend,
                        1 if self.allow_mismatch else 0)

    def args(self) -> tuple:
        if self.nargs == 2:
            return (self.gap, self.match)
        if self.nargs in (3, 4):
            return (self.gap, self.match, self.mismatch) + ((self.allow_mismatch,) if self.nargs == 4 else ())
        return (self.gap_open, self.gap_extend, self.match, self.mismatch, self.allow_mismatch)

    def __repr__(self):
        return f"ScoringSystem{self.args()}"


# --------------------------------------------------------------------------------- results
@dataclass
class Entry:
    """AlignedSequence::Entry (include/SequenceAlignment.h:17-53)."""
    first: object
    second: object
    is_match: bool

    def get(self, index: int):
        assert index in (0, 1), "Index out of bounds!"
        return self.first if index == 0 else self.second

    def match(self) -> bool:
        return self.is_match

    def mismatch(self) -> bool:
        return not self.is_match


class AlignedSequence:
    """AlignedSequence<Ty, Blank> (include/SequenceAlignment.h:13-80): an ordered list of Entry."""

    def __init__(self, entries: Optional[List[Entry]] = None, blank="-"):
        self.Data: List[Entry] = entries or []
        self.blank = blank

    def __iter__(self):
        return iter(self.Data)

    def __len__(self):
        return len(self.Data)

    def rows(self) -> Tuple[str, str, str]:
        """The three lines the reference's printAlignment prints (include/Test.cpp:10-31)."""
        r0 = "".join(str(e.first) for e in self.Data)
        bars = "".join("|" if e.is_match else " " for e in self.Data)
        r1 = "".join(str(e.second) for e in self.Data)
        return r0, bars, r1


@dataclass
class PairResult:
    score: int
    end_i: int
    end_j: int
    start_i: int
    start_j: int
    flags: int
    ops: bytes   # traceback order


def expand_ops(algo: int, s1: Sequence, s2: Sequence, r: PairResult, blank="-",
               match_fn: Optional[Callable] = None) -> AlignedSequence:
    """Host half of buildResult: op stream -> Entry list, plus forceGlobal for the local modes
    (SequenceAligner::forceGlobal, include/SequenceAlignment.h:156-189)."""
    local: List[Entry] = []
    i, j = r.end_i, r.end_j
    for op in r.ops:
        c = chr(op)
        if c in "MS":
            local.append(Entry(s1[i - 1], s2[j - 1], c == "M"))
            i -= 1; j -= 1
        elif c == "X":
            local.append(Entry(s1[i - 1], blank, False))
            local.append(Entry(blank, s2[j - 1], False))
            i -= 1; j -= 1
        elif c in "Uu":
            local.append(Entry(s1[i - 1], blank, False))
            if c == "U":
                i -= 1
        elif c in "Ll":
            local.append(Entry(blank, s2[j - 1], False))
            if c == "L":
                j -= 1
        else:
            raise SeqalibError(f"bad op {op!r}")
    local.reverse()   # push_front order -> forward order
    if r.flags & SA_FLAG_SIZE_HACK or algo in (SA_NW, SA_GLOBAL_GOTOH, SA_HIRSCHBERG, SA_MYERS_MILLER):
        return AlignedSequence(local, blank)
    idx1, idx2, end1, end2 = r.start_i, r.start_j, r.end_i, r.end_j
    front = [Entry(s1[k], blank, False) for k in range(idx1)] + [Entry(blank, s2[k], False) for k in range(idx2)]
    back = [Entry(s1[k], blank, False) for k in range(end1, len(s1))] + \
           [Entry(blank, s2[k], False) for k in range(end2, len(s2))]
    return AlignedSequence(front + local + back, blank)


# ---------------------------------------------------------------------------------- engine
def _band_arg(band) -> int:
    band = int(band)
    if band < 0 or band > 0xFFFFFFFF:
        raise SeqalibError(f"band must be in [0, 2^32): {band}")
    return band


def _free_ends_arg(free_ends) -> int:
    free_ends = int(free_ends)
    if free_ends < 0 or free_ends > 0xFFFFFFFF:
        raise SeqalibError(f"free_ends must be an OR of SA_FREE_*: {free_ends}")
    return free_ends


def _diag_arg(diag, npairs: int) -> np.ndarray:
    try:
        d = np.asarray(diag, dtype=np.int64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise SeqalibError(f"diag must be an array of integers: {e}")
    if len(d) != npairs:
        raise SeqalibError(f"diag holds {len(d)} seed diagonals for {npairs} pairs")
    if d.size and (d.min() < -(2 ** 31) or d.max() >= 2 ** 31):
        raise SeqalibError("a seed diagonal does not fit 32 bits")
    return np.ascontiguousarray(d, dtype=np.int32)


def _xdrop_arg(xdrop) -> int:
    xdrop = int(xdrop)
    if xdrop < -(2 ** 31) or xdrop >= 2 ** 31:
        raise SeqalibError(f"xdrop does not fit 32 bits: {xdrop}")   # (the library answers a value below SA_XDROP_OFF)
    return xdrop


def _lut_arg(lut) -> Optional[np.ndarray]:
    return None if lut is None else np.ascontiguousarray(lut, dtype=np.uint8).reshape(65536)


def _as_bytes(s) -> bytes:
    if isinstance(s, (bytes, bytearray)):
        return bytes(s)
    if isinstance(s, str):
        return s.encode("latin-1")
    if isinstance(s, np.ndarray) and s.dtype == np.uint8:
        return s.tobytes()
    raise TypeError("sequences must be str, bytes or uint8 arrays (use the symbol mapping for other types)")


class SubstitutionMatrix:
    """Dense 256 x 256 int16 score table for the matrix calls (sa_align_batch_matrix): table[a, b] is
    the diagonal term of Seq1 symbol a against Seq2 symbol b.

    alphabet: the symbols (str, bytes or ints 0..255) that index `table`;
    table: a K x K array-like (table[i][j] = score of alphabet[i] against alphabet[j], not
           necessarily symmetric), or a dict {(a, b): score} over symbols of the alphabet;
    default: the score of every pair the table does not give (pairs of a dict that are missing,
             symbols outside the alphabet); None leaves those at 0."""

    def __init__(self, alphabet, table, default: Optional[int] = None):
        def sym(x):
            if isinstance(x, str):
                x = ord(x)
            x = int(x)
            if not 0 <= x <= 255:
                raise SeqalibError(f"symbol {x} is not a byte")
            return x

        syms = [sym(x) for x in alphabet]
        if len(set(syms)) != len(syms):
            raise SeqalibError("SubstitutionMatrix: the alphabet repeats a symbol")
        self.alphabet = bytes(syms)
        full = np.full((256, 256), 0 if default is None else int(default), dtype=np.int64)
        if isinstance(table, dict):
            for (a, b), v in table.items():
                a, b = sym(a), sym(b)
                if a not in syms or b not in syms:
                    raise SeqalibError("SubstitutionMatrix: table entry outside the alphabet")
                full[a, b] = int(v)
        else:
            t = np.asarray(table, dtype=np.int64)
            if t.shape != (len(syms), len(syms)):
                raise SeqalibError(f"SubstitutionMatrix: table must be {len(syms)} x {len(syms)}")
            full[np.ix_(syms, syms)] = t
        if full.min() < -32768 or full.max() > 32767:
            raise SeqalibError("SubstitutionMatrix: scores must fit int16")
        self.table = np.ascontiguousarray(full, dtype=np.int16)

    def score(self, a, b) -> int:
        a = ord(a) if isinstance(a, str) else int(a)
        b = ord(b) if isinstance(b, str) else int(b)
        return int(self.table[a, b])


def _submat_arg(matrix) -> np.ndarray:
    t = matrix.table if isinstance(matrix, SubstitutionMatrix) else matrix
    t = np.ascontiguousarray(t, dtype=np.int16)
    if t.size != 65536:
        raise SeqalibError("substitution matrix must be a SubstitutionMatrix or a 256 x 256 int16 table")
    return t.reshape(65536)


def pack_pairs(pairs: Sequence[Tuple[object, object]]):
    """Concatenate pairs into (seq1, off1, seq2, off2) uint8/uint64 arrays."""
    b1 = [_as_bytes(a) for a, _ in pairs]
    b2 = [_as_bytes(b) for _, b in pairs]
    off1 = np.zeros(len(pairs) + 1, dtype=np.uint64)
    off2 = np.zeros(len(pairs) + 1, dtype=np.uint64)
    off1[1:] = np.cumsum([len(x) for x in b1]) if b1 else []
    off2[1:] = np.cumsum([len(x) for x in b2]) if b2 else []
    s1 = np.frombuffer(b"".join(b1), dtype=np.uint8).copy() if b1 else np.zeros(0, np.uint8)
    s2 = np.frombuffer(b"".join(b2), dtype=np.uint8).copy() if b2 else np.zeros(0, np.uint8)
    return s1, off1, s2, off2


def lut_from_fn(fn: Callable[[str, str], bool], alphabet1: Iterable[int], alphabet2: Iterable[int]) -> np.ndarray:
    """256x256 match table from a predicate over characters (the reference's MatchFnTy)."""
    lut = np.zeros((256, 256), dtype=np.uint8)
    for a in alphabet1:
        for b in alphabet2:
            lut[a, b] = 1 if fn(chr(a), chr(b)) else 0
    return lut


def match_bitmaps(pairs: Sequence[Tuple[Sequence, Sequence]], match: Optional[Callable] = None):
    """The generic-Ty input of sa_align_batch_bits for pairs of sequences of ANY symbols (lists or
    tuples of ints, objects, ...): length offsets and per-pair m x n match bitmaps, i.e. the
    reference's cacheAllMatches (SASmithWaterman.h:20-45) packed to bits.  match(a, b) is the
    MatchFnTy; None means equality (the reference's nullptr match fn).  Hashable symbols are coded
    first (by type and value, so 1, 1.0 and True stay distinct), and the predicate runs once per
    distinct (a, b) pair of a pair's sequences."""
    n_p = len(pairs)
    off1 = np.zeros(n_p + 1, dtype=np.uint64)
    off2 = np.zeros(n_p + 1, dtype=np.uint64)
    bits_off = np.zeros(n_p + 1, dtype=np.uint64)
    chunks = []
    for p, (a, b) in enumerate(pairs):
        m, n = len(a), len(b)
        off1[p + 1] = off1[p] + m
        off2[p + 1] = off2[p] + n
        wn = (n + 31) // 32
        if m and n:
            try:
                ua = {}
                c1 = np.fromiter((ua.setdefault((type(x), x), len(ua)) for x in a), dtype=np.int64, count=m)
                ub = {}
                c2 = np.fromiter((ub.setdefault((type(x), x), len(ub)) for x in b), dtype=np.int64, count=n)
                va, vb = [k[1] for k in ua], [k[1] for k in ub]
                if match is None:
                    tab = np.array([[x == y for y in vb] for x in va], dtype=bool)
                else:
                    tab = np.array([[bool(match(x, y)) for y in vb] for x in va], dtype=bool)
                mm = tab[c1][:, c2]
            except TypeError:   # unhashable symbols: evaluate every cell, as the reference does
                f = (lambda x, y: x == y) if match is None else match
                mm = np.array([[bool(f(x, y)) for y in b] for x in a], dtype=bool)
            packed = np.packbits(mm, axis=1, bitorder="little")
            row = np.zeros((m, 4 * wn), dtype=np.uint8)
            row[:, :packed.shape[1]] = packed
            chunks.append(row.reshape(-1).view("<u4"))
        bits_off[p + 1] = bits_off[p] + m * wn
    bits = np.concatenate(chunks) if chunks else np.zeros(1, dtype=np.uint32)
    return off1, off2, np.ascontiguousarray(bits, dtype=np.uint32), bits_off


class Engine:
    """One context per GPU (sa_create).  Not thread-safe; use one Engine per host thread."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.sa_create(device, C.byref(h))
        if rc != 0:
            raise SeqalibError(f"sa_create({device}) failed: {self.L.sa_last_error(None).decode()}")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.sa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.L.sa_last_error(self.h).decode()
            raise SeqalibError(f"{what}: {self.L.sa_status_string(rc).decode()} ({msg})")

    def set_workspace_limit(self, nbytes: int):
        self._check(self.L.sa_set_workspace_limit(self.h, nbytes), "sa_set_workspace_limit")

    def align_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                     s2: np.ndarray, off2: np.ndarray, lut: Optional[np.ndarray] = None, out=None):
        """Host-buffer batch (sa_align_batch).  Returns (results structured array, ops uint8 array).
        out: optional (results, ops) arrays of a previous call with the same shapes, reused as the
        output buffers (a caller that keeps its buffers avoids re-faulting ~m+n bytes per pair)."""
        npairs = len(off1) - 1
        s1 = np.ascontiguousarray(s1, dtype=np.uint8)
        s2 = np.ascontiguousarray(s2, dtype=np.uint8)
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        off2 = np.ascontiguousarray(off2, dtype=np.uint64)
        ops_cap = int(off1[-1] + off2[-1]) + npairs + 1
        if out is not None and out[0].base is not None and len(out[0].base) == max(npairs, 1) \
                and out[0].base.dtype == RESULT_DTYPE and out[1].dtype == np.uint8 and len(out[1]) == ops_cap \
                and out[1].flags.c_contiguous and out[1].flags.writeable:
            res, ops = out[0].base, out[1]
        else:
            res = np.zeros(max(npairs, 1), dtype=RESULT_DTYPE)
            ops = np.zeros(ops_cap, dtype=np.uint8)
        lut_p = 0
        if lut is not None:
            lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(65536)
            lut_p = _ptr(lut)
        sc = scoring._c()
        rc = self.L.sa_align_batch(self.h, algo, C.byref(sc), _ptr(s1), _ptr(off1), _ptr(s2), _ptr(off2),
                                   npairs, lut_p, _ptr(res), _ptr(ops), ops_cap)
        self._check(rc, "sa_align_batch")
        return res[:npairs], ops

    def align_banded_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                            s2: np.ndarray, off2: np.ndarray, band: int, lut: Optional[np.ndarray] = None):
        """Banded host-buffer batch (sa_align_batch_banded): NW / SW over the cells within `band`
        diagonals of each pair's corner-to-corner corridor.  Returns (results, ops) as align_packed."""
        return self._banded_call("sa_align_batch_banded", algo, scoring, s1, off1, s2, off2, band, lut)

    def align_banded_affine_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, band: int, lut: Optional[np.ndarray] = None):
        """Banded affine host-buffer batch (sa_align_batch_banded_affine): LocalGotoh / GlobalGotoh over
        the cells within `band` diagonals of each pair's corridor, raw path (no LocalGotoh size hack).
        Returns (results, ops) as align_packed."""
        return self._banded_call("sa_align_batch_banded_affine", algo, scoring, s1, off1, s2, off2, band, lut)

    def align_banded_ends_free_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                      s2: np.ndarray, off2: np.ndarray, band: int, free_ends: int,
                                      lut: Optional[np.ndarray] = None):
        """Ends-free banded host-buffer batch (sa_align_batch_banded_ends_free): banded NW (SA_NW,
        SA_HIRSCHBERG) or banded GlobalGotoh in which the heads / tails named by `free_ends` (an OR of
        SA_FREE_*) stay unaligned at no cost.  Returns (results, ops) as align_packed."""
        return self._banded_call("sa_align_batch_banded_ends_free", algo, scoring, s1, off1, s2, off2, band, lut,
                                       (_free_ends_arg(free_ends),))

    def score_banded_ends_free_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                      s2: np.ndarray, off2: np.ndarray, band: int, free_ends: int,
                                      lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Ends-free banded score batch (sa_score_batch_banded_ends_free): the results array (start = -1, nops = 0)."""
        return self._banded_call("sa_score_batch_banded_ends_free", algo, scoring, s1, off1, s2, off2, band, lut,
                                       (_free_ends_arg(free_ends),), with_ops=False)

    def align_banded_ends_free(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                               free_ends: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the ends-free banded call."""
        def call(algo, scoring, s1, off1, s2, off2, band, lut):
            return self.align_banded_ends_free_packed(algo, scoring, s1, off1, s2, off2, band, free_ends, lut)
        return self._align_banded_pairs(call, algo, scoring, pairs, band, lut)

    def score_banded_ends_free(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                               free_ends: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the ends-free banded call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_banded_ends_free_packed(algo, scoring, s1, off1, s2, off2, band, free_ends, lut))

    def align_banded_seeded_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, diag, band: int, free_ends: int,
                                   lut: Optional[np.ndarray] = None):
        """Seeded ends-free banded host-buffer batch (sa_align_batch_banded_seeded): the ends-free call with
        pair p's band `band` diagonals either side of its seed diagonal diag[p] (k = j - i; an int32 array
        of npairs).  Returns (results, ops) as align_packed."""
        d = _diag_arg(diag, len(off1) - 1)
        return self._banded_call("sa_align_batch_banded_seeded", algo, scoring, s1, off1, s2, off2, band, lut,
                                       (_free_ends_arg(free_ends),), (_ptr(d),))

    def score_banded_seeded_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, diag, band: int, free_ends: int,
                                   lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Seeded ends-free banded score batch (sa_score_batch_banded_seeded): the results array (start = -1, nops = 0)."""
        d = _diag_arg(diag, len(off1) - 1)
        return self._banded_call("sa_score_batch_banded_seeded", algo, scoring, s1, off1, s2, off2, band, lut,
                                       (_free_ends_arg(free_ends),), (_ptr(d),), with_ops=False)

    def align_banded_seeded(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], diag,
                            band: int, free_ends: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the seeded banded call."""
        def call(algo, scoring, s1, off1, s2, off2, band, lut):
            return self.align_banded_seeded_packed(algo, scoring, s1, off1, s2, off2, diag, band, free_ends, lut)
        return self._align_banded_pairs(call, algo, scoring, pairs, band, lut)

    def score_banded_seeded(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], diag,
                            band: int, free_ends: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the seeded banded call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_banded_seeded_packed(algo, scoring, s1, off1, s2, off2, diag, band, free_ends, lut))

    def align_banded_extend_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, band: int, xdrop: int,
                                   lut: Optional[np.ndarray] = None):
        """Banded X-drop extension host-buffer batch (sa_align_batch_banded_extend): banded NW (SA_NW,
        SA_HIRSCHBERG) or GlobalGotoh anchored at (0, 0) in the band round diagonal 0, ending at its best
        cell; a pair whose score falls more than xdrop below its best stops early (SA_FLAG_DROPPED;
        SA_XDROP_OFF: never).  Returns (results, ops) as align_packed."""
        return self._banded_call("sa_align_batch_banded_extend", algo, scoring, s1, off1, s2, off2, band, lut,
                                 (_xdrop_arg(xdrop),))

    def score_banded_extend_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, band: int, xdrop: int,
                                   lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Banded extension score batch (sa_score_batch_banded_extend): the results array (start = -1, nops = 0)."""
        return self._banded_call("sa_score_batch_banded_extend", algo, scoring, s1, off1, s2, off2, band, lut,
                                 (_xdrop_arg(xdrop),), with_ops=False)

    def align_banded_extend(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                            xdrop: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the banded extension call."""
        def call(algo, scoring, s1, off1, s2, off2, band, lut):
            return self.align_banded_extend_packed(algo, scoring, s1, off1, s2, off2, band, xdrop, lut)
        return self._align_banded_pairs(call, algo, scoring, pairs, band, lut)

    def score_banded_extend(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                            xdrop: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the banded extension call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_banded_extend_packed(algo, scoring, s1, off1, s2, off2, band, xdrop, lut))

    def _packed_call(self, fn, algo, scoring, s1, off1, s2, off2, mid, with_ops):
        """One host-buffer batch call of the banded / matrix families.  mid: the entry point's arguments
        between npairs and results, in order (an array passes as its address, None as NULL); with_ops:
        an align call, which returns (results, ops) -- a score call returns the results alone."""
        npairs = len(off1) - 1
        s1 = np.ascontiguousarray(s1, dtype=np.uint8)
        s2 = np.ascontiguousarray(s2, dtype=np.uint8)
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        off2 = np.ascontiguousarray(off2, dtype=np.uint64)
        res = np.zeros(max(npairs, 1), dtype=RESULT_DTYPE)
        out = [_ptr(res)]
        if with_ops:
            ops_cap = int(off1[-1] + off2[-1]) + npairs + 1
            ops = np.zeros(ops_cap, dtype=np.uint8)
            out += [_ptr(ops), ops_cap]
        # (mid itself stays bound until the call has returned: it is what keeps converted copies alive)
        ptrs = [0 if a is None else _ptr(a) if isinstance(a, np.ndarray) else a for a in mid]
        sc = scoring._c()
        rc = getattr(self.L, fn)(self.h, algo, C.byref(sc), _ptr(s1), _ptr(off1), _ptr(s2), _ptr(off2),
                                 npairs, *ptrs, *out)
        self._check(rc, fn)
        return (res[:npairs], ops) if with_ops else res[:npairs]

    # pre: the call's arguments between match_lut and band (the seeded calls' diag); extra: those after band
    def _banded_call(self, fn, algo, scoring, s1, off1, s2, off2, band, lut, extra=(), pre=(), with_ops=True):
        return self._packed_call(fn, algo, scoring, s1, off1, s2, off2,
                                 (_lut_arg(lut), *pre, _band_arg(band), *extra), with_ops)

    def score_banded_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                            s2: np.ndarray, off2: np.ndarray, band: int, lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Banded score batch (sa_score_batch_banded): the results array (start = -1, nops = 0)."""
        return self._banded_call("sa_score_batch_banded", algo, scoring, s1, off1, s2, off2, band, lut, with_ops=False)

    def score_banded_affine_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, band: int, lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Banded affine score batch (sa_score_batch_banded_affine): the results array (start = -1, nops = 0)."""
        return self._banded_call("sa_score_batch_banded_affine", algo, scoring, s1, off1, s2, off2, band, lut, with_ops=False)

    def align_banded(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                     lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the banded call."""
        return self._align_banded_pairs(self.align_banded_packed, algo, scoring, pairs, band, lut)

    def align_banded_affine(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                            lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the banded affine call."""
        return self._align_banded_pairs(self.align_banded_affine_packed, algo, scoring, pairs, band, lut)

    def _align_banded_pairs(self, call, algo, scoring, pairs, band, lut):
        s1, off1, s2, off2 = pack_pairs(pairs)
        res, ops = call(algo, scoring, s1, off1, s2, off2, band, lut)
        return self._pair_results(res, ops, off1, off2)

    @staticmethod
    def _pair_results(res, ops, off1, off2) -> List[PairResult]:
        """An align call's (results, ops) as PairResults: pair p's ops start at off1[p] + off2[p] + p."""
        out = []
        for p in range(len(res)):
            o = int(off1[p] + off2[p]) + p
            r = res[p]
            out.append(PairResult(int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]),
                                  int(r["start_j"]), int(r["flags"]), ops[o:o + int(r["nops"])].tobytes()))
        return out

    def score_banded(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                     lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the banded call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_banded_packed(algo, scoring, s1, off1, s2, off2, band, lut))

    def score_banded_affine(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], band: int,
                            lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the banded affine call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_banded_affine_packed(algo, scoring, s1, off1, s2, off2, band, lut))

    def align_matrix_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                            s2: np.ndarray, off2: np.ndarray, matrix, lut: Optional[np.ndarray] = None):
        """Substitution-matrix host-buffer batch (sa_align_batch_matrix): the diagonal term is
        matrix[a, b] (a SubstitutionMatrix or a 256 x 256 int16 table); only the gap terms of
        `scoring` are read; `lut` labels diagonal ops 'M' / 'S'.  Returns (results, ops) as align_packed."""
        return self._packed_call("sa_align_batch_matrix", algo, scoring, s1, off1, s2, off2,
                                 (_submat_arg(matrix), _lut_arg(lut)), True)

    def score_matrix_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                            s2: np.ndarray, off2: np.ndarray, matrix, lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Substitution-matrix score batch (sa_score_batch_matrix): the results array (start = -1, nops = 0)."""
        return self._packed_call("sa_score_batch_matrix", algo, scoring, s1, off1, s2, off2,
                                 (_submat_arg(matrix), _lut_arg(lut)), False)

    def align_matrix(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], matrix,
                     lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the matrix call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        res, ops = self.align_matrix_packed(algo, scoring, s1, off1, s2, off2, matrix, lut)
        return self._pair_results(res, ops, off1, off2)

    def score_matrix(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], matrix,
                     lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the matrix call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_matrix_packed(algo, scoring, s1, off1, s2, off2, matrix, lut))

    def align_banded_matrix_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, matrix, band: int,
                                   lut: Optional[np.ndarray] = None):
        """Banded substitution-matrix host-buffer batch (sa_align_batch_banded_matrix): the band of
        align_banded_packed (SW / NW) or align_banded_affine_packed (LocalGotoh / GlobalGotoh) with the
        diagonal term matrix[a, b]; only the gap terms of `scoring` are read; `lut` labels diagonal ops
        'M' / 'S'.  Returns (results, ops) as align_packed."""
        return self._packed_call("sa_align_batch_banded_matrix", algo, scoring, s1, off1, s2, off2,
                                 (_submat_arg(matrix), _lut_arg(lut), _band_arg(band)), True)

    def score_banded_matrix_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                                   s2: np.ndarray, off2: np.ndarray, matrix, band: int,
                                   lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Banded substitution-matrix score batch (sa_score_batch_banded_matrix): the results array
        (start = -1, nops = 0)."""
        return self._packed_call("sa_score_batch_banded_matrix", algo, scoring, s1, off1, s2, off2,
                                 (_submat_arg(matrix), _lut_arg(lut), _band_arg(band)), False)

    def align_banded_matrix(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], matrix,
                            band: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """align() through the banded matrix call."""
        def call(algo, scoring, s1, off1, s2, off2, band, lut):
            return self.align_banded_matrix_packed(algo, scoring, s1, off1, s2, off2, matrix, band, lut)
        return self._align_banded_pairs(call, algo, scoring, pairs, band, lut)

    def score_banded_matrix(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]], matrix,
                            band: int, lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """score() through the banded matrix call."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_banded_matrix_packed(algo, scoring, s1, off1, s2, off2, matrix, band, lut))

    def align_bits(self, algo: int, scoring: ScoringSystem, off1: np.ndarray, off2: np.ndarray, bits: np.ndarray,
                   bits_off: np.ndarray):
        """Generic-Ty batch (sa_align_batch_bits) from match_bitmaps(): (results, ops)."""
        npairs = len(off1) - 1
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        off2 = np.ascontiguousarray(off2, dtype=np.uint64)
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        bits_off = np.ascontiguousarray(bits_off, dtype=np.uint64)
        res = np.zeros(max(npairs, 1), dtype=RESULT_DTYPE)
        ops_cap = int(off1[-1] + off2[-1]) + npairs + 1
        ops = np.zeros(ops_cap, dtype=np.uint8)
        sc = scoring._c()
        rc = self.L.sa_align_batch_bits(self.h, algo, C.byref(sc), _ptr(off1), _ptr(off2), npairs, _ptr(bits),
                                        _ptr(bits_off), _ptr(res), _ptr(ops), ops_cap)
        self._check(rc, "sa_align_batch_bits")
        return res[:npairs], ops

    def align_generic(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[Sequence, Sequence]],
                      match: Optional[Callable] = None) -> List[PairResult]:
        """Align pairs of sequences of any symbol type with any match predicate (the reference's
        templated ContainerType / Ty / MatchFnTy): the symbols stay on the host, the GPU gets the
        match bitmaps.  Expand with expand_ops(algo, a, b, r, blank=...)."""
        off1, off2, bits, bits_off = match_bitmaps(pairs, match)
        res, ops = self.align_bits(algo, scoring, off1, off2, bits, bits_off)
        return self._pair_results(res, ops, off1, off2)

    def align(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]],
              lut: Optional[np.ndarray] = None) -> List[PairResult]:
        s1, off1, s2, off2 = pack_pairs(pairs)
        res, ops = self.align_packed(algo, scoring, s1, off1, s2, off2, lut)
        return self._pair_results(res, ops, off1, off2)

    def align_device(self, algo: int, scoring: ScoringSystem, d_s1: int, d_off1: int, d_s2: int, d_off2: int,
                     npairs: int, max_m: int, max_n: int, d_res: int, d_ops: int, stream: int = 0,
                     d_lut: int = 0):
        """Device-resident batch (sa_align_batch_device); pointers are device addresses."""
        sc = scoring._c()
        rc = self.L.sa_align_batch_device(self.h, algo, C.byref(sc), d_s1, d_off1, d_s2, d_off2, npairs, max_m,
                                          max_n, d_lut or None, d_res, d_ops, stream or None)
        self._check(rc, "sa_align_batch_device")

    def align_banded_seeded_device(self, algo: int, scoring: ScoringSystem, d_seq1: int, seq1_bytes: int, d_start1: int,
                                   d_len1: int, d_seq2: int, seq2_bytes: int, d_start2: int, d_len2: int, npairs: int,
                                   max_m: int, max_n: int, d_diag: int, band: int, free_ends: int, d_res: int, d_ops: int,
                                   d_ops_off: int, ops_bytes: int, stream: int = 0, d_lut: int = 0):
        """Device-resident seeded banded batch (sa_align_batch_banded_seeded_device): pair p is the slices
        d_seq1[start1[p] .. + len1[p]) and d_seq2[start2[p] .. + len2[p]) of two resident buffers, its ops go to
        d_ops + ops_off[p].  Pointers are device addresses (uint64 starts and ops offsets, uint32 lengths, int32
        diagonals); asynchronous on `stream`.  A refused pair has a zero result with SA_FLAG_BAD_SHAPE or
        SA_FLAG_BAD_BAND."""
        sc = scoring._c()
        rc = self.L.sa_align_batch_banded_seeded_device(
            self.h, algo, C.byref(sc), d_seq1 or None, seq1_bytes, d_start1 or None, d_len1 or None, d_seq2 or None,
            seq2_bytes, d_start2 or None, d_len2 or None, npairs, max_m, max_n, d_lut or None, d_diag or None,
            _band_arg(band), _free_ends_arg(free_ends), d_res or None, d_ops or None, d_ops_off or None, ops_bytes,
            stream or None)
        self._check(rc, "sa_align_batch_banded_seeded_device")

    def score_banded_seeded_device(self, algo: int, scoring: ScoringSystem, d_seq1: int, seq1_bytes: int, d_start1: int,
                                   d_len1: int, d_seq2: int, seq2_bytes: int, d_start2: int, d_len2: int, npairs: int,
                                   max_m: int, max_n: int, d_diag: int, band: int, free_ends: int, d_res: int,
                                   stream: int = 0, d_lut: int = 0):
        """Scores and end cells of align_banded_seeded_device's pairs (sa_score_batch_banded_seeded_device):
        start = (-1, -1), nops = 0; no records, no walk, no ops."""
        sc = scoring._c()
        rc = self.L.sa_score_batch_banded_seeded_device(
            self.h, algo, C.byref(sc), d_seq1 or None, seq1_bytes, d_start1 or None, d_len1 or None, d_seq2 or None,
            seq2_bytes, d_start2 or None, d_len2 or None, npairs, max_m, max_n, d_lut or None, d_diag or None,
            _band_arg(band), _free_ends_arg(free_ends), d_res or None, stream or None)
        self._check(rc, "sa_score_batch_banded_seeded_device")

    # ---- score-only calls: scores and end cells, no traceback (include/seqalib_hip.h sa_score_batch)
    def score_packed(self, algo: int, scoring: ScoringSystem, s1: np.ndarray, off1: np.ndarray,
                     s2: np.ndarray, off2: np.ndarray, lut: Optional[np.ndarray] = None) -> np.ndarray:
        """Host-buffer score batch (sa_score_batch): the results structured array (start = -1,
        nops = 0); no op buffer exists anywhere."""
        npairs = len(off1) - 1
        s1 = np.ascontiguousarray(s1, dtype=np.uint8)
        s2 = np.ascontiguousarray(s2, dtype=np.uint8)
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        off2 = np.ascontiguousarray(off2, dtype=np.uint64)
        res = np.zeros(max(npairs, 1), dtype=RESULT_DTYPE)
        lut_p = 0
        if lut is not None:
            lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(65536)
            lut_p = _ptr(lut)
        sc = scoring._c()
        rc = self.L.sa_score_batch(self.h, algo, C.byref(sc), _ptr(s1), _ptr(off1), _ptr(s2), _ptr(off2),
                                   npairs, lut_p, _ptr(res))
        self._check(rc, "sa_score_batch")
        return res[:npairs]

    def score_bits(self, algo: int, scoring: ScoringSystem, off1: np.ndarray, off2: np.ndarray, bits: np.ndarray,
                   bits_off: np.ndarray) -> np.ndarray:
        """Generic-Ty score batch (sa_score_batch_bits) from match_bitmaps(): the results array."""
        npairs = len(off1) - 1
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        off2 = np.ascontiguousarray(off2, dtype=np.uint64)
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        bits_off = np.ascontiguousarray(bits_off, dtype=np.uint64)
        res = np.zeros(max(npairs, 1), dtype=RESULT_DTYPE)
        sc = scoring._c()
        rc = self.L.sa_score_batch_bits(self.h, algo, C.byref(sc), _ptr(off1), _ptr(off2), npairs, _ptr(bits),
                                        _ptr(bits_off), _ptr(res))
        self._check(rc, "sa_score_batch_bits")
        return res[:npairs]

    @staticmethod
    def _score_results(res: np.ndarray) -> List[PairResult]:
        return [PairResult(int(r["score"]), int(r["end_i"]), int(r["end_j"]), int(r["start_i"]), int(r["start_j"]),
                           int(r["flags"]), b"") for r in res]

    def score_generic(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[Sequence, Sequence]],
                      match: Optional[Callable] = None) -> List[PairResult]:
        """score() for pairs of sequences of any symbol type with any match predicate (match bitmaps)."""
        off1, off2, bits, bits_off = match_bitmaps(pairs, match)
        return self._score_results(self.score_bits(algo, scoring, off1, off2, bits, bits_off))

    def score(self, algo: int, scoring: ScoringSystem, pairs: Sequence[Tuple[object, object]],
              lut: Optional[np.ndarray] = None) -> List[PairResult]:
        """Scores and end cells of a batch; PairResult.ops is b"", start_i = start_j = -1."""
        s1, off1, s2, off2 = pack_pairs(pairs)
        return self._score_results(self.score_packed(algo, scoring, s1, off1, s2, off2, lut))

    def score_device(self, algo: int, scoring: ScoringSystem, d_s1: int, d_off1: int, d_s2: int, d_off2: int,
                     npairs: int, max_m: int, max_n: int, d_res: int, stream: int = 0, d_lut: int = 0):
        """Device-resident score batch (sa_score_batch_device); pointers are device addresses.  Works
        with set_pipeline(True), interleaved with align_device calls."""
        sc = scoring._c()
        rc = self.L.sa_score_batch_device(self.h, algo, C.byref(sc), d_s1, d_off1, d_s2, d_off2, npairs, max_m,
                                          max_n, d_lut or None, d_res, stream or None)
        self._check(rc, "sa_score_batch_device")

    def set_pipeline(self, enable: bool):
        """Overlap consecutive align_device calls (sa_set_pipeline); results need wait()."""
        self._check(self.L.sa_set_pipeline(self.h, 1 if enable else 0), "sa_set_pipeline")

    def test_hook(self, hook: int, value: int) -> int:
        """Tests only (sa_test_hook): SA_HOOK_HAND_TAG / SA_HOOK_POISON_WS / SA_HOOK_F16 (value 2:
        returns 1 when the context turned the f16 cell off)."""
        rc = self.L.sa_test_hook(self.h, hook, value)
        if rc > 0:
            return rc
        self._check(rc, "sa_test_hook")
        return 0

    def wait(self):
        """Wait for all pipelined align_device work (sa_wait)."""
        self._check(self.L.sa_wait(self.h), "sa_wait")

    def last_timings(self) -> Tuple[float, float, int]:
        f, t, n = C.c_float(), C.c_float(), C.c_int()
        self._check(self.L.sa_last_timings(self.h, C.byref(f), C.byref(t), C.byref(n)), "sa_last_timings")
        return f.value, t.value, n.value

    def last_kernel_timings(self) -> Tuple[float, float]:
        """(fill kernels alone, fill stream = fill + end-cell replay) of the last call, ms; the call
        must have run with $SEQALIB_KERNEL_TIMING set."""
        f, s = C.c_float(), C.c_float()
        self._check(self.L.sa_last_kernel_timings(self.h, C.byref(f), C.byref(s)), "sa_last_kernel_timings")
        return f.value, s.value


    def last_plan_ex(self) -> Tuple[int, int, int, int]:
        """last_plan() plus the records the fill stored (SA_RECORDS_FLAGS / _TAGS / _SCORE_ONLY)."""
        k, R, W, rec = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.sa_last_plan_ex(self.h, C.byref(k), C.byref(R), C.byref(W), C.byref(rec)), "sa_last_plan_ex")
        return k.value, R.value, W.value, rec.value

    def last_plan(self) -> Tuple[int, int, int]:
        """(kernel, R, W) of the last call: kernel is SA_KERNEL_INT32, SA_KERNEL_T16,
        or SA_KERNEL_T16_ENDCELL; W = 0 for the multi-workgroup plan (one single-wave workgroup per
        band of 64*R rows)."""
        k, R, W = C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.sa_last_plan(self.h, C.byref(k), C.byref(R), C.byref(W)), "sa_last_plan")
        return k.value, R.value, W.value


def plan_query(algo: int, max_m: int, max_n: int, npairs: int):
    L = load_library()
    R, W = C.c_int(), C.c_int()
    db, rb = C.c_uint64(), C.c_uint64()
    rc = L.sa_plan_query(algo, max_m, max_n, npairs, C.byref(R), C.byref(W), C.byref(db), C.byref(rb))
    if rc:
        raise SeqalibError("sa_plan_query failed")
    return R.value, W.value, db.value, rb.value


def plan_query_ex(algo: int, scoring: "ScoringSystem", max_m: int, max_n: int, npairs: int, nsym: int = 4):
    """(kernel, R, W, workspace bytes per pair) the engine selects for a batch with `nsym`
    distinct symbols under `scoring` (sa_plan_query_ex)."""
    L = load_library()
    k, R, W, ws = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    sc = scoring._c()
    rc = L.sa_plan_query_ex(algo, C.byref(sc), max_m, max_n, npairs, nsym, C.byref(k), C.byref(R), C.byref(W),
                            C.byref(ws))
    if rc:
        raise SeqalibError("sa_plan_query_ex failed")
    return k.value, R.value, W.value, ws.value


def banded_plan_query(algo: int, max_m: int, max_n: int, band: int, npairs: int = 1):
    """(cells per lane and step, pairs per wave, workspace bytes per pair) of the banded path for a
    pair of max_m x max_n at half-width `band` (sa_banded_plan_query).  Raises outside its limits."""
    L = load_library()
    R, ppw, ws = C.c_int(), C.c_int(), C.c_uint64()
    rc = L.sa_banded_plan_query(algo, max_m, max_n, _band_arg(band), npairs, C.byref(R), C.byref(ppw), C.byref(ws))
    if rc:
        raise SeqalibError(f"sa_banded_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return R.value, ppw.value, ws.value


def banded_affine_plan_query(algo: int, max_m: int, max_n: int, band: int, npairs: int = 1):
    """banded_plan_query for the banded affine calls (sa_banded_affine_plan_query): cells per lane and
    step (at most 16: up to 2048 diagonals inside the matrix), pairs per wave, bytes of 4-bit records."""
    L = load_library()
    R, ppw, ws = C.c_int(), C.c_int(), C.c_uint64()
    rc = L.sa_banded_affine_plan_query(algo, max_m, max_n, _band_arg(band), npairs, C.byref(R), C.byref(ppw), C.byref(ws))
    if rc:
        raise SeqalibError(f"sa_banded_affine_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return R.value, ppw.value, ws.value


def banded_seeded_plan_query(algo: int, m: int, n: int, diag: int, band: int, free_ends: int):
    """(cells per lane and step, pairs per wave, record bytes) of the seeded banded calls for one pair of
    m x n seeded at diagonal `diag` (sa_banded_seeded_plan_query).  Raises where the calls refuse the shape:
    a diagonal outside the matrix, a band with no legal begin or end, a band wider than the path holds."""
    L = load_library()
    R, ppw, ws = C.c_int(), C.c_int(), C.c_uint64()
    rc = L.sa_banded_seeded_plan_query(algo, m, n, int(diag), _band_arg(band), _free_ends_arg(free_ends),
                                       C.byref(R), C.byref(ppw), C.byref(ws))
    if rc:
        raise SeqalibError(f"sa_banded_seeded_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return R.value, ppw.value, ws.value


def banded_seeded_device_plan_query(algo: int, max_m: int, max_n: int, band: int):
    """(cells per lane of the widest variant a pair inside max_m x max_n can take, record bytes provisioned per
    pair, plan bytes per pair) of the device-resident seeded calls (sa_banded_seeded_device_plan_query).  Raises
    where the calls refuse the bound shape."""
    L = load_library()
    R, rec, plan = C.c_int(), C.c_uint64(), C.c_uint64()
    rc = L.sa_banded_seeded_device_plan_query(algo, max_m, max_n, _band_arg(band), C.byref(R), C.byref(rec), C.byref(plan))
    if rc:
        raise SeqalibError(f"sa_banded_seeded_device_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return R.value, rec.value, plan.value


def banded_extend_plan_query(algo: int, m: int, n: int, band: int):
    """(cells per lane and step, pairs per wave, record bytes) of the banded extension calls for one pair of
    m x n (sa_banded_extend_plan_query).  Raises where the calls refuse the shape."""
    L = load_library()
    R, ppw, ws = C.c_int(), C.c_int(), C.c_uint64()
    rc = L.sa_banded_extend_plan_query(algo, m, n, _band_arg(band), C.byref(R), C.byref(ppw), C.byref(ws))
    if rc:
        raise SeqalibError(f"sa_banded_extend_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return R.value, ppw.value, ws.value


def matrix_plan_query(algo: int, scoring: "ScoringSystem", max_m: int, max_n: int, npairs: int, nsym: int = 20):
    """(kernel, R, W, workspace bytes per pair) of sa_align_batch_matrix for a batch of this shape with
    nsym distinct symbols (sa_matrix_plan_query; no GPU needed)."""
    L = load_library()
    k, r, w, ws = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    sc = scoring._c()
    rc = L.sa_matrix_plan_query(algo, C.byref(sc), max_m, max_n, npairs, nsym, C.byref(k), C.byref(r), C.byref(w),
                                C.byref(ws))
    if rc != 0:
        raise SeqalibError(f"sa_matrix_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return k.value, r.value, w.value, ws.value


def score_plan_query(algo: int, scoring: "ScoringSystem", max_m: int, max_n: int, npairs: int, nsym: int = 4):
    """plan_query_ex for a host score call (sa_score_plan_query): with nsym > 4 the record-free int32
    fill, whose workspace per pair holds no direction records.  SA_MYERS_MILLER raises."""
    L = load_library()
    k, R, W, ws = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    sc = scoring._c()
    rc = L.sa_score_plan_query(algo, C.byref(sc), max_m, max_n, npairs, nsym, C.byref(k), C.byref(R), C.byref(W),
                               C.byref(ws))
    if rc:
        raise SeqalibError(f"sa_score_plan_query: {L.sa_status_string(rc).decode()} ({L.sa_last_error(None).decode()})")
    return k.value, R.value, W.value, ws.value


# ------------------------------------------------------------------- synthetic inputs (host)
def synth_dna(seed: int, length: int) -> bytes:
    L = load_library()
    out = np.zeros(length, dtype=np.uint8)
    if L.sa_synth_dna(seed, length, _ptr(out)):
        raise SeqalibError("sa_synth_dna failed")
    return out.tobytes()


def synth_mutate(src: bytes, seed: int) -> bytes:
    L = load_library()
    a = np.frombuffer(src, dtype=np.uint8).copy()
    cap = 2 * len(src) + 16
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_uint32()
    if L.sa_synth_mutate(_ptr(a), len(src), seed, _ptr(out), cap, C.byref(n)):
        raise SeqalibError("sa_synth_mutate failed")
    return out[: n.value].tobytes()


def synth_dna_batch(base: int, npairs: int, len1: int, len2: int, threads: int = 8):
    L = load_library()
    s1 = np.zeros(npairs * len1, dtype=np.uint8)
    s2 = np.zeros(npairs * len2, dtype=np.uint8)
    o1 = np.zeros(npairs + 1, dtype=np.uint64)
    o2 = np.zeros(npairs + 1, dtype=np.uint64)
    if L.sa_synth_dna_batch(base, npairs, len1, len2, _ptr(s1), _ptr(o1), _ptr(s2), _ptr(o2), threads):
        raise SeqalibError("sa_synth_dna_batch failed")
    return s1, o1, s2, o2


# ------------------------------------------------------------- reference-shaped aligners
_engines = {}


def _engine(device: int = 0) -> Engine:
    e = _engines.get(device)
    if e is None:
        e = _engines[device] = Engine(device)
    return e


class _Aligner:
    ALGO = SA_SW

    def __init__(self, scoring: Optional[ScoringSystem] = None, match=None, device: int = 0, blank="-", matrix=None):
        """matrix: a SubstitutionMatrix (or 256 x 256 int16 table); the aligner then scores diagonal
        moves with it through the matrix calls (the scoring's gap terms still apply, `match` only
        labels matching pairs).  SmithWatermanSA, NeedlemanWunschSA, LocalGotohSA and GlobalGotohSA."""
        self.scoring = scoring if scoring is not None else self.getDefaultScoring()
        self.match_fn = match
        if matrix is not None and self.ALGO in (SA_HIRSCHBERG, SA_MYERS_MILLER):
            raise SeqalibError(f"{type(self).__name__} does not take a substitution matrix")
        self.matrix = None if matrix is None else _submat_arg(matrix)
        self.device = device
        self.blank = blank
        self.last: Optional[PairResult] = None

    @staticmethod
    def getDefaultScoring() -> ScoringSystem:
        return ScoringSystem(-1, 2, -1)

    def getScoring(self):
        return self.scoring

    def getMatchOperation(self):
        return self.match_fn

    def _lut(self, pairs):
        if self.match_fn is None:
            return None
        al1 = sorted({c for a, _ in pairs for c in _as_bytes(a)})
        al2 = sorted({c for _, b in pairs for c in _as_bytes(b)})
        return lut_from_fn(self.match_fn, al1, al2)

    def getAlignments(self, pairs: Sequence[Tuple[object, object]], band: Optional[int] = None) -> List[AlignedSequence]:
        """band: half-width of the banded call (NeedlemanWunschSA, HirschbergSA = NW, SmithWatermanSA;
        the other aligners raise SeqalibError -- LocalGotohSA and GlobalGotohSA band through
        getBandedAlignments / getBandedScores instead); None: the unbanded path."""
        eng = _engine(self.device)
        if self.matrix is not None:
            if band is not None:
                raise SeqalibError("a substitution matrix and band= cannot be combined here: use getBandedMatrixAlignments / getBandedMatrixScores")
            res = eng.align_matrix(self.ALGO, self.scoring, pairs, self.matrix, self._lut(pairs))
        elif band is None:
            res = eng.align(self.ALGO, self.scoring, pairs, self._lut(pairs))
        else:
            res = eng.align_banded(self.ALGO, self.scoring, pairs, band, self._lut(pairs))
        out = []
        for (a, b), r in zip(pairs, res):
            if r.flags & SA_FLAG_DIVERGED:
                raise SeqalibError("the reference traceback does not terminate for this scoring")
            if r.flags & SA_FLAG_TIMEOUT:
                raise SeqalibError("device hand-off timed out; result invalid")
            out.append(expand_ops(self.ALGO if not (r.flags & SA_FLAG_SIZE_HACK) else SA_NW,
                                  a, b, r, self.blank))
        self.last = res[-1] if res else None
        return out

    def getAlignment(self, seq1, seq2, band: Optional[int] = None) -> AlignedSequence:
        return self.getAlignments([(seq1, seq2)], band=band)[0]

    def getScore(self) -> Optional[int]:
        return None if self.last is None else self.last.score

    def _score_results(self, pairs, band: Optional[int] = None) -> List[PairResult]:
        if self.matrix is not None:
            if band is not None:
                raise SeqalibError("a substitution matrix and band= cannot be combined here: use getBandedMatrixAlignments / getBandedMatrixScores")
            res = _engine(self.device).score_matrix(self.ALGO, self.scoring, pairs, self.matrix, self._lut(pairs))
        elif band is None:
            res = _engine(self.device).score(self.ALGO, self.scoring, pairs, self._lut(pairs))
        else:
            res = _engine(self.device).score_banded(self.ALGO, self.scoring, pairs, band, self._lut(pairs))
        for r in res:
            if r.flags & SA_FLAG_TIMEOUT:
                raise SeqalibError("device hand-off timed out; result invalid")
        self.last = res[-1] if res else None
        return res

    def getScores(self, pairs: Sequence[Tuple[object, object]], band: Optional[int] = None) -> List[int]:
        """The getScore() of every pair in one GPU pass with no traceback; getScore() afterwards is
        the last pair's.  band: as getAlignments (it raises on the Gotoh classes: getBandedScores)."""
        return [r.score for r in self._score_results(pairs, band)]


    def _ends_free_check(self):
        if self.ALGO not in (SA_NW, SA_HIRSCHBERG, SA_GLOBAL_GOTOH):
            raise SeqalibError(f"{type(self).__name__} has no ends-free form: NeedlemanWunschSA, HirschbergSA (= NW) and GlobalGotohSA do")
        if self.matrix is not None:
            raise SeqalibError("a substitution matrix and free ends cannot be combined: the ends-free banded calls take match / mismatch scorings")

    def getEndsFreeAlignments(self, pairs: Sequence[Tuple[object, object]], band: int, free_ends: int) -> List[AlignedSequence]:
        """Semi-global banded alignments (sa_align_batch_banded_ends_free; NeedlemanWunschSA, HirschbergSA =
        NW, GlobalGotohSA; the other aligners raise SeqalibError): the heads / tails named by free_ends
        (an OR of SA_FREE_*) stay unaligned at no cost.  The aligned core comes from the ops; the free
        ends are printed the way forceGlobal prints a local alignment's."""
        self._ends_free_check()
        res = _engine(self.device).align_banded_ends_free(self.ALGO, self.scoring, pairs, band, free_ends, self._lut(pairs))
        self.last = res[-1] if res else None
        return [expand_ops(SA_SW, a, b, r, self.blank) for (a, b), r in zip(pairs, res)]   # (SA_SW: forceGlobal over (start, end))

    def getEndsFreeAlignment(self, seq1, seq2, band: int, free_ends: int) -> AlignedSequence:
        return self.getEndsFreeAlignments([(seq1, seq2)], band, free_ends)[0]

    def _ends_free_score_results(self, pairs, band: int, free_ends: int) -> List[PairResult]:
        self._ends_free_check()
        res = _engine(self.device).score_banded_ends_free(self.ALGO, self.scoring, pairs, band, free_ends, self._lut(pairs))
        self.last = res[-1] if res else None
        return res

    def getEndsFreeScores(self, pairs: Sequence[Tuple[object, object]], band: int, free_ends: int) -> List[int]:
        return [r.score for r in self._ends_free_score_results(pairs, band, free_ends)]

    def getEndsFreeEndCells(self, pairs: Sequence[Tuple[object, object]], band: int, free_ends: int) -> List[Tuple[int, int]]:
        """(end_i, end_j) of every pair: the last row-major candidate of the last row / column holding the maximum."""
        return [(r.end_i, r.end_j) for r in self._ends_free_score_results(pairs, band, free_ends)]


    def _seeded_check(self, pairs, diags):
        if self.ALGO not in (SA_NW, SA_HIRSCHBERG, SA_GLOBAL_GOTOH):
            raise SeqalibError(f"{type(self).__name__} has no seeded form: NeedlemanWunschSA, HirschbergSA (= NW) and GlobalGotohSA do")
        if self.matrix is not None:
            raise SeqalibError("a substitution matrix and a seeded band cannot be combined: the seeded banded calls take match / mismatch scorings")
        return _diag_arg(diags, len(pairs))

    def getSeededAlignments(self, pairs: Sequence[Tuple[object, object]], diags, band: int, free_ends: int) -> List[AlignedSequence]:
        """getEndsFreeAlignments with pair p's band `band` diagonals either side of its seed diagonal
        diags[p] (k = j - i; sa_align_batch_banded_seeded), so the band's width does not grow with the
        longer sequence.  NeedlemanWunschSA, HirschbergSA = NW, GlobalGotohSA; the other aligners raise
        SeqalibError, as does a diags of another length than pairs."""
        d = self._seeded_check(pairs, diags)
        res = _engine(self.device).align_banded_seeded(self.ALGO, self.scoring, pairs, d, band, free_ends, self._lut(pairs))
        self.last = res[-1] if res else None
        return [expand_ops(SA_SW, a, b, r, self.blank) for (a, b), r in zip(pairs, res)]   # (SA_SW: forceGlobal over (start, end))

    def getSeededAlignment(self, seq1, seq2, diag: int, band: int, free_ends: int) -> AlignedSequence:
        return self.getSeededAlignments([(seq1, seq2)], [diag], band, free_ends)[0]

    def _seeded_score_results(self, pairs, diags, band: int, free_ends: int) -> List[PairResult]:
        d = self._seeded_check(pairs, diags)
        res = _engine(self.device).score_banded_seeded(self.ALGO, self.scoring, pairs, d, band, free_ends, self._lut(pairs))
        self.last = res[-1] if res else None
        return res

    def getSeededScores(self, pairs: Sequence[Tuple[object, object]], diags, band: int, free_ends: int) -> List[int]:
        return [r.score for r in self._seeded_score_results(pairs, diags, band, free_ends)]

    def getSeededEndCells(self, pairs: Sequence[Tuple[object, object]], diags, band: int, free_ends: int) -> List[Tuple[int, int]]:
        """(end_i, end_j) of every pair, as getEndsFreeEndCells."""
        return [(r.end_i, r.end_j) for r in self._seeded_score_results(pairs, diags, band, free_ends)]


    def _extension_check(self):
        if self.ALGO not in (SA_NW, SA_HIRSCHBERG, SA_GLOBAL_GOTOH):
            raise SeqalibError(f"{type(self).__name__} has no extension form: NeedlemanWunschSA, HirschbergSA (= NW) and GlobalGotohSA do")
        if self.matrix is not None:
            raise SeqalibError("a substitution matrix and an extension cannot be combined: the banded extension calls take match / mismatch scorings")

    def getExtensionAlignments(self, pairs: Sequence[Tuple[object, object]], band: int, xdrop: int) -> List[AlignedSequence]:
        """X-drop extensions (sa_align_batch_banded_extend; NeedlemanWunschSA, HirschbergSA = NW,
        GlobalGotohSA; the other aligners raise SeqalibError): each pair aligned from its first symbols
        on, inside `band` diagonals either side of the main one, up to the cell of its best score; a pair
        whose score falls more than xdrop below its best is abandoned there (SA_XDROP_OFF: never).  The
        aligned prefix comes from the ops; the unextended tails are printed the way forceGlobal prints a
        local alignment's."""
        self._extension_check()
        res = _engine(self.device).align_banded_extend(self.ALGO, self.scoring, pairs, band, xdrop, self._lut(pairs))
        self.last = res[-1] if res else None
        return [expand_ops(SA_SW, a, b, r, self.blank) for (a, b), r in zip(pairs, res)]   # (SA_SW: forceGlobal over (start, end))

    def getExtensionAlignment(self, seq1, seq2, band: int, xdrop: int) -> AlignedSequence:
        return self.getExtensionAlignments([(seq1, seq2)], band, xdrop)[0]

    def _extension_score_results(self, pairs, band: int, xdrop: int) -> List[PairResult]:
        self._extension_check()
        res = _engine(self.device).score_banded_extend(self.ALGO, self.scoring, pairs, band, xdrop, self._lut(pairs))
        self.last = res[-1] if res else None
        return res

    def getExtensionScores(self, pairs: Sequence[Tuple[object, object]], band: int, xdrop: int) -> List[int]:
        return [r.score for r in self._extension_score_results(pairs, band, xdrop)]

    def getExtensionEndCells(self, pairs: Sequence[Tuple[object, object]], band: int, xdrop: int) -> List[Tuple[int, int]]:
        """(end_i, end_j) of every pair: the last row-major cell holding the extension's maximum, (0, 0) if none is positive."""
        return [(r.end_i, r.end_j) for r in self._extension_score_results(pairs, band, xdrop)]

    def getExtensionDropped(self, pairs: Sequence[Tuple[object, object]], band: int, xdrop: int) -> List[bool]:
        """Whether the X-drop rule stopped each pair (SA_FLAG_DROPPED)."""
        return [bool(r.flags & SA_FLAG_DROPPED) for r in self._extension_score_results(pairs, band, xdrop)]


class _LocalAligner(_Aligner):
    def getEndCells(self, pairs: Sequence[Tuple[object, object]], band: Optional[int] = None) -> List[Tuple[int, int]]:
        """(MaxRow, MaxCol) of every pair -- the last row-major cell holding the maximum (band: the
        last in-band one; it raises on LocalGotohSA, whose banded form is getBandedEndCells)."""
        return [(r.end_i, r.end_j) for r in self._score_results(pairs, band)]


class _BandedMatrix:
    """The banded matrix calls (sa_align_batch_banded_matrix) on the four classes that take a
    substitution matrix.  They are separate methods because band= on getAlignments / getScores and
    getBanded* keep raising on an aligner built with matrix=.  Results are the raw path's (no
    LocalGotoh size hack)."""

    def _banded_matrix_check(self):
        if self.matrix is None:
            raise SeqalibError("getBandedMatrix* need an aligner built with matrix=")

    def getBandedMatrixAlignments(self, pairs: Sequence[Tuple[object, object]], band: int) -> List[AlignedSequence]:
        self._banded_matrix_check()
        res = _engine(self.device).align_banded_matrix(self.ALGO, self.scoring, pairs, self.matrix, band, self._lut(pairs))
        self.last = res[-1] if res else None
        return [expand_ops(self.ALGO, a, b, r, self.blank) for (a, b), r in zip(pairs, res)]

    def getBandedMatrixAlignment(self, seq1, seq2, band: int) -> AlignedSequence:
        return self.getBandedMatrixAlignments([(seq1, seq2)], band)[0]

    def _banded_matrix_score_results(self, pairs, band: int) -> List[PairResult]:
        self._banded_matrix_check()
        res = _engine(self.device).score_banded_matrix(self.ALGO, self.scoring, pairs, self.matrix, band, self._lut(pairs))
        self.last = res[-1] if res else None
        return res

    def getBandedMatrixScores(self, pairs: Sequence[Tuple[object, object]], band: int) -> List[int]:
        return [r.score for r in self._banded_matrix_score_results(pairs, band)]


class _BandedMatrixLocal(_BandedMatrix):
    def getBandedMatrixEndCells(self, pairs: Sequence[Tuple[object, object]], band: int) -> List[Tuple[int, int]]:
        """(MaxRow, MaxCol) of every pair: the last in-band row-major cell holding the maximum."""
        return [(r.end_i, r.end_j) for r in self._banded_matrix_score_results(pairs, band)]


class _BandedAffine:
    """The banded affine calls on LocalGotohSA / GlobalGotohSA.  They are separate methods because
    band= on getAlignments / getScores keeps raising for these classes.  Results are the raw path's
    (no LocalGotoh size hack); with a substitution matrix the banded form is getBandedMatrix*."""

    def _banded_affine_check(self):
        if self.matrix is not None:
            raise SeqalibError("a substitution matrix and a band cannot be combined here: use getBandedMatrixAlignments / getBandedMatrixScores")

    def getBandedAlignments(self, pairs: Sequence[Tuple[object, object]], band: int) -> List[AlignedSequence]:
        self._banded_affine_check()
        res = _engine(self.device).align_banded_affine(self.ALGO, self.scoring, pairs, band, self._lut(pairs))
        self.last = res[-1] if res else None
        return [expand_ops(self.ALGO, a, b, r, self.blank) for (a, b), r in zip(pairs, res)]

    def getBandedAlignment(self, seq1, seq2, band: int) -> AlignedSequence:
        return self.getBandedAlignments([(seq1, seq2)], band)[0]

    def _banded_score_results(self, pairs, band: int) -> List[PairResult]:
        self._banded_affine_check()
        res = _engine(self.device).score_banded_affine(self.ALGO, self.scoring, pairs, band, self._lut(pairs))
        self.last = res[-1] if res else None
        return res

    def getBandedScores(self, pairs: Sequence[Tuple[object, object]], band: int) -> List[int]:
        return [r.score for r in self._banded_score_results(pairs, band)]


class SmithWatermanSA(_LocalAligner, _BandedMatrixLocal):
    ALGO = SA_SW

    @staticmethod
    def getDefaultScoring():
        return ScoringSystem(-1, 1, -1)   # SASmithWaterman.h:352


class NeedlemanWunschSA(_Aligner, _BandedMatrix):
    ALGO = SA_NW


class LocalGotohSA(_LocalAligner, _BandedAffine, _BandedMatrixLocal):
    ALGO = SA_LOCAL_GOTOH

    def getBandedEndCells(self, pairs: Sequence[Tuple[object, object]], band: int) -> List[Tuple[int, int]]:
        """(MaxRow, MaxCol) of every pair: the last in-band row-major cell holding the maximum."""
        return [(r.end_i, r.end_j) for r in self._banded_score_results(pairs, band)]


class HirschbergSA(_Aligner):
    """HirschbergSA (SAHirschberg.h): linear-space NW with the reference's own split/tie rules.
    Default scoring is NeedlemanWunschSA's (-1, 2, -1) (:166-167)."""
    ALGO = SA_HIRSCHBERG


class GlobalGotohSA(_Aligner, _BandedAffine, _BandedMatrix):
    ALGO = SA_GLOBAL_GOTOH


class MyersMillerSA(_Aligner):
    """MyersMillerSA (SAMyersMiller.h): linear-space affine global alignment with the reference's
    own midpoint/tie rules and base cases.  Default scoring (-1, 2, -1) (:406) leaves the affine
    terms unset in the reference; pass a 4/5-argument ScoringSystem."""
    ALGO = SA_MYERS_MILLER

    @staticmethod
    def getDefaultScoring():
        return ScoringSystem(-1, 2, -1)
