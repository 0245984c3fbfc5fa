/* seqalib_hip.h — C ABI of the MI355X (gfx950) pairwise-alignment engine (libseqalib_hip.so).
 *
 * This is the drop-in boundary for the reference's DP hot path (przemektmalon/SeqALib):
 *   SequenceAligner::getAlignment (include/SequenceAlignment.h:153) as implemented by
 *     SmithWatermanSA::getAlignment   (include/SASmithWaterman.h:358-366)
 *     NeedlemanWunschSA::getAlignment (include/SANeedlemanWunsch.h:256-264)
 *     LocalGotohSA::getAlignment      (include/SALocalGotoh.h:518-526)
 *     GlobalGotohSA::getAlignment     (include/SAGlobalGotoh.h:450-459)
 * i.e. cacheAllMatches -> computeScoreMatrix -> buildResult, batched over independent pairs.
 * The header-only C++ API in include/seqalib/ (same class names and templates as the
 * reference) sits on top of this ABI; forceGlobal and the AlignedSequence list are built on the
 * host from the op stream returned here.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every function returns an int
 * status (SA_OK = 0, negative on error) and never throws; sa_last_error() explains the last
 * failure on a context.  A context is bound to one device and must be used from one host thread
 * at a time (one context per GPU for multi-GPU work).
 */
#ifndef SEQALIB_HIP_H
#define SEQALIB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_ABI_VERSION 1

/* Algorithms on the path. */
enum {
    SA_SW = 0,            /* SmithWatermanSA   — linear gap, local  (SASmithWaterman.h)   */
    SA_NW = 1,            /* NeedlemanWunschSA — linear gap, global (SANeedlemanWunsch.h) */
    SA_LOCAL_GOTOH = 2,   /* LocalGotohSA      — affine gap, local  (SALocalGotoh.h)      */
    SA_GLOBAL_GOTOH = 3,  /* GlobalGotohSA     — affine gap, global (SAGlobalGotoh.h)     */
    SA_HIRSCHBERG = 4,    /* HirschbergSA      — linear gap, global, linear space (SAHirschberg.h):
                             the reference's own split/tie rules, not just an optimal alignment;
                             score = NW H[m][n]; ops in traceback order like NW */
    SA_MYERS_MILLER = 5   /* MyersMillerSA     — affine gap, global, linear space (SAMyersMiller.h):
                             the reference's own midpoint/tie rules and base cases; reads
                             gap_open/gap_extend/match/mismatch/allow_mismatch; score = the top
                             call's optimum (the reference exposes none); ops like NW */
};

/* Status codes. */
enum {
    SA_OK = 0,
    SA_ERR_ARG = -1,          /* bad argument (null pointer, bad algo, inconsistent sizes)  */
    SA_ERR_HIP = -2,          /* HIP runtime error (no device, launch failure, ...)          */
    SA_ERR_NOMEM = -3,        /* device or host allocation failed                            */
    SA_ERR_CAPACITY = -4,     /* caller's output buffer (ops) too small                      */
    SA_ERR_UNSUPPORTED = -5   /* input outside what the engine supports (e.g. length >= 2^24) */
};

/* Per-pair result flags (sa_result.flags). */
enum {
    SA_FLAG_DIVERGED = 1,     /* the reference's traceback would never terminate here
                                 (only reachable with scorings whose gap terms are >= 0) */
    SA_FLAG_BAD_SHAPE = 2,    /* device API: pair longer than the max_m/max_n it was given */
    SA_FLAG_SIZE_HACK = 4,    /* LocalGotoh pair replaced by NW (SALocalGotoh.h:484-488)   */
    SA_FLAG_TIMEOUT = 8,      /* internal, never returned: a multi-workgroup (SPLIT) band's
                                 bounded wait for the band above it expired; the same call
                                 re-runs such pairs on the single-workgroup plan         */
    SA_FLAG_RECOVERED = 16,   /* informational: a consistency guard of the band-parallel
                                 traceback fired and the pair was re-walked serially; the
                                 result is exact                                          */
    SA_FLAG_DROPPED = 32      /* sa_*_batch_banded_extend: the X-drop rule stopped the pair's
                                 sweep before the end of its band                         */
};

/* ScoringSystem (include/SequenceAlignment.h:82-131).  Which fields are meaningful depends on
 * the constructor the caller used: linear algorithms read gap/match/mismatch/allow_mismatch,
 * affine algorithms read gap_open/gap_extend/match/mismatch/allow_mismatch.  For the 2-argument
 * form (Gap, Match) the reference sets Mismatch = INT_MIN and AllowMismatch = false. */
typedef struct {
    int32_t gap, match, mismatch, gap_open, gap_extend, allow_mismatch;
} sa_scoring;

/* One pair's result.
 *   score   SW/LocalGotoh: the maximum cell score (the reference's MaxScore);
 *           NW/GlobalGotoh: H[m][n] (M[m][n]).  SW on an empty input: INT32_MIN.
 *   end_i, end_j     SW/LocalGotoh: (MaxRow, MaxCol) — the last row-major cell holding the max;
 *                    NW/GlobalGotoh: (m, n).
 *   start_i, start_j where the traceback stopped (the forceGlobal idx1/idx2 for local modes).
 *   nops    number of ops written for this pair (traceback order, see below).
 * The ops of pair p live at ops + sa_ops_offset(p) where
 *   sa_ops_offset(p) = seq1_off[p] + seq2_off[p] + p   (room for m + n + 1 ops per pair). */
typedef struct {
    int32_t score;
    int32_t end_i, end_j;
    int32_t start_i, start_j;
    uint32_t nops;
    uint32_t flags;
    uint32_t reserved;
} sa_result;

/* Op codes, in traceback order (the order the reference's buildResult push_front()s them):
 *   'M' diagonal, match fn true       -> Entry(Seq1[i-1], Seq2[j-1], true),  i--, j--
 *   'S' diagonal, match fn false      -> Entry(Seq1[i-1], Seq2[j-1], false), i--, j--
 *   'U' up                            -> Entry(Seq1[i-1], Blank, false),     i--
 *   'L' left                          -> Entry(Blank, Seq2[j-1], false),     j--
 *   'X' diagonal, !AllowMismatch, no match -> Entry(Seq1[i-1],Blank) then Entry(Blank,Seq2[j-1])
 *   'u' / 'l' LocalGotoh gap-open whose score is <= 0: the entry of 'U' / 'L' without moving,
 *       then stop (SALocalGotoh.h:395-400 and :451-456). */

typedef struct sa_ctx sa_ctx;

/* Library / device discovery. */
int sa_version(void);
int sa_device_count(int* count);
const char* sa_status_string(int status);

/* Context lifetime.  sa_create binds to `device` (HIP ordinal) and allocates nothing large;
 * the device workspace grows on demand and is kept until sa_destroy / sa_trim. */
int sa_create(int device, sa_ctx** out);
void sa_destroy(sa_ctx* ctx);
const char* sa_last_error(const sa_ctx* ctx);
int sa_set_workspace_limit(sa_ctx* ctx, uint64_t bytes);   /* 0 = automatic (80% of free HBM) */
int sa_trim(sa_ctx* ctx);                                   /* free the cached workspace */

/* Cross-call pipeline of the device API (off by default).  When enabled, consecutive
 * sa_align_batch_device calls overlap: call k's traceback runs on an internal stream while call
 * k+1's fill runs on another, with SA_PIPELINE_DEPTH workspace slots (that many times the HBM).
 * A call is ordered after work
 * already enqueued on the caller's stream, but the caller's stream is NOT ordered after the
 * call's results: wait with sa_wait(ctx) (or a device-wide synchronize) before reading
 * d_results / d_ops, and give any SA_PIPELINE_DEPTH consecutive calls distinct output buffers.
 * Disabling waits for pipelined work.  The host API (sa_align_batch) never pipelines. */
#define SA_PIPELINE_DEPTH 2
int sa_set_pipeline(sa_ctx* ctx, int enable);
int sa_wait(sa_ctx* ctx);

/* Host-buffer batch API (used by the C++ drop-in headers).
 * seq1/seq2: concatenated symbol bytes; seq*_off: npairs+1 offsets (seq*_off[0] = 0).
 * match_lut: NULL for byte equality (the reference's `equal<char>` / nullptr match fn), or a
 *   256x256 table, match_lut[a*256 + b] != 0 iff match(a, b).
 * results: npairs entries.  ops: buffer of ops_cap bytes, pair p's ops at sa_ops_offset(p), so
 *   ops_cap >= seq1_off[npairs] + seq2_off[npairs] + npairs.
 * LocalGotoh pairs of the three sizes in SALocalGotoh.h:484-488 are aligned with NW, as the
 * reference does (flag SA_FLAG_SIZE_HACK).  Blocking; returns when results are on the host. */
int sa_align_batch(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                   const uint8_t* seq1, const uint64_t* seq1_off,
                   const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                   const uint8_t* match_lut, sa_result* results, uint8_t* ops, uint64_t ops_cap);

/* sa_align_batch in `chunks` contiguous pair ranges of near-equal sum of m*n (0: one, or
 * $SEQALIB_HOST_CHUNKS), pipelined on the device (chunk g's traceback beside chunk g+1's fill), and
 * cb(user, pair_begin, pair_end) called on the calling thread as soon as a range's results and op
 * streams are in the caller's buffers -- so a caller can post-process chunk g (the C++ drop-in
 * builds its AlignedSequence lists) while later chunks are still on the GPU.  cb may be NULL.
 * LocalGotoh reports the whole batch once at the end; Hirschberg / Myers-Miller run as one chunk. */
typedef void (*sa_chunk_cb)(void* user, uint32_t pair_begin, uint32_t pair_end);
int sa_align_batch_cb(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                      const uint8_t* seq1, const uint64_t* seq1_off,
                      const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                      const uint8_t* match_lut, sa_result* results, uint8_t* ops, uint64_t ops_cap,
                      uint32_t chunks, sa_chunk_cb cb, void* user);

/* Generic-Ty batch API (any symbol type, any number of distinct symbols: the path the C++
 * drop-in takes when a batch has more than 256 distinct symbols).  Instead of symbols the caller
 * passes each pair's match matrix -- the reference's cacheAllMatches (e.g. SASmithWaterman.h:
 * 20-45) packed to bits: pair p's bitmap starts at word bits_off[p] of `match_bits`, row-major,
 * ceil(n/32) 32-bit words per row, bit (j % 32) of word [i * ceil(n/32) + j / 32] =
 * match(Seq1[i], Seq2[j]).  seq*_off are the npairs+1 length offsets of the sequences (they
 * size the ops as in sa_align_batch); bits_off has npairs+1 entries.  SW, NW, LocalGotoh (with
 * the size hack) and GlobalGotoh; results and ops exactly as sa_align_batch.  Blocking. */
int sa_align_batch_bits(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                        const uint64_t* seq1_off, const uint64_t* seq2_off, uint32_t npairs,
                        const uint32_t* match_bits, const uint64_t* bits_off,
                        sa_result* results, uint8_t* ops, uint64_t ops_cap);

/* Several GPUs of one node behind one handle.  sa_multi_create opens one persistent context per
 * listed device (a device may be listed twice).  sa_multi_align_batch has exactly the contract of
 * sa_align_batch: the batch is cut into contiguous pair ranges of near-equal sum of m*n, one per
 * context, aligned concurrently (one host thread each, no collective), and every range writes its
 * results and op streams in place in the caller's buffers. */
typedef struct sa_multi sa_multi;
int sa_multi_create(const int* devices, int ndevices, sa_multi** out);
void sa_multi_destroy(sa_multi* multi);
const char* sa_multi_last_error(const sa_multi* multi);
int sa_multi_align_batch(sa_multi* multi, int algo, const sa_scoring* scoring,
                         const uint8_t* seq1, const uint64_t* seq1_off,
                         const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                         const uint8_t* match_lut, sa_result* results, uint8_t* ops, uint64_t ops_cap);

/* Device-resident batch API: every pointer is device memory (HBM) and the work is enqueued on
 * `stream` (a hipStream_t; NULL = the context's own stream).  Asynchronous: returns after
 * enqueueing.  max_m/max_n must bound every pair's lengths (pairs that exceed them are skipped
 * with SA_FLAG_BAD_SHAPE).  d_match_lut as in sa_align_batch (device copy) or NULL.
 * d_ops must hold seq1_off[npairs] + seq2_off[npairs] + npairs bytes.
 * No LocalGotoh size hack here: this is the raw kernel path. */
int sa_align_batch_device(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                          const uint8_t* d_seq1, const uint64_t* d_seq1_off,
                          const uint8_t* d_seq2, const uint64_t* d_seq2_off, uint32_t npairs,
                          uint32_t max_m, uint32_t max_n, const uint8_t* d_match_lut,
                          sa_result* d_results, uint8_t* d_ops, void* stream);

/* Score-only batch API: the score and the end cell of every pair, with no traceback.  Each call is
 * its align counterpart (sa_align_batch, sa_align_batch_bits, sa_align_batch_device,
 * sa_multi_align_batch) without the ops buffer: same arguments, argument checks, status codes,
 * chunking and threading rules.  Nothing allocates, packs or downloads an op stream and no
 * traceback kernel is launched.  For every pair it returns the sa_result the align call returns,
 * except that
 *   start_i = start_j = -1, nops = 0, reserved = 0;
 *   SA_FLAG_DIVERGED and SA_FLAG_RECOVERED never appear (they are properties of the walk);
 *   SA_FLAG_BAD_SHAPE (device API) and SA_FLAG_SIZE_HACK (host API: the three LocalGotoh sizes
 *   report the NW score, as sa_align_batch does) appear exactly as in the align call.
 * score, end_i and end_j are bit-exact with the align path: SW / LocalGotoh the last row-major cell
 * holding the maximum (SW on an empty input: INT32_MIN), NW / GlobalGotoh H[m][n] at (m, n).
 * SA_HIRSCHBERG is accepted and means NW (its score is NW's H[m][n]); SA_MYERS_MILLER returns
 * SA_ERR_UNSUPPORTED (its score is defined by its own recursion).
 * Batches on the int32 kernels (LUT match functions, more than 4 distinct symbols, bitmaps,
 * !AllowMismatch, scorings beyond 16 bits) run a fill that stores nothing for a traceback
 * (SA_RECORDS_NONE): a pair's workspace is then its row buffer, O(n), so far more pairs fit one
 * launch and a pair whose records would exceed sa_set_workspace_limit still scores.  DNA batches
 * keep the T16 / score-only fills and their end-cell replay, and only skip the walks.
 * The device call works with sa_set_pipeline, interleaved with pipelined align calls.  After a
 * score call sa_last_timings reports traceback_ms = 0. */
int sa_score_batch(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                   const uint8_t* seq1, const uint64_t* seq1_off,
                   const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                   const uint8_t* match_lut, sa_result* results);
int sa_score_batch_bits(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                        const uint64_t* seq1_off, const uint64_t* seq2_off, uint32_t npairs,
                        const uint32_t* match_bits, const uint64_t* bits_off, sa_result* results);
int sa_score_batch_device(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                          const uint8_t* d_seq1, const uint64_t* d_seq1_off,
                          const uint8_t* d_seq2, const uint64_t* d_seq2_off, uint32_t npairs,
                          uint32_t max_m, uint32_t max_n, const uint8_t* d_match_lut,
                          sa_result* d_results, void* stream);
int sa_multi_score_batch(sa_multi* multi, int algo, const sa_scoring* scoring,
                         const uint8_t* seq1, const uint64_t* seq1_off,
                         const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                         const uint8_t* match_lut, sa_result* results);

/* Banded NW / SW: only the cells within `band` diagonals of the corner-to-corner corridor are
 * computed, so a pair costs O((m + n) * B) cells and record bytes instead of O(m * n).
 * For a pair of lengths m, n and half-width w = band, cell (i, j) (0 <= i <= m, 0 <= j <= n) is in
 * the band when lo <= j - i <= hi with lo = min(0, n - m) - w, hi = max(0, n - m) + w, i.e.
 * B = |n - m| + 2w + 1 diagonals; the band is per pair and always holds (0, 0) and (m, n).
 * The recurrences, borders, tie rules, traceback order and op codes are those of sa_align_batch's
 * SA_NW / SA_SW restricted to in-band cells: a candidate that would read a cell outside the band is
 * no candidate (it never wins the maximum and never compares equal in the walk); in-band border
 * cells keep i * gap / j * gap (NW) or 0 (SW); the SW end cell is the last in-band cell in row-major
 * order holding the maximum.  With band >= max(m, n) the band is the whole matrix and every result
 * field and op equals sa_align_batch's; for any band the score is <= the unbanded score.
 * Arguments, argument checks, status codes, the blocking host-buffer contract, sa_ops_offset and the
 * splitting into launches under sa_set_workspace_limit are sa_align_batch's / sa_score_batch's
 * (score call: start = (-1, -1), nops = 0, reserved = 0, flags = 0, no walk, no records).
 *   algo: SA_SW, SA_NW, or SA_HIRSCHBERG (= SA_NW); the affine algorithms: SA_ERR_UNSUPPORTED.
 *   scoring: gap, match, mismatch, allow_mismatch.  allow_mismatch == 0 needs band >= 1
 *     (band == 0: SA_ERR_UNSUPPORTED, a one-diagonal band has no other candidate).
 *   band >= 2^31 (B overflows 32 bits): SA_ERR_ARG.
 *   (These algorithm, scoring and band checks are made before the context is looked at, so they
 *   give the same status with a NULL context; a NULL context with valid arguments: SA_ERR_ARG.)
 *   SA_ERR_UNSUPPORTED also for a pair with
 *     (m + n + 1) * max(|gap|, |match|, |mismatch|) >= 2^29 (mismatch counted only when allowed),
 *     more than 4096 band diagonals inside its matrix (min(hi, n) - max(lo, -m) + 1: the band of a
 *       pair lives in the registers of one wave),
 *     SW: (m + 1) * that number of diagonals >= 2^31.
 * sa_last_timings works after either call; sa_last_plan_ex reports SA_KERNEL_BANDED, the cells per
 * lane and step of the widest variant the call used, 1 wave, and SA_RECORDS_BAND2 / SA_RECORDS_NONE.
 * The small-call kernel is never used, whatever SEQALIB_TINY says. */
int sa_align_batch_banded(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                          const uint8_t* seq1, const uint64_t* seq1_off,
                          const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                          const uint8_t* match_lut, uint32_t band,
                          sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_banded(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                          const uint8_t* seq1, const uint64_t* seq1_off,
                          const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                          const uint8_t* match_lut, uint32_t band, sa_result* results);
/* Plan of the banded path for a pair of max_m x max_n (host-only query, no device needed): cells per
 * lane and step R, pairs per wave (4, 2 or 1), and the device workspace such a pair occupies in an
 * align call's launch: its 2-bit records, (m + n + 2 - max(lo, -m)) * 2 R L / 8 bytes rounded up to
 * L words, where 2 R L < 2 B is the variant's capacity in diagonals (at least 32) -- O((m + n) * B).
 * This is what the pair needs: a workspace limit of this size is enough for it.  A call that joins
 * two under-filled launches of neighbouring variants may let the pair occupy up to twice as much,
 * and only while the limit leaves room for that.  A score call's pair occupies none.  Status codes as the calls' (SA_ERR_UNSUPPORTED: the shape is
 * outside the limits above). */
int sa_banded_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t band, uint32_t npairs,
                         int* cells_per_lane, int* pairs_per_wave, uint64_t* workspace_bytes_per_pair);

/* Banded LocalGotoh / GlobalGotoh (affine gaps): the band, the cost and the calling contract of
 * sa_align_batch_banded / sa_score_batch_banded, for SA_LOCAL_GOTOH and SA_GLOBAL_GOTOH.
 * Band.  As above: lo = min(0, n - m) - w, hi = max(0, n - m) + w, clipped to the matrix; cell (i, j)
 *   exists iff lo <= j - i <= hi.
 * Recurrence.  That of the raw (unhacked) Gotoh path of sa_align_batch, three values per cell:
 *     X(i, j) = max(M(i-1, j) + gap_open + gap_extend, X(i-1, j) + gap_extend)      (vertical gap)
 *     Y(i, j) = max(M(i, j-1) + gap_open + gap_extend, Y(i, j-1) + gap_extend)      (horizontal gap)
 *     M(i, j) = max(M(i-1, j-1) + match / mismatch, X(i, j), Y(i, j) [, 0 for LocalGotoh])
 *   Borders: M(i, 0) = M(0, j) = 0 for LocalGotoh; gap_open + k * gap_extend for GlobalGotoh with
 *   M(0, 0) = 0; X = Y = -10000 on every border cell (the reference's constant).
 *   A term that would read a cell outside the band is no candidate: X(i, j) does not exist when
 *   (i-1, j) is outside the band, Y(i, j) does not exist when (i, j-1) is; a non-existent X or Y takes
 *   no part in M's maximum and never compares equal in the walk; if (i-1, j) exists but its X does
 *   not, X(i, j) is the open term alone (Y likewise).
 * Walk.  The reference's state machine (type 0 in M, 1 in a vertical gap, 2 in a horizontal one):
 *   in type 0 the diagonal is tried first, then M == X (to type 1), then M == Y (to type 2); in type
 *   1 / 2 the extend term is tried before the open term (which returns to type 0); a comparison
 *   against a non-existent value is false.  GlobalGotoh borders: j == 0 gives 'U', i == 0 gives 'L'.
 *   Op codes and traceback order as in sa_align_batch.  With gap_extend <= 0 the walk always finds an
 *   equal candidate and, for LocalGotoh, never emits 'u' / 'l'.
 * LocalGotoh end cell: the last in-band cell in row-major order holding the maximum; score = M
 *   there.  An empty input gives what the raw unbanded path gives: score 0, end (0, 0), no ops.
 * The LocalGotoh size hack is never applied (as in the matrix and device calls): SA_FLAG_SIZE_HACK
 *   never appears, flags = 0.
 * Score call: start = (-1, -1), nops = 0, reserved = 0, flags = 0; no records, no walk.
 * With band >= max(m, n) every result field and op equals the unbanded raw Gotoh result; for any
 *   band the score is <= the unbanded score.
 * Status codes (these checks are made before the context is looked at, so they give the same status
 * with a NULL context; a NULL context with valid arguments: SA_ERR_ARG):
 *   algo: SA_ERR_UNSUPPORTED for the four other algorithms, SA_ERR_ARG for an invalid value.
 *   gap_extend > 0: SA_ERR_UNSUPPORTED (gap_open may have any sign).
 *   allow_mismatch == 0 with band == 0: SA_ERR_UNSUPPORTED.     band >= 2^31: SA_ERR_ARG.
 *   SA_ERR_UNSUPPORTED also for a pair with
 *     (m + n + 1) * max(|gap_open| + |gap_extend|, |match|, |mismatch|) + 10000 >= 2^29 (mismatch
 *       counted only when allowed),
 *     a sequence of >= 2^24 symbols,
 *     more than 2048 band diagonals inside its matrix (min(hi, n) - max(lo, -m) + 1: three values per
 *       cell fit the registers of one wave up to 16 cells per lane and step),
 *     LocalGotoh: (m + 1) * that number of diagonals >= 2^31.
 * sa_last_timings works after either call; sa_last_plan_ex reports SA_KERNEL_BANDED, the cells per
 * lane and step of the widest variant the call used, 1 wave, and SA_RECORDS_BAND4 / SA_RECORDS_NONE. */
int sa_align_batch_banded_affine(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const uint8_t* match_lut, uint32_t band,
                                 sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_banded_affine(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const uint8_t* match_lut, uint32_t band, sa_result* results);
/* sa_banded_plan_query for the affine calls: cells per lane and step R (1 .. 16), pairs per wave, and
 * the pair's 4-bit records in an align call's launch, (m + n + 2 - max(lo, -m)) * 2 R L / 4 bytes
 * rounded up to L words -- twice the linear call's for the same shape.  SA_ERR_UNSUPPORTED beyond
 * 2048 diagonals inside the matrix and outside the other limits above. */
int sa_banded_affine_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t band, uint32_t npairs,
                                int* cells_per_lane, int* pairs_per_wave, uint64_t* workspace_bytes_per_pair);

/* Substitution-matrix scoring: the diagonal move of cell (i, j) scores submat[a * 256 + b], a = Seq1
 * symbol i-1, b = Seq2 symbol j-1, instead of one of the two numbers match / mismatch.
 *   submat: a dense 256 x 256 int16 table on the host; it need not be symmetric, and only the entries
 *     of symbols that occur in the batch are read.
 *   algo: SA_SW, SA_NW, SA_LOCAL_GOTOH, SA_GLOBAL_GOTOH; SA_HIRSCHBERG and SA_MYERS_MILLER return
 *     SA_ERR_UNSUPPORTED.
 * Recurrences, borders, tie order, the end-cell rule, traceback order and op codes are sa_align_batch's
 * with allow_mismatch = 1, the term (match(a, b) ? match : mismatch) replaced by submat[a][b].
 * scoring->match, mismatch and allow_mismatch are ignored; gap (linear) or gap_open / gap_extend
 * (affine) are read as in sa_align_batch.  A diagonal op is 'M' when match_lut says the two symbols
 * match (NULL: byte equality), else 'S'; 'X' never appears.  match_lut labels ops only: it changes
 * no score.
 * This is the raw path, like the device API: the LocalGotoh size hack is not applied, so
 * SA_FLAG_SIZE_HACK never appears; SA_FLAG_DIVERGED keeps its meaning.
 * The score call follows the score contract above: start = (-1, -1), nops = 0, reserved = 0, no walk,
 * SA_RECORDS_NONE, traceback_ms == 0.
 * Arguments, the blocking host-buffer contract, sa_ops_offset and the splitting into launches under
 * sa_set_workspace_limit are sa_align_batch's / sa_score_batch's.  NULL submat, or any other bad
 * argument: SA_ERR_ARG.  SA_ERR_UNSUPPORTED, with a message, for
 *   more than 64 distinct symbols in the batch, both sequence sets counted together;
 *   a pair with (m + n + 1) * max(|gap terms|, max |S|) >= 2^29, where the gap terms are gap (linear)
 *     or gap_open and gap_extend (affine) and max |S| runs over the symbol pairs of the batch;
 *   a sequence of 2^24 symbols or more.
 *   (These checks are made before the context is looked at, so they give the same status with a NULL
 *   context; a NULL context with valid arguments: SA_ERR_ARG.)
 * sa_last_timings works after either call; sa_last_plan_ex reports SA_KERNEL_INT32 with the plan of
 * a LUT batch of the same shape and SA_RECORDS_FLAGS / SA_RECORDS_NONE.  The T16, score-only and
 * small-call kernels are never used, and every walk is the one-lane-per-pair kernel, whatever
 * SEQALIB_T16, SEQALIB_TINY or SEQALIB_TB say. */
int sa_align_batch_matrix(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                          const uint8_t* seq1, const uint64_t* seq1_off,
                          const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                          const int16_t* submat, const uint8_t* match_lut,
                          sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_matrix(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                          const uint8_t* seq1, const uint64_t* seq1_off,
                          const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                          const int16_t* submat, const uint8_t* match_lut, sa_result* results);
/* Plan of sa_align_batch_matrix for a batch of npairs pairs up to max_m x max_n with nsym distinct
 * symbols (host-only query, no device needed): always SA_KERNEL_INT32, with the rows per lane, waves
 * (0: one single-wave workgroup per band) and per-pair workspace sa_plan_query_ex reports for a batch
 * that runs the int32 kernel alone (a forced plan of 16 rows per lane runs at most 8 waves).  The
 * scoring's match / mismatch are not read.  nsym > 64 and lengths >= 2^24: SA_ERR_UNSUPPORTED. */
int sa_matrix_plan_query(int algo, const sa_scoring* scoring, uint32_t max_m, uint32_t max_n,
                         uint32_t npairs, int nsym, int* kernel, int* rows_per_lane, int* waves,
                         uint64_t* workspace_bytes_per_pair);

/* Banded substitution-matrix scoring: the band of sa_align_batch_banded (SA_SW, SA_NW: 2-bit records,
 * up to 4096 band diagonals inside the matrix) or of sa_align_batch_banded_affine (SA_LOCAL_GOTOH,
 * SA_GLOBAL_GOTOH: 4-bit records, up to 2048) with the diagonal term of sa_align_batch_matrix.
 * Band geometry, the rule that a term which would read a cell outside the band is no candidate,
 * borders, tie order, the end-cell rule, traceback order and op codes are those banded calls'; the
 * only change is the diagonal term, (match(a, b) ? match : mismatch) replaced by submat[a * 256 + b].
 * scoring->match, mismatch and allow_mismatch are ignored: mismatches are always allowed, so band == 0
 * is valid for every scoring and 'X' never appears.  gap (linear) or gap_open / gap_extend (affine) are
 * read.  A diagonal op is 'M' when match_lut says the two symbols match (NULL: byte equality), else
 * 'S'; match_lut labels ops only, it changes no score.
 * This is the raw path: the LocalGotoh size hack is never applied and flags = 0.
 * Score call: start = (-1, -1), nops = 0, reserved = 0, flags = 0; no records, no walk,
 * traceback_ms == 0.
 * With band >= max(m, n) every result field and op equals sa_align_batch_matrix's, for scorings where
 * that call sets no flag; for any band the score is <= the unbanded matrix score.  Empty inputs give
 * what the banded calls without a table give.
 * Status codes (these checks are made before the context is looked at, so they give the same status
 * with a NULL context; a NULL context with valid arguments: SA_ERR_ARG):
 *   NULL scoring, NULL submat, an invalid algo, band >= 2^31, bad offsets or buffers: SA_ERR_ARG.
 *   SA_HIRSCHBERG, SA_MYERS_MILLER: SA_ERR_UNSUPPORTED, as in the matrix calls.
 *   An affine algo with gap_extend > 0: SA_ERR_UNSUPPORTED (gap_open may have any sign).
 *   More than 64 distinct symbols in the batch, both sequence sets together: SA_ERR_UNSUPPORTED.
 *   SA_ERR_UNSUPPORTED also for a pair with
 *     a sequence of >= 2^24 symbols,
 *     linear: (m + n + 1) * max(|gap|, max |S|) >= 2^29,
 *     affine: (m + n + 1) * max(|gap_open| + |gap_extend|, max |S|) + 10000 >= 2^29 (the banded affine
 *       calls' bound, stricter than sa_align_batch_matrix's),
 *     more than 4096 (linear) or 2048 (affine) band diagonals inside its matrix,
 *     SA_SW / SA_LOCAL_GOTOH: (m + 1) * that number of diagonals >= 2^31,
 *   where max |S| runs over the symbol pairs of the batch.
 *   ops_cap too small: SA_ERR_CAPACITY.  One pair's records above the workspace limit: SA_ERR_NOMEM.
 * There is no plan query of its own: a pair's variant and workspace are what sa_banded_plan_query
 * (SA_SW, SA_NW) or sa_banded_affine_plan_query (SA_LOCAL_GOTOH, SA_GLOBAL_GOTOH) report for the same
 * shape and band.  sa_last_timings works after either call; sa_last_plan_ex reports SA_KERNEL_BANDED,
 * the cells per lane and step of the widest variant the call used, 1 wave, and SA_RECORDS_BAND2 /
 * SA_RECORDS_BAND4 / SA_RECORDS_NONE. */
int sa_align_batch_banded_matrix(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const int16_t* submat, const uint8_t* match_lut, uint32_t band,
                                 sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_banded_matrix(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const int16_t* submat, const uint8_t* match_lut, uint32_t band,
                                 sa_result* results);

/* Ends-free (semi-global) banded alignment: banded NW / banded GlobalGotoh in which the unaligned head
 * or tail of a sequence may cost nothing -- a read inside a reference window (fit: SA_FREE_SEQ2_BEGIN |
 * SA_FREE_SEQ2_END with the read as Seq1), two overlapping reads (overlap: SA_FREE_SEQ1_BEGIN |
 * SA_FREE_SEQ2_END, a suffix of Seq1 against a prefix of Seq2, or the mirrored pair of flags), a primer
 * against a read end (prefix / suffix: one END or one BEGIN flag). */
#define SA_FREE_SEQ1_BEGIN 1   /* leading Seq1 symbols may stay unaligned at no cost  */
#define SA_FREE_SEQ1_END   2   /* trailing Seq1 symbols may stay unaligned at no cost */
#define SA_FREE_SEQ2_BEGIN 4   /* leading Seq2 symbols ...                            */
#define SA_FREE_SEQ2_END   8   /* trailing Seq2 symbols ...                           */
/* Band, recurrence, the rule that a term which would read a cell outside the band is no candidate, tie
 * order, records, traceback order and op codes are those of sa_align_batch_banded with SA_NW
 * (algo SA_NW, or SA_HIRSCHBERG meaning NW: 2-bit records, up to 4096 band diagonals inside the matrix)
 * or of sa_align_batch_banded_affine with SA_GLOBAL_GOTOH (4-bit records, up to 2048), with exactly
 * these changes, free_ends being any OR of the four flags:
 * Borders.  With SA_FREE_SEQ1_BEGIN the in-band cells (i, 0) hold H = 0 (GlobalGotoh: M = 0); without it
 *   i * gap (gap_open + i * gap_extend).  SA_FREE_SEQ2_BEGIN does the same for (0, j).  (0, 0) is 0.
 *   GlobalGotoh's X = Y = -10000 on every border cell, as in the affine call.
 * End cell.  The candidates are these in-band cells, border cells included: (m, n); with
 *   SA_FREE_SEQ1_END every (i, n); with SA_FREE_SEQ2_END every (m, j).  The end cell is the last
 *   candidate in row-major order that holds the maximum of H (M) over the candidates, so (m, n) wins
 *   ties; score is that value, (end_i, end_j) that cell.  A negative score is a score like any other.
 * Walk.  From the end cell (GlobalGotoh: in type 0), with the banded call's candidate order / state
 *   machine; the symbols after the end cell produce no op.  At j == 0: stop with SA_FREE_SEQ1_BEGIN, else
 *   'U' down to (0, 0).  At i == 0: stop with SA_FREE_SEQ2_BEGIN, else 'L'.  (start_i, start_j) is where
 *   the walk stopped; flags = 0.
 * free_ends == 0: every result field and every op equals sa_align_batch_banded's (SA_NW) /
 *   sa_align_batch_banded_affine's (SA_GLOBAL_GOTOH).
 * Score call: start = (-1, -1), nops = 0, reserved = 0, flags = 0; no records, no walk,
 *   traceback_ms == 0; score and end cell as the align call's.
 * The band is unchanged: lo = min(0, n - m) - w, hi = max(0, n - m) + w.  It holds every start diagonal
 *   a Seq1 of length m can have inside a Seq2 of length n (and the reverse) plus w of slack, so w bounds
 *   how far outside the corner-to-corner corridor a free start or end may lie: an overlap of two
 *   equal-length reads can leave at most w symbols of each free.
 * Status codes (all these checks are made before the context is looked at, so they give the same status
 * with a NULL context; a NULL context with valid arguments: SA_ERR_ARG):
 *   algo: SA_SW, SA_LOCAL_GOTOH, SA_MYERS_MILLER: SA_ERR_UNSUPPORTED; an invalid value: SA_ERR_ARG.
 *   free_ends > 15: SA_ERR_ARG.
 *   Every other argument check, pair limit and status code of sa_align_batch_banded with SA_NW /
 *   sa_align_batch_banded_affine with SA_GLOBAL_GOTOH, unchanged: band >= 2^31 SA_ERR_ARG;
 *   allow_mismatch == 0 with band == 0, gap_extend > 0 (GlobalGotoh), the 2^29 score bounds, a sequence
 *   of >= 2^24 symbols, more than 4096 / 2048 band diagonals inside the matrix: SA_ERR_UNSUPPORTED.
 *   There is no (m + 1) * diagonals < 2^31 limit: the end-cell search orders its at most m + n + 1
 *   candidates by position along the last column and then the last row.
 * Records, workspace, launch splitting under sa_set_workspace_limit and the joining of neighbouring
 * variants are the banded calls'.  There is no plan query of its own: sa_banded_plan_query (SA_NW) /
 * sa_banded_affine_plan_query (SA_GLOBAL_GOTOH) describe these calls too.  sa_last_timings works after
 * either call; sa_last_plan_ex reports SA_KERNEL_BANDED, the cells per lane and step of the widest
 * variant the call used, 1 wave, and SA_RECORDS_BAND2 / SA_RECORDS_BAND4 / SA_RECORDS_NONE. */
int sa_align_batch_banded_ends_free(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                    const uint8_t* seq1, const uint64_t* seq1_off,
                                    const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                    const uint8_t* match_lut, uint32_t band, uint32_t free_ends,
                                    sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_banded_ends_free(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                    const uint8_t* seq1, const uint64_t* seq1_off,
                                    const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                    const uint8_t* match_lut, uint32_t band, uint32_t free_ends,
                                    sa_result* results);

/* Seeded ends-free banded alignment: the ends-free calls above with every pair's band placed round a
 * seed diagonal instead of the corner-to-corner corridor.  diag[p] = k_p is the seed diagonal of pair p
 * (k = j - i: a read, Seq1, that starts at position s of its window, Seq2, lies on k = s); band = w is
 * the same for every pair.
 * Band.  lo = k_p - w, hi = k_p + w, clipped to the matrix as everywhere: lo' = max(lo, -m),
 *   hi' = min(hi, n), B' = hi' - lo' + 1 <= 2w + 1 diagonals.  The window length does not enter the
 *   band's width, so a short read can go against a whole contig (n < 2^24) and two long reads that
 *   overlap by little need no wide band.
 * Algorithms.  SA_NW (SA_HIRSCHBERG means NW): 2-bit records, B' <= 4096.  SA_GLOBAL_GOTOH: 4-bit
 *   records, B' <= 2048.
 * Semantics.  Exactly those of sa_align_batch_banded_ends_free with this band in place of its band:
 *   the borders, "a term that would read a cell outside the band is no candidate", the end-cell rule
 *   (the last candidate in row-major order holding the maximum), the walk with its stop rules, tie order
 *   and op codes, and the score contract for the score call.  (0, 0) and (m, n) need not be in the band,
 *   which changes two things:
 *   A legal begin must exist in the band: lo' <= 0 <= hi' (the cell (0, 0)), or SA_FREE_SEQ2_BEGIN and
 *     hi' >= 0 (a row-0 cell), or SA_FREE_SEQ1_BEGIN and lo' <= 0 (a column-0 cell).
 *   A legal end must exist in the band: lo' <= n - m <= hi' (the cell (m, n)), or SA_FREE_SEQ2_END and
 *     lo' <= n - m (a last-row cell), or SA_FREE_SEQ1_END and hi' >= n - m (a last-column cell).
 *   A pair that lacks either answers SA_ERR_UNSUPPORTED with a message naming the pair and the missing
 *   end.  Under this rule a border cell whose begin is not free is in the band only when (0, 0) is, so
 *   "in-band border cells keep k * gap" is exactly the DP restricted to the band; (m, n) is a candidate
 *   only when it is in the band.
 * Equivalences.
 *   (a) With w >= m + n every result field and op equals sa_align_batch_banded_ends_free's with a
 *       whole-matrix band.
 *   (b) When n - m is even, diag = (n - m) / 2 and w' = w + |n - m| / 2: the call at w' equals the
 *       ends-free call at w in every field and op (n == m: diag = 0 and the same w).
 *   (c) For a fixed diag the score does not fall as w grows.
 * Status codes (all checked before the context is looked at, so a NULL context gives the same answer;
 * a NULL context with valid arguments: SA_ERR_ARG):
 *   diag NULL with npairs > 0; diag[p] outside [-m_p, n_p] (the seed diagonal does not cross the matrix;
 *   the message names the pair); free_ends > 15; an invalid algo; band >= 2^31: SA_ERR_ARG.
 *   SA_SW, SA_LOCAL_GOTOH, SA_MYERS_MILLER: SA_ERR_UNSUPPORTED.
 *   Everything else as the ends-free calls: the 2^29 score bound per pair, m, n < 2^24, gap_extend <= 0
 *   for GlobalGotoh, band == 0 needs allow_mismatch, B' above 4096 / 2048: SA_ERR_UNSUPPORTED;
 *   SA_ERR_CAPACITY; SA_ERR_NOMEM.
 * Records (align call): tend - tb + 1 steps per pair with
 *   tb = (max(-lo', 0) + max(-hi', 0)) & ~1 and tend = min(m + n, 2m + hi', 2n - lo') - lo',
 *   about 2 min(m, n) + 2w steps whatever the longer sequence's length.  Launch splitting under
 *   sa_set_workspace_limit, the joining of neighbouring variants ($SEQALIB_BAND_MERGE), sa_last_timings
 *   and sa_last_plan_ex (SA_KERNEL_BANDED, the widest variant's cells per lane, 1 wave,
 *   SA_RECORDS_BAND2 / BAND4 / NONE) work as for the banded calls.
 * sa_banded_seeded_plan_query (host-only): variant, pairs per wave and record bytes of one shape, or the
 *   status the calls give it (SA_ERR_UNSUPPORTED for an illegal band).  sa_banded_plan_query and
 *   sa_banded_affine_plan_query describe the corridor band and do not apply. */
int sa_align_batch_banded_seeded(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const uint8_t* match_lut, const int32_t* diag, uint32_t band, uint32_t free_ends,
                                 sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_banded_seeded(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const uint8_t* match_lut, const int32_t* diag, uint32_t band, uint32_t free_ends,
                                 sa_result* results);
int sa_banded_seeded_plan_query(int algo, uint64_t m, uint64_t n, int32_t diag, uint32_t band, uint32_t free_ends,
                                int* cells_per_lane, int* pairs_per_wave, uint64_t* ws_bytes_per_pair);

/* Device-resident seeded banded calls: the seeded calls above over two buffers that already lie on the device
 * -- a mapper's reads and its reference -- so that no window is copied per call.  Every d_ pointer is device
 * memory.  Pair p is Seq1 = d_seq1[d_start1[p] .. + d_len1[p]) and Seq2 = d_seq2[d_start2[p] .. + d_len2[p]) with
 * seed diagonal d_diag[p]; slices may overlap and come in any order.  Its ops (traceback order, nops bytes) go to
 * d_ops + d_ops_off[p], a region that needs room for len1 + len2 + 1 bytes; regions may come in any order and
 * must not overlap.  max_m / max_n bound the lengths, as in sa_align_batch_device.
 *
 * Semantics: for every pair that is run, every field of its sa_result and every op equals what
 * sa_align_batch_banded_seeded / sa_score_batch_banded_seeded returns for the two slices with the same diag,
 * band, free_ends, scoring and match table (d_match_lut: a device copy of the 256 x 256 table, or NULL).  The
 * score call keeps the score contract (start (-1, -1), nops 0).  SA_NW, SA_HIRSCHBERG (= SA_NW) and
 * SA_GLOBAL_GOTOH.  A pair's fill variant is the narrowest its clipped band fits; the device form never merges
 * variants (the host call does, unless SEQALIB_BAND_MERGE=0; results do not depend on it).
 *
 * Ordering: asynchronous, as sa_align_batch_device.  The call is ordered after the work already on `stream`
 * (NULL: the context's stream) and after the context's previous call; it plans, fills and walks on that stream
 * and returns after enqueueing, without a stream synchronisation, a device-to-host copy or a host read of any
 * length (the context's workspace grows on first use, which drains the context as in every call).
 * sa_set_pipeline does not change it.  npairs == 0: SA_OK, nothing enqueued.
 *
 * Host-side status (made before the context is looked at, so the same with a NULL context; a NULL context with
 * valid arguments: SA_ERR_ARG): algorithm class, free_ends > 15, band >= 2^31, NULL scoring, gap_extend > 0,
 * band == 0 without allow_mismatch: as the host seeded calls.  With npairs > 0 a NULL d_start*, d_len*, d_diag,
 * d_results (align: d_ops, d_ops_off) or a NULL d_seq* with seq*_bytes > 0: SA_ERR_ARG.  From the bound shape
 * alone -- stricter than the host calls, which judge every pair by its own clipped band -- SA_ERR_UNSUPPORTED for
 * max_m or max_n >= 2^24; (max_m + max_n + 1) * max(|gap|, |match|, |mismatch|) >= 2^29 (GlobalGotoh:
 * |gap_open| + |gap_extend| for |gap|, + 10000); min(2 * band + 1, max_m + max_n + 1) above 4096 (NW) or 2048
 * (GlobalGotoh).  One pair's provision above the workspace limit: SA_ERR_NOMEM.
 *
 * Device-side refusals: a refused pair gets an all-zero sa_result with one flag; it writes no op and neither its
 * slices nor its ops region are touched.  SA_FLAG_BAD_SHAPE, checked first: len1 > max_m, len2 > max_n,
 * start + len beyond seq*_bytes, (align) ops_off + len1 + len2 + 1 beyond ops_bytes.  SA_FLAG_BAD_BAND: diag
 * outside [-len1, len2], or the band holds no legal begin or no legal end (the rule of the seeded calls above).
 *
 * Workspace: the pairs are run in chunks, contiguous pair ranges one after another on the stream; a chunk's
 * provision is its pairs x (record_bytes_per_pair + plan_bytes_per_pair) plus 8,704 bytes (a fixed head and
 * alignment), a score call's the plan bytes only.  record_bytes_per_pair is a bound over every pair inside max_m x max_n at any
 * diagonal: the records of the variant of min(2 * band + 1, max_m + max_n + 1) diagonals over
 * min(max_m + max_n, 2 max_m + 2 band, 2 max_n + 2 band) + 2 steps.  sa_banded_seeded_device_plan_query
 * (host-only) returns both and the cells per lane of that variant.
 *
 * sa_last_timings: fill_ms is the planner kernels plus the fills, traceback_ms the walks, launches the chunks.
 * sa_last_plan_ex: SA_KERNEL_BANDED, the cells per lane of the widest variant a pair inside the bounds can take,
 * 1 wave, SA_RECORDS_BAND2 / BAND4 / NONE. */
#define SA_FLAG_BAD_BAND 64   /* device seeded calls: diag outside [-m, n], or the band holds no legal begin / end */
int sa_align_batch_banded_seeded_device(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                        const uint8_t* d_seq1, uint64_t seq1_bytes, const uint64_t* d_start1, const uint32_t* d_len1,
                                        const uint8_t* d_seq2, uint64_t seq2_bytes, const uint64_t* d_start2, const uint32_t* d_len2,
                                        uint32_t npairs, uint32_t max_m, uint32_t max_n, const uint8_t* d_match_lut,
                                        const int32_t* d_diag, uint32_t band, uint32_t free_ends,
                                        sa_result* d_results, uint8_t* d_ops, const uint64_t* d_ops_off, uint64_t ops_bytes,
                                        void* stream);
int sa_score_batch_banded_seeded_device(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                        const uint8_t* d_seq1, uint64_t seq1_bytes, const uint64_t* d_start1, const uint32_t* d_len1,
                                        const uint8_t* d_seq2, uint64_t seq2_bytes, const uint64_t* d_start2, const uint32_t* d_len2,
                                        uint32_t npairs, uint32_t max_m, uint32_t max_n, const uint8_t* d_match_lut,
                                        const int32_t* d_diag, uint32_t band, uint32_t free_ends,
                                        sa_result* d_results, void* stream);
int sa_banded_seeded_device_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t band,
                                       int* widest_cells_per_lane, uint64_t* record_bytes_per_pair, uint64_t* plan_bytes_per_pair);

/* Banded X-drop extension: the alignment mode of a seed-and-extend mapper.  The alignment is anchored at
 * (0, 0), may end at any cell, and a pair's sweep is abandoned once its score has fallen too far below
 * its best.  A caller extends to the right of a seed by passing the two suffixes after the seed, and to
 * the left by passing the two reversed prefixes.  band = w and xdrop are the same for every pair.
 * Algorithms.  SA_NW (SA_HIRSCHBERG means NW): 2-bit records, B' <= 4096.  SA_GLOBAL_GOTOH: 4-bit
 *   records, B' <= 2048.  SA_SW, SA_LOCAL_GOTOH, SA_MYERS_MILLER: SA_ERR_UNSUPPORTED; an invalid value:
 *   SA_ERR_ARG.
 * Band.  That of the seeded calls round diagonal 0: lo' = max(-w, -m), hi' = min(w, n), B' = hi' - lo' + 1
 *   <= 2w + 1: w diagonals either side of diagonal 0.  The anchor (0, 0) is always inside it, (m, n) need
 *   not be; there is no legality rule and no diag argument.
 * Recurrence, borders, tie order, records and op codes.  Those of sa_align_batch_banded_seeded with
 *   free_ends = 0: borders k * gap (NW), gap_open + k * gap_extend with X = Y = -10000 (GlobalGotoh); a
 *   term that would read a cell outside the band is no candidate.
 * End cell.  The candidates are (0, 0), which holds 0, and every in-band interior cell (i >= 1, j >= 1)
 *   the sweep computed; border cells other than (0, 0) are no candidates.  The end cell is the last
 *   candidate in row-major order that holds the maximum of H (GlobalGotoh: M) over the candidates; score
 *   is that value, never negative, and (end_i, end_j) that cell.
 * Drop rule.  Steps are the band's own: an in-band cell (i, j) belongs to step t = i + j - lo'; the last
 *   step is tend = min(m + n, 2m + hi', 2n - lo') - lo'.  A checkpoint follows every step t with
 *   t = SA_XDROP_PERIOD - 1 (mod SA_XDROP_PERIOD) and t < tend.  There, best is the candidates' maximum
 *   over all steps <= t, and recent the maximum of H (M) over the interior in-band cells of the steps
 *   t - SA_XDROP_PERIOD + 1 .. t.  If those steps hold at least one interior cell, xdrop >= 0 and
 *   best - recent > xdrop, the pair stops: it has no cells of later steps, and SA_FLAG_DROPPED is set.
 *   Nothing is pruned before the stop: every cell of a step <= t has exactly the value the unstopped
 *   recurrence gives it.  xdrop = SA_XDROP_OFF never stops; xdrop < -1: SA_ERR_ARG.
 * Walk.  From the end cell (GlobalGotoh: in type 0) to (0, 0) with the banded call's candidate order /
 *   state machine; at j == 0 'U', at i == 0 'L'.  start = (0, 0); flags is 0 or SA_FLAG_DROPPED.  The ops
 *   cover Seq1[0, end_i) and Seq2[0, end_j) only.
 * Score call.  start = (-1, -1), nops = 0, reserved = 0; no records, no walk; score, end cell and
 *   SA_FLAG_DROPPED exactly as the align call's.
 * Equivalences.
 *   (a) For any xdrop, a result with end cell (e_i, e_j) equals sa_align_batch_banded_seeded on the
 *       prefixes Seq1[0, e_i) and Seq2[0, e_j) with diag = 0, the same band and free_ends = 0, in score,
 *       end cell, start, nops and every op: the two prefix bands hold the same cells with the same values.
 *   (b) For fixed inputs the score does not fall as xdrop grows, and equals the SA_XDROP_OFF score from
 *       some xdrop on.
 * Status codes (all checked before the context is looked at, so a NULL context gives the same answer; a
 * NULL context with valid arguments: SA_ERR_ARG):
 *   an invalid algo; band >= 2^31; xdrop < -1: SA_ERR_ARG.
 *   As the seeded calls: band == 0 without allow_mismatch, gap_extend > 0 (GlobalGotoh), the 2^29 score
 *   bound per pair, m or n >= 2^24, B' above 4096 / 2048: SA_ERR_UNSUPPORTED.  (m + 1) * B' >= 2^31:
 *   SA_ERR_UNSUPPORTED, as for banded SW, whose end-cell key this is.  SA_ERR_CAPACITY; SA_ERR_NOMEM.
 * Records (align call): sized for tend - tb + 1 steps per pair as in the seeded call, tb = (-lo') & ~1; a
 *   stopped pair leaves the rest unwritten.  Launch splitting under sa_set_workspace_limit, the joining of
 *   neighbouring variants ($SEQALIB_BAND_MERGE), sa_last_timings and sa_last_plan_ex (SA_KERNEL_BANDED,
 *   the widest variant's cells per lane, 1 wave, SA_RECORDS_BAND2 / BAND4 / NONE) work as for the banded
 *   calls.  The cost of a call depends on its data: a wave leaves the sweep once all its pairs have
 *   stopped or ended.
 * sa_banded_extend_plan_query (host-only): variant, pairs per wave and record bytes of one shape, or the
 *   status the calls give it. */
#define SA_XDROP_OFF (-1)
#define SA_XDROP_PERIOD 16
int sa_align_batch_banded_extend(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const uint8_t* match_lut, uint32_t band, int32_t xdrop,
                                 sa_result* results, uint8_t* ops, uint64_t ops_cap);
int sa_score_batch_banded_extend(sa_ctx* ctx, int algo, const sa_scoring* scoring,
                                 const uint8_t* seq1, const uint64_t* seq1_off,
                                 const uint8_t* seq2, const uint64_t* seq2_off, uint32_t npairs,
                                 const uint8_t* match_lut, uint32_t band, int32_t xdrop,
                                 sa_result* results);
int sa_banded_extend_plan_query(int algo, uint64_t m, uint64_t n, uint32_t band,
                                int* cells_per_lane, int* pairs_per_wave, uint64_t* ws_bytes_per_pair);

/* Device time of the kernels of the last sa_align_batch[_device] call, from HIP events
 * recorded on the stream they ran on: total fill-kernel ms, total traceback-kernel ms, and the
 * number of fill launches.  Waits for those events. */
int sa_last_timings(sa_ctx* ctx, float* fill_ms, float* traceback_ms, int* fill_launches);
// With $SEQALIB_KERNEL_TIMING set during the last call: the fill kernels alone (HIP events around
// each fill launch on its stream) and the whole fill-stream span (fill + end-cell replay, = the
// fill_ms of sa_last_timings).  SA_ERR_ARG when the last call ran without the variable.
int sa_last_kernel_timings(sa_ctx* ctx, float* fill_kernel_ms, float* fill_stream_ms);

/* Fill kernel of the last sa_align_batch[_device] call: SA_KERNEL_INT32 (int32 scores, equality
 * flags; any alphabet, LUT, scoring) or SA_KERNEL_T16 (tagged 16-bit profile kernels: SW/NW and,
 * with the affine cell, LocalGotoh/GlobalGotoh, all with allow-mismatch, <= 4 distinct symbols in
 * the batch, score range checked).  Also R and W.  Environment: SEQALIB_T16=0 forces the int32
 * kernel. */
#define SA_KERNEL_INT32 0
#define SA_KERNEL_T16 1
#define SA_KERNEL_T16_ENDCELL 2   /* T16 SW / LocalGotoh with per-chunk maxima + end-cell replay */
/* Host-buffer calls of at most 64 pairs with m <= 256, n <= 1024, m * n <= 32768 (SW / NW /
 * LocalGotoh / GlobalGotoh): one kernel fills and walks each pair in one wave (int32 cells, flags
 * in LDS), reading and writing pinned host memory.  Such a call reports 0 fill launches to
 * sa_last_timings.  Environment: SEQALIB_TINY=0 sends them through the batch kernels. */
#define SA_KERNEL_TINY 3
#define SA_KERNEL_BANDED 4   /* sa_align_batch_banded / sa_score_batch_banded and their _affine forms */
int sa_last_plan(sa_ctx* ctx, int* kernel, int* rows_per_lane, int* waves);
/* sa_last_plan plus what the fill stored for the traceback: SA_RECORDS_FLAGS (int32 equality
 * flags), SA_RECORDS_TAGS (T16 move tags per cell) or SA_RECORDS_SCORE_ONLY (score-only T16 SW fill:
 * per-chunk snapshots + each lane's last row per step; the traceback recomputes the blocks along
 * its path).  Environment: SEQALIB_SO=0 keeps the tagged records. */
#define SA_RECORDS_FLAGS 0
#define SA_RECORDS_TAGS 1
#define SA_RECORDS_SCORE_ONLY 2
#define SA_RECORDS_NONE 3   /* score calls on the int32 / small-call kernels: the fill stored nothing for a traceback */
#define SA_RECORDS_BAND2 4  /* banded align calls: 2 bits per in-band cell, laid out by anti-diagonal */
#define SA_RECORDS_BAND4 5  /* banded affine align calls: 4 bits per in-band cell */
int sa_last_plan_ex(sa_ctx* ctx, int* kernel, int* rows_per_lane, int* waves, int* records);

/* Plan of the int32 kernel for a batch (host-only query, no device needed): rows per lane R,
 * waves per workgroup W, direction bytes per pair, row-buffer bytes per pair.  The plan the
 * engine actually selects (T16 for DNA) is sa_plan_query_ex's. */
int sa_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t npairs,
                  int* rows_per_lane, int* waves, uint64_t* dir_bytes_per_pair,
                  uint64_t* rowbuf_bytes_per_pair);

/* Plan of a batch for a given scoring (host-only query, no device needed): the kernel the
 * engine selects when the batch holds `nsym` distinct symbols (SA_KERNEL_*; T16 needs nsym <= 4
 * and a scoring whose scores provably fit 16 bits), its R and W (W = 0: the multi-workgroup
 * plan), and the device workspace one pair occupies (direction records + row buffers + end-cell
 * snapshots; the larger of the T16 and int32 variants when the scoring admits T16, since the
 * variant is chosen on the device and both are provisioned).  A pipelined context
 * (sa_set_pipeline) holds SA_PIPELINE_DEPTH such slots per pair of a launch. */
int sa_plan_query_ex(int algo, const sa_scoring* scoring, uint32_t max_m, uint32_t max_n,
                     uint32_t npairs, int nsym, int* kernel, int* rows_per_lane, int* waves,
                     uint64_t* workspace_bytes_per_pair);

/* sa_plan_query_ex for a score call (host-only query, no device needed): the kernel a host score
 * call (sa_score_batch) runs when the batch holds `nsym` distinct symbols, its R and W, and the
 * device workspace one pair occupies.  With nsym > 4, or a scoring that does not admit T16, that is
 * the record-free int32 fill: row buffers only, no direction records.  With nsym <= 4 it is the
 * align call's plan (the T16 / score-only fills keep their edge streams and snapshots for the
 * end-cell replay).  SA_HIRSCHBERG means NW; SA_MYERS_MILLER: SA_ERR_UNSUPPORTED. */
int sa_score_plan_query(int algo, const sa_scoring* scoring, uint32_t max_m, uint32_t max_n,
                        uint32_t npairs, int nsym, int* kernel, int* rows_per_lane, int* waves,
                        uint64_t* workspace_bytes_per_pair);

/* Tests only (tests/test_gpu_robust.py).  SA_HOOK_HAND_TAG: the band-unit hand-off tag of the
 * context's last launch becomes `value` (0..65535; the next launch takes value + 1, and at 65535 the
 * hand-off buffer is zeroed and the tags restart at 1).  SA_HOOK_POISON_WS: every 32-bit word of the
 * context's cached workspace becomes `value` (after its pending work; synchronous), as stale words
 * of earlier calls of other shapes would be.  SA_HOOK_F16: 0 / 1 allows / turns off the f16 cell of
 * the two-pairs-per-wave SW fill for the context (after its pending work); 2 returns 1 when it is
 * off (the context turned it off after a launch flagged more than 1/64 of its pairs), else 0.
 * Returns SA_OK or SA_ERR_ARG (SA_HOOK_F16 with 2: 1 / 0). */
#define SA_HOOK_HAND_TAG 1
#define SA_HOOK_POISON_WS 2
#define SA_HOOK_F16 3
int sa_test_hook(sa_ctx* ctx, int hook, uint64_t value);

/* Synthetic DNA: std::mt19937_64(seed), symbol = "ACGT"[g() & 3]. */
int sa_synth_dna(uint64_t seed, uint32_t len, uint8_t* out);
/* "Related" copy of src: per position r = g() % 100: r < 10 substitute "ACGT"[g()&3];
 * r < 12 insert "ACGT"[g()&3] before it; r < 14 delete it; else copy.  g = mt19937_64(seed).
 * Writes at most cap bytes; *out_len = produced length (may exceed cap -> SA_ERR_CAPACITY). */
int sa_synth_mutate(const uint8_t* src, uint32_t len, uint64_t seed, uint8_t* out, uint32_t cap,
                    uint32_t* out_len);
/* npairs independent pairs: pair p uses seeds base+2p+1 (seq1, len1) and base+2p+2 (seq2, len2);
 * writes concatenated sequences and npairs+1 offsets.  Uses up to `threads` host threads. */
int sa_synth_dna_batch(uint64_t base, uint32_t npairs, uint32_t len1, uint32_t len2,
                       uint8_t* seq1, uint64_t* seq1_off, uint8_t* seq2, uint64_t* seq2_off,
                       int threads);

#ifdef __cplusplus
}
#endif
#endif /* SEQALIB_HIP_H */
