// sa_api_ctx.h — what the host translation units of the C ABI share (sa_api.hip, sa_api_banded.hip): the
// context, error reporting, call ordering, the context's device buffers, and the argument checks and the
// matrix recode that more than one family of calls runs.  Private to seqalib_amd/csrc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "sa_dc.h"
#include "sa_internal.h"

constexpr int kKEv = 6;   // SEQALIB_KERNEL_TIMING events per fill launch (two per variant, <= 3)
// Cross-call pipeline: workspace slots (call k's fill waits for call k-2's traceback).  Three slots
// with the fills alternating between two streams (call k+1's fill starting in call k's fill tail)
// measured slower, 19.5 vs 18.2 ms per headline step (round 5, profiles/pipe_slots_ab_r05.txt).
constexpr int kPipeSlots = SA_PIPELINE_DEPTH;

struct sa_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // cached device workspace (direction slots + row buffers + LUT bits)
    uint8_t* ws = nullptr;
    uint64_t ws_bytes = 0;
    uint64_t ws_limit = 0;  // 0 = automatic
    // cached device I/O buffers for the host API
    uint8_t* io = nullptr;
    uint64_t io_bytes = 0;
    // timing of the last call
    std::vector<hipEvent_t> events;  // 3 per fill launch: start, fill end, traceback end
    int launches = 0;
    // $SEQALIB_KERNEL_TIMING: per launch and variant, events around the fill kernel alone
    // (kKEv per launch: [2k] before, [2k + 1] after variant k's fill; kvars[launch] variants)
    std::vector<hipEvent_t> kevents;
    std::vector<int> kvars;
    hipStream_t timed_stream = nullptr;
    // aux words of the T16 decision (sa_internal.h kAux*), one kAuxWords slot per pipeline slot
    uint32_t* aux = nullptr;
    // plan of the last call: one entry per kernel variant it enqueued (T16 first when the batch
    // was T16-eligible by scoring and shape; the device picked one by the batch alphabet, and
    // h_sel receives that choice asynchronously, ev_sel marks its arrival)
    int nvar = 0, var_kernel[2] = {0, 0}, var_R[2] = {0, 0}, var_W[2] = {0, 0}, var_records[2] = {0, 0};
    uint32_t* h_sel = nullptr;
    hipEvent_t ev_sel = nullptr;
    // the last call's selection when the host decided it (host_alphabet), else -1: then the
    // device's word arrives in h_sel (a host write there could race with a pending download)
    int host_sel = -1;
    // cross-call pipeline of the device API (sa_set_pipeline): fills on s_fill, tracebacks on
    // s_tb, kPipeSlots workspace slots; ev_slot[k] = traceback of the last call that used slot k done
    int pipeline = 0;
    // Band-unit hand-off buffer (score-only SW / NW fills, sa_fill_impl.h BU): the row granules, the
    // column-segment state and the per-unit maxima, all {tag, value} words polled by their consumers.
    // Only those fills write it (every kernel that touches it runs on the fill stream, so one copy
    // serves both pipeline slots), and it is zeroed when allocated and whenever hand_tag wraps: a word
    // there carries the tag of the launch that wrote it or 0, so a consumer can never take an earlier
    // launch's word -- of any shape -- for its producer's.  hand_tag: the last launch's tag, 1..65535.
    uint8_t* hand = nullptr;
    uint64_t hand_bytes = 0;
    uint32_t hand_tag = 0;
    bool hand_dirty = false;   // (tests: sa_test_hook poisoned it) zero before the next launch
    hipStream_t s_fill = nullptr, s_tb = nullptr;
    hipEvent_t ev_in = nullptr, ev_slot[kPipeSlots] = {};
    // The f16 SW cell (sa_fill_so2.hip FK) re-runs in int32 every pair whose score may pass 2,000.
    // Each of its launches has a number f16_seq; its end cell posts {seq, flagged pairs} to h_f16
    // (coherent pinned, d_f16 on the device) and f16_cnt[seq % 4] keeps the launch's pair count.
    // A launch that flagged more than 1/64 of its pairs turns the cell off for the context
    // (f16_off): such batches run the 16-bit integer cell, exact to 8,191, instead of re-running.
    unsigned long long* h_f16 = nullptr;
    unsigned long long* d_f16 = nullptr;
    uint32_t f16_seq = 0, f16_seen = 0, f16_cnt[4] = {};
    bool f16_off = false;
    uint64_t pipe_k = 0;
    // SPLIT plans (few pairs, one workgroup per band): [ticket, pad to 256 B][granules][partials]
    uint8_t* split = nullptr;
    uint64_t split_bytes = 0;
    // HirschbergSA / MyersMillerSA level-loop buffers and the host API's pinned upload staging
    sa::DcWork dc;
    sa::HostBuf<uint8_t> stage, ostage;
    // the small-call path (align_tiny): coherent pinned inputs and outputs the kernel reads and
    // writes in place (host pointer, device pointer)
    uint8_t* tiny_io = nullptr;
    uint8_t* tiny_dev = nullptr;
    // host API: download stream and per-chunk events (align_host)
    hipStream_t s_out = nullptr;
    std::vector<hipEvent_t> host_ev;
    // Calls on one context are ordered: every call's stream waits for ev_last, the end of the
    // last un-pipelined call (whatever stream it ran on), since they share the workspace, the
    // I/O cache and the DC buffers.
    hipEvent_t ev_last = nullptr;
    bool ev_last_set = false;
    // kernels the last call launched after its fills' end (ev[1]): walks, the segmented traceback,
    // the SPLIT fallback behind them.  A score call launches none, and sa_last_timings then reports
    // traceback_ms = 0 instead of the few microseconds between two event records
    int tb_kernels = 0;
};

namespace sa {

// Defined in sa_api.hip.
int fail(sa_ctx* c, int code, const std::string& msg);   // c may be NULL: the thread's text alone
int hip_fail(sa_ctx* c, hipError_t e, const char* what);
int order_after_last(sa_ctx* c, hipStream_t st);
int mark_last(sa_ctx* c, hipStream_t st);
int ensure_ws(sa_ctx* c, uint64_t need);
int ensure_io(sa_ctx* c, uint64_t need);
uint64_t ws_budget(sa_ctx* c);
bool lut_is_identity(const uint8_t* lut);
void par_for(uint64_t n, uint64_t grain, std::function<void(uint64_t, uint64_t)> fn);

#define SA_HIP(c, call)                                   \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(c, e_, #call); \
    } while (0)

// ---------------------------------------------------------------------------- argument checks
// The algorithm, scoring, free_ends and band checks of one family of calls, in the order the checks
// run: scoring, the algorithm's range, free_ends, the band overflow when `band_early` holds its text,
// the algorithm's class, gap_extend, the band overflow when `band` holds its text, band = 0.
struct CallRules {
    uint32_t algos;                      // bit a: the family takes algorithm a
    const char* unsupported;             // the message for the others
    bool free_ends = false;              // free_ends <= 15 is checked
    const char* band_early = nullptr;    // (the seeded calls: their own text, ahead of the algorithm's class)
    bool gap_extend = false;             // an affine algorithm needs gap_extend <= 0
    const char* band = nullptr;
    bool band0 = false;                  // band = 0 needs allow_mismatch
};
constexpr const char* kBandOverflow = "band: |n - m| + 2 * band + 1 diagonals overflow 32 bits";
constexpr uint32_t kAlgoMatrix = 1u << SA_SW | 1u << SA_NW | 1u << SA_LOCAL_GOTOH | 1u << SA_GLOBAL_GOTOH;
constexpr const char* kMatrixAlgos = "matrix calls support SA_SW, SA_NW, SA_LOCAL_GOTOH and SA_GLOBAL_GOTOH only";
// sa_align_batch_matrix / sa_score_batch_matrix / sa_matrix_plan_query, and the matrix band calls
constexpr CallRules kMatrixRules = {.algos = kAlgoMatrix, .unsupported = kMatrixAlgos};
constexpr CallRules kBandedMatrixRules = {.algos = kAlgoMatrix, .unsupported = kMatrixAlgos, .gap_extend = true, .band = kBandOverflow};
// the banded calls (sa_api_banded.hip) and the device-resident seeded ones (sa_api_banded_device.hip): the
// linear and affine bands' rules, and the seeded calls' own, which run ahead of their algorithm's
constexpr CallRules kLinearRules = {
    .algos = 1u << SA_SW | 1u << SA_NW | 1u << SA_HIRSCHBERG,
    .unsupported = "banded calls support the linear-gap algorithms only (SA_SW, SA_NW, SA_HIRSCHBERG)",
    .band = kBandOverflow, .band0 = true};
constexpr CallRules kAffineRules = {
    .algos = 1u << SA_LOCAL_GOTOH | 1u << SA_GLOBAL_GOTOH,
    .unsupported = "banded affine calls support SA_LOCAL_GOTOH and SA_GLOBAL_GOTOH only",
    .gap_extend = true, .band = kBandOverflow, .band0 = true};
constexpr uint32_t kAlgoGlobal = 1u << SA_NW | 1u << SA_HIRSCHBERG | 1u << SA_GLOBAL_GOTOH;
constexpr CallRules kSeededRules = {
    .algos = kAlgoGlobal,
    .unsupported = "seeded banded calls support the global algorithms SA_NW, SA_HIRSCHBERG and SA_GLOBAL_GOTOH only",
    .free_ends = true, .band_early = "band: 2 * band + 1 diagonals overflow 32 bits"};

inline int check_call(sa_ctx* c, const CallRules& r, int algo, const sa_scoring* sc, uint32_t band, uint32_t free_ends) {
    if (!sc) return fail(c, SA_ERR_ARG, "scoring is NULL");
    if (algo < SA_SW || algo > SA_MYERS_MILLER) return fail(c, SA_ERR_ARG, "unknown algorithm");
    if (r.free_ends && free_ends > 15) return fail(c, SA_ERR_ARG, "free_ends holds bits outside SA_FREE_*");
    if (r.band_early && band >= 0x80000000u) return fail(c, SA_ERR_ARG, r.band_early);
    if (!((r.algos >> algo) & 1)) return fail(c, SA_ERR_UNSUPPORTED, r.unsupported);
    if (r.gap_extend && is_affine(algo) && sc->gap_extend > 0)
        return fail(c, SA_ERR_UNSUPPORTED, "banded affine calls need gap_extend <= 0 (the records decide the walk only then)");
    if (r.band && band >= 0x80000000u) return fail(c, SA_ERR_ARG, r.band);
    if (r.band0 && band == 0 && !sc->allow_mismatch)
        return fail(c, SA_ERR_UNSUPPORTED, "band = 0 needs allow_mismatch (a one-diagonal band has no other candidate)");
    return SA_OK;
}

// The buffers of a host batch call (notb: a score call, which has no ops buffer).
inline int check_batch_buffers(sa_ctx* c, const uint8_t* seq1, const uint64_t* off1, const uint8_t* seq2, const uint64_t* off2,
                               uint32_t npairs, const sa_result* results, const uint8_t* ops, bool notb) {
    if (!off1 || !off2 || (npairs && (!results || (!notb && !ops)))) return fail(c, SA_ERR_ARG, "NULL buffer");
    if ((off1[npairs] && !seq1) || (off2[npairs] && !seq2)) return fail(c, SA_ERR_ARG, "NULL sequence buffer");
    if (off1[0] != 0 || off2[0] != 0) return fail(c, SA_ERR_ARG, "offsets must start at 0");
    for (uint32_t p = 0; p < npairs; ++p)
        if (off1[p + 1] < off1[p] || off2[p + 1] < off2[p]) return fail(c, SA_ERR_ARG, "offsets must be non-decreasing");
    return SA_OK;
}

// ------------------------------------------------------------------------------ matrix recode
// A matrix call's recode: the batch's K used symbols in byte order, their codes, the used K x K corner of
// the caller's table, dense (row stride K; K >= 1), and that corner's extremes (0 included).
struct SubRecode {
    uint8_t code[256];
    int syms[kSubMaxSyms];
    int K;
    std::vector<int16_t> tab;   // kSubMaxSyms^2 entries, the first K * K used
    int32_t smin, smax;
};
inline int sub_recode(sa_ctx* c, const uint8_t* seq1, uint64_t t1, const uint8_t* seq2, uint64_t t2, const int16_t* submat,
                      SubRecode* sub) {
    // the batch's symbols, both sides together: codes in byte order
    bool seen[256] = {};
    for (uint64_t k = 0; k < t1; ++k) seen[seq1[k]] = true;
    for (uint64_t k = 0; k < t2; ++k) seen[seq2[k]] = true;
    memset(sub->code, 0, sizeof(sub->code));
    int K = 0;
    for (int b = 0; b < 256; ++b)
        if (seen[b]) {
            if (K == kSubMaxSyms)
                return fail(c, SA_ERR_UNSUPPORTED, "matrix calls take batches of at most " + std::to_string(kSubMaxSyms) +
                                                       " distinct symbols (both sequence sets together)");
            sub->code[b] = (uint8_t)K;
            sub->syms[K++] = b;
        }
    if (K == 0) sub->syms[K++] = 0;   // (no symbol at all: a one-entry table, so that no lane indexes outside it)
    sub->K = K;
    sub->tab.assign(kSubMaxSyms * kSubMaxSyms, 0);
    sub->smax = sub->smin = 0;
    for (int a = 0; a < K; ++a)
        for (int b = 0; b < K; ++b) {
            const int16_t s = submat[sub->syms[a] * 256 + sub->syms[b]];
            sub->tab[a * K + b] = s;
            sub->smax = std::max<int32_t>(sub->smax, s);
            sub->smin = std::min<int32_t>(sub->smin, s);
        }
    return SA_OK;
}
// What the host's decisions read of a matrix call's scoring: the diagonal term's extremes as match /
// mismatch, with mismatches allowed.
inline sa_scoring sub_scoring(const sa_scoring& sc, const SubRecode& sub) {
    sa_scoring s = sc;
    s.match = sub.smax;
    s.mismatch = sub.smin;
    s.allow_mismatch = 1;
    return s;
}

}  // namespace sa
