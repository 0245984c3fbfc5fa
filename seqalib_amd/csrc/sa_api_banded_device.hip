// sa_api_banded_device.hip — the host layer of the device-resident seeded band calls of the C ABI
// (include/seqalib_hip.h: sa_align_batch_banded_seeded_device, sa_score_batch_banded_seeded_device,
// sa_banded_seeded_device_plan_query).  The host knows the bound shape only: it checks what that decides,
// provisions records for the bound (sa_band_plan.h band_plan_bound_seeded), cuts the pairs into chunks that fit
// the workspace, and per chunk enqueues the planner (sa_band_planner.hip), every fill variant up to the
// bound's with the grid of a full chunk, and one walk -- all on the caller's stream, with no read of a length
// and no synchronisation.  The kernels live in sa_banded_seeded_dev.hip / sa_banded_affine_seeded_dev.hip;
// this unit defines none.  DESIGN.md §2.20.
#include <stdlib.h>

#include "sa_api_ctx.h"
#include "sa_band_plan.h"

using namespace sa;

namespace {

struct SeededDeviceCall {
    int algo;
    const sa_scoring* sc;
    const uint8_t* seq1;
    uint64_t seq1_bytes;
    const uint64_t* start1;
    const uint32_t* len1;
    const uint8_t* seq2;
    uint64_t seq2_bytes;
    const uint64_t* start2;
    const uint32_t* len2;
    uint32_t npairs, max_m, max_n;
    const uint8_t* lut;
    const int32_t* diag;
    uint32_t band, free_ends;
    sa_result* res;
    uint8_t* ops;              // notb: NULL
    const uint64_t* ops_off;
    uint64_t ops_bytes;
    void* stream;
    bool notb;
};

// What the bound shape decides: SA_ERR_UNSUPPORTED, or the bound the call provisions from.
int bound_checks(sa_ctx* c, bool affine, const sa_scoring* sc, uint32_t max_m, uint32_t max_n, uint32_t band, BandPlanBound* b) {
    if (max_m >= (1u << 24) || max_n >= (1u << 24)) return fail(c, SA_ERR_UNSUPPORTED, "sequence length >= 2^24");
    auto a = [](int32_t x) { return (int64_t)(x < 0 ? -(int64_t)x : x); };
    const int64_t gap = affine ? a(sc->gap_open) + a(sc->gap_extend) : a(sc->gap);
    const int64_t big = std::max(std::max(gap, a(sc->match)), sc->allow_mismatch ? a(sc->mismatch) : 0);
    if (((int64_t)max_m + max_n + 1) * big + (affine ? 10000 : 0) >= kBandScoreLimit)
        return fail(c, SA_ERR_UNSUPPORTED,
                    affine ? "device seeded calls need (max_m + max_n + 1) * max(|gap_open| + |gap_extend|, |match|, |mismatch|) + 10000 < 2^29"
                           : "device seeded calls need (max_m + max_n + 1) * max(|gap|, |match|, |mismatch|) < 2^29");
    *b = band_plan_bound_seeded((int32_t)max_m, (int32_t)max_n, (int32_t)std::min(band, kBandMaxW), affine);
    if (b->vmax < 0)
        return fail(c, SA_ERR_UNSUPPORTED,
                    "a band of min(2 * band + 1, max_m + max_n + 1) diagonals exceeds the " +
                        (affine ? std::to_string(kBandAffineMaxDiagonals) + " one wave holds with three values per cell"
                                : std::to_string(kBandMaxDiagonals) + " one wave holds"));
    return SA_OK;
}

const sa_scoring kAnyScoring{0, 0, 0, 0, 0, 1};

int seeded_device_batch(sa_ctx* c, const SeededDeviceCall& k) {
    // ---- the checks that need no context
    int rc = check_call(c, kSeededRules, k.algo, k.sc, k.band, k.free_ends);
    if (rc) return rc;
    if (k.npairs && (!k.start1 || !k.len1 || !k.start2 || !k.len2 || !k.diag || !k.res || (!k.notb && (!k.ops || !k.ops_off))))
        return fail(c, SA_ERR_ARG, "NULL buffer");
    if (k.npairs && ((k.seq1_bytes && !k.seq1) || (k.seq2_bytes && !k.seq2))) return fail(c, SA_ERR_ARG, "NULL sequence buffer");
    const bool affine = k.algo == SA_GLOBAL_GOTOH;
    if ((rc = check_call(c, affine ? kAffineRules : kLinearRules, k.algo, k.sc, k.band, k.free_ends))) return rc;
    BandPlanBound bound;
    if ((rc = bound_checks(c, affine, k.sc, k.max_m, k.max_n, k.band, &bound))) return rc;
    if (!c) return fail(nullptr, SA_ERR_ARG, "ctx is NULL");
    if (!k.npairs) return SA_OK;

    // ---- chunks: [head][plan records][lists][records], the last three sized by the chunk's pairs
    SA_HIP(c, hipSetDevice(c->device));
    const uint64_t rec_words = k.notb ? 0 : bound.rec_words;
    const uint64_t fixed = 4ull * kBandPlanHeadWords + 512;   // (the head, and the two blocks' alignment)
    const uint64_t budget = ws_budget(c);
    const uint32_t per = budget > fixed ? band_plan_chunk_pairs(rec_words + kBandPlanWords, budget - fixed, k.npairs) : 0;
    if (!per)
        return fail(c, SA_ERR_NOMEM, "one pair's provision (" + std::to_string((rec_words + kBandPlanWords) * 4 + fixed) +
                                         " bytes: the bound shape's band records and its plan) exceeds the workspace limit");
    auto al = [](uint64_t x) { return (x + 255) & ~(uint64_t)255; };
    const uint64_t b_head = 4ull * kBandPlanHeadWords, b_plans = al(sizeof(BandPlanRec) * (uint64_t)per), b_lists = al(4ull * per);
    hipStream_t st = k.stream ? (hipStream_t)k.stream : c->stream;
    if ((rc = order_after_last(c, st))) return rc;
    // pipelined device calls (sa_set_pipeline) do not mark the context's last call: their slots' events do, and
    // this call uses the workspace they share -- ordered behind them on the device, not waited for on the host
    for (hipEvent_t ev : c->ev_slot)
        if (ev) SA_HIP(c, hipStreamWaitEvent(st, ev, 0));
    if ((rc = ensure_ws(c, b_head + b_plans + b_lists + 4ull * rec_words * per))) return rc;
    uint32_t* bits = nullptr;
    if (k.lut) {   // the bit table lives in the tail of the I/O cache, as sa_align_batch_device keeps it
        if ((rc = ensure_io(c, 8192))) return rc;
        bits = reinterpret_cast<uint32_t*>(c->io + c->io_bytes - 8192);
        SA_HIP(c, launch_band_lut_bits(k.lut, bits, st));
    }
    uint32_t* const head = reinterpret_cast<uint32_t*>(c->ws);
    BandPlanRec* const plans = reinterpret_cast<BandPlanRec*>(c->ws + b_head);
    uint32_t* const lists = reinterpret_cast<uint32_t*>(c->ws + b_head + b_plans);
    uint32_t* const recs = reinterpret_cast<uint32_t*>(c->ws + b_head + b_plans + b_lists);

    const bool kernel_timing = getenv("SEQALIB_KERNEL_TIMING") != nullptr;
    c->launches = 0;
    c->kvars.clear();
    c->timed_stream = st;
    c->tb_kernels = 0;
    const sa_scoring* const sc = k.sc;
    for (uint32_t first = 0; first < k.npairs; first += per) {
        const uint32_t count = std::min(per, k.npairs - first);
        while ((int)c->events.size() < 3 * (c->launches + 1)) {
            hipEvent_t ev;
            SA_HIP(c, hipEventCreate(&ev));
            c->events.push_back(ev);
        }
        hipEvent_t* ev = &c->events[3 * c->launches];
        hipEvent_t* kev = nullptr;
        if (kernel_timing) {   // the fills alone: sa_last_kernel_timings; fill_ms less that is the planner's share
            while ((int)c->kevents.size() < kKEv * (c->launches + 1)) {
                hipEvent_t e;
                SA_HIP(c, hipEventCreate(&e));
                c->kevents.push_back(e);
            }
            c->kvars.resize(c->launches + 1);
            c->kvars[c->launches] = 1;
            kev = &c->kevents[kKEv * c->launches];
        }
        BandPlannerParams pp;
        pp.seq1 = k.seq1;
        pp.seq1_bytes = k.seq1_bytes;
        pp.start1 = k.start1;
        pp.len1 = k.len1;
        pp.seq2 = k.seq2;
        pp.seq2_bytes = k.seq2_bytes;
        pp.start2 = k.start2;
        pp.len2 = k.len2;
        pp.diag = k.diag;
        pp.ops_off = k.notb ? nullptr : k.ops_off;
        pp.ops_bytes = k.ops_bytes;
        pp.res = k.res;
        pp.first = first;
        pp.count = count;
        pp.max_m = k.max_m;
        pp.max_n = k.max_n;
        pp.w = (int32_t)std::min(k.band, kBandMaxW);
        pp.free_ends = k.free_ends;
        pp.affine = affine;
        pp.vmax = bound.vmax;
        pp.span = bound.span;
        pp.bound_words = rec_words;
        pp.head = head;
        pp.plans = plans;
        pp.lists = lists;
        BandAffineParams bp;   // (the linear launchers take its BandParams base); read as sa_internal.h kBandSeededDev says
        bp.seq1 = k.seq1;
        bp.off1 = reinterpret_cast<const uint64_t*>(plans);
        bp.seq2 = k.seq2;
        bp.off2 = nullptr;     // per variant below
        bp.lutbits = bits;
        bp.idx = lists;
        bp.recoff = nullptr;
        bp.rec = recs;
        bp.res = k.res;
        bp.ops = k.ops;
        bp.count = count;
        bp.band = (uint32_t)pp.w;
        bp.gap = sc->gap;
        bp.match = sc->match;
        bp.mismatch = sc->allow_mismatch ? sc->mismatch : kBandNeg;
        bp.allow = sc->allow_mismatch;
        bp.R = 0;
        bp.L = 0;
        bp.submat = nullptr;
        bp.sub_k = 0;
        bp.free_ends = k.free_ends;
        bp.gap_open = sc->gap_open;
        bp.gap_extend = sc->gap_extend;
        SA_HIP(c, hipEventRecord(ev[0], st));
        SA_HIP(c, launch_band_planner(pp, st));
        if (kev) SA_HIP(c, hipEventRecord(kev[0], st));
        for (int v = 0; v <= bound.vmax; ++v) {
            bp.off2 = reinterpret_cast<const uint64_t*>(head + kBandPlanHeadLists + 2 * v);
            SA_HIP(c, affine ? launch_banded_affine_seeded_dev_fill(v, bits != nullptr, !k.notb, bp, st)
                             : launch_banded_seeded_dev_fill(v, bits != nullptr, !k.notb, bp, st));
        }
        if (kev) SA_HIP(c, hipEventRecord(kev[1], st));
        SA_HIP(c, hipEventRecord(ev[1], st));
        if (!k.notb) {
            SA_HIP(c, affine ? launch_banded_affine_seeded_dev_tb(bits != nullptr, bp, st) : launch_banded_seeded_dev_tb(bits != nullptr, bp, st));
            c->tb_kernels++;
        }
        SA_HIP(c, hipEventRecord(ev[2], st));
        c->launches++;
    }
    c->nvar = 1;
    c->host_sel = -1;
    c->var_kernel[0] = SA_KERNEL_BANDED;
    c->var_R[0] = kBandR[bound.vmax];
    c->var_W[0] = 1;
    c->var_records[0] = k.notb ? SA_RECORDS_NONE : affine ? SA_RECORDS_BAND4 : SA_RECORDS_BAND2;
    return mark_last(c, st);
}

}  // namespace

extern "C" {

int sa_align_batch_banded_seeded_device(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* d_seq1, uint64_t seq1_bytes,
                                        const uint64_t* d_start1, const uint32_t* d_len1, const uint8_t* d_seq2, uint64_t seq2_bytes,
                                        const uint64_t* d_start2, const uint32_t* d_len2, uint32_t npairs, uint32_t max_m,
                                        uint32_t max_n, const uint8_t* d_match_lut, const int32_t* d_diag, uint32_t band,
                                        uint32_t free_ends, sa_result* d_results, uint8_t* d_ops, const uint64_t* d_ops_off,
                                        uint64_t ops_bytes, void* stream) {
    return seeded_device_batch(c, SeededDeviceCall{algo, sc, d_seq1, seq1_bytes, d_start1, d_len1, d_seq2, seq2_bytes, d_start2, d_len2,
                                                   npairs, max_m, max_n, d_match_lut, d_diag, band, free_ends, d_results, d_ops,
                                                   d_ops_off, ops_bytes, stream, false});
}

int sa_score_batch_banded_seeded_device(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* d_seq1, uint64_t seq1_bytes,
                                        const uint64_t* d_start1, const uint32_t* d_len1, const uint8_t* d_seq2, uint64_t seq2_bytes,
                                        const uint64_t* d_start2, const uint32_t* d_len2, uint32_t npairs, uint32_t max_m,
                                        uint32_t max_n, const uint8_t* d_match_lut, const int32_t* d_diag, uint32_t band,
                                        uint32_t free_ends, sa_result* d_results, void* stream) {
    return seeded_device_batch(c, SeededDeviceCall{algo, sc, d_seq1, seq1_bytes, d_start1, d_len1, d_seq2, seq2_bytes, d_start2, d_len2,
                                                   npairs, max_m, max_n, d_match_lut, d_diag, band, free_ends, d_results, nullptr,
                                                   nullptr, 0, stream, true});
}

int sa_banded_seeded_device_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t band, int* widest_cells_per_lane,
                                       uint64_t* record_bytes_per_pair, uint64_t* plan_bytes_per_pair) {
    int rc = check_call(nullptr, kSeededRules, algo, &kAnyScoring, band, 0);
    if (rc) return rc;
    const bool affine = algo == SA_GLOBAL_GOTOH;
    BandPlanBound bound;
    if ((rc = bound_checks(nullptr, affine, &kAnyScoring, max_m, max_n, band, &bound))) return rc;
    if (widest_cells_per_lane) *widest_cells_per_lane = kBandR[bound.vmax];
    if (record_bytes_per_pair) *record_bytes_per_pair = bound.rec_words * 4;
    if (plan_bytes_per_pair) *plan_bytes_per_pair = kBandPlanWords * 4;
    return SA_OK;
}

}  // extern "C"
