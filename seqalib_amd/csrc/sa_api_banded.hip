// sa_api_banded.hip — the host layer of the banded calls of the C ABI (include/seqalib_hip.h): checks,
// grouping into launches (sa_band_group.h), device layout, the launch loop and the download.  The
// kernels live in sa_banded*.hip; this unit defines none.
//
// Every pair gets the fill variant (cells per lane R, lanes per pair L) its clipped band fits; the pairs of
// one variant are launched together, longest first, in as many launches as sa_set_workspace_limit leaves
// room for their records.  A score call stores no records and launches no walk.  The linear, affine,
// matrix, ends-free, seeded and extension calls differ in their checks, variant list, record size and
// launchers only.
#include <stdlib.h>

#include "sa_api_ctx.h"
#include "sa_band_group.h"
#include "sa_band_plan.h"

using namespace sa;

namespace {

// ------------------------------------------------------------------------------------ the call
// One banded call, as its entry point describes it.
struct BandCall {
    int algo;
    const sa_scoring* sc;
    const uint8_t* seq1;
    const uint64_t* off1;
    const uint8_t* seq2;
    const uint64_t* off2;
    uint32_t npairs;
    const uint8_t* lut;
    uint32_t band;
    sa_result* results;
    uint8_t* ops;          // notb: NULL, ops_cap 0
    uint64_t ops_cap;
    bool notb;             // a score call: no records, no walk, no ops
    // the family
    const CallRules* rules = nullptr;   // the checks banded_batch runs first (NULL: the entry point has run its own)
    bool affine = false;                // 4-bit records, the first kBandAffineVariants variants, gap_open / gap_extend
    // the matrix band calls: *sc holds the table's extremes as match / mismatch with allow_mismatch = 1 (what
    // banded_pair_plan bounds the scores by), lut only labels, the sequences are recoded on their way up
    const SubRecode* sub = nullptr;
    // the ends-free calls: the SA_FREE_* bits for their fills and walks; all else is the global call's
    bool ends_free = false;
    uint32_t free_ends = 0;
    // the seeded calls (ends-free too; the entry point has checked -m <= diag[p] <= n): every pair's band lies
    // round its seed diagonal, which travels behind each launch's idx entries.  diag may be NULL when npairs is 0
    bool seeded = false;
    const int32_t* diag = nullptr;
    // the extension calls: the seeded band round diagonal 0 for every pair (no diagonals travel), NW's or
    // GlobalGotoh's borders, and xdrop for their fills
    bool extend = false;
    int32_t xdrop = SA_XDROP_OFF;
};

// (kLinearRules, kAffineRules, kAlgoGlobal and kSeededRules: sa_api_ctx.h, shared with sa_api_banded_device.hip)
// the ends-free and seeded calls' own checks; the linear or affine rules of their algorithm follow
// (banded_batch), for the seeded calls behind the diag checks
constexpr CallRules kEndsFreeRules = {
    .algos = kAlgoGlobal,
    .unsupported = "ends-free banded calls support the global algorithms SA_NW, SA_HIRSCHBERG and SA_GLOBAL_GOTOH only",
    .free_ends = true};
constexpr CallRules kExtendRules = {
    .algos = kAlgoGlobal,
    .unsupported = "banded extension calls support the global algorithms SA_NW, SA_HIRSCHBERG and SA_GLOBAL_GOTOH only",
    .band_early = "band: 2 * band + 1 diagonals overflow 32 bits"};

// What the launch loop and the plan read of a call's family, fixed for the whole call.  The launchers
// (sa_internal.h) differ in their signatures; fill and walk adapt them: the ends-free and seeded ones take
// no algorithm and only kMatchEq / kMatchLut, as the extension ones; the linear ones the BandParams base of
// the block.
using BandFill = hipError_t (*)(int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s);
using BandWalk = hipError_t (*)(int algo, bool lut, const BandAffineParams& p, hipStream_t s);
struct BandFamily {
    BandFill fill;
    BandWalk walk;
    uint64_t (*rec_words)(const BandGeom&, int);
    int nvariants;
    int records;   // SA_RECORDS_*
};
constexpr BandFamily linear_family(BandFill fill, BandWalk walk) {
    return {fill, walk, band_rec_words, kBandVariants, SA_RECORDS_BAND2};
}
constexpr BandFamily affine_family(BandFill fill, BandWalk walk) {
    return {fill, walk, band_affine_rec_words, kBandAffineVariants, SA_RECORDS_BAND4};
}
const BandFamily kBandFamilies[4][2] = {   // [corridor, ends-free, seeded, extension][linear, affine]
    {linear_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_fill(algo, v, mm, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_tb(algo, lut, p, s); }),
     affine_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_fill(algo, v, mm, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_tb(algo, lut, p, s); })},
    {linear_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_free_fill(v, mm == kMatchLut, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_free_tb(lut, p, s); }),
     affine_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_free_fill(v, mm == kMatchLut, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_free_tb(lut, p, s); })},
    {linear_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_seeded_fill(v, mm == kMatchLut, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_seeded_tb(lut, p, s); }),
     affine_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_seeded_fill(v, mm == kMatchLut, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_seeded_tb(lut, p, s); })},
    {linear_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_extend_fill(v, mm == kMatchLut, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_extend_tb(lut, p, s); }),
     affine_family([](int algo, int v, int mm, bool rec, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_extend_fill(v, mm == kMatchLut, rec, p, s); },
                   [](int algo, bool lut, const BandAffineParams& p, hipStream_t s) { return launch_banded_affine_extend_tb(lut, p, s); })},
};
const BandFamily& band_family(bool extend, bool seeded, bool ends_free, bool affine) {
    return kBandFamilies[extend ? 3 : seeded ? 2 : ends_free ? 1 : 0][affine];
}

// ------------------------------------------------------------------------------ per-pair limits
// The seeded calls' band of one pair (seed NULL: the corridor band of every other call).
struct BandSeed {
    int32_t diag;        // the seed diagonal, -m <= diag <= n (checked by the caller)
    uint32_t free_ends;
    uint64_t pair;       // for the message
    bool extend = false; // the extension calls: diag 0, no legality rule (the anchor (0, 0) is in every band), SW's key limit
};

// The seeded legality rule: the band must hold a legal begin and a legal end (include/seqalib_hip.h).
int banded_seed_legal(sa_ctx* c, const BandSeed& sd, const BandGeom& g, int64_t m, int64_t n) {
    const int legal = band_seed_legality(g, m, n, sd.free_ends);   // (sa_band_plan.h: the device planner's rule too)
    const bool begin = legal & 1, end = legal & 2;
    if (legal == kBandSeedLegal) return SA_OK;
    return fail(c, SA_ERR_UNSUPPORTED,
                "pair " + std::to_string(sd.pair) + ": the band [" + std::to_string(g.lo) + ", " + std::to_string(g.hi) +
                    "] holds no legal " + (begin ? "end" : end ? "begin" : "begin and no legal end") +
                    " under free_ends = " + std::to_string(sd.free_ends));
}

int banded_seed_in_matrix(sa_ctx* c, uint64_t pair, uint64_t m, uint64_t n, int32_t diag) {
    if ((int64_t)diag < -(int64_t)m || (int64_t)diag > (int64_t)n)
        return fail(c, SA_ERR_ARG, "pair " + std::to_string(pair) + ": seed diagonal " + std::to_string(diag) +
                                       " does not cross the " + std::to_string(m) + " x " + std::to_string(n) + " matrix");
    return SA_OK;
}

// One pair's geometry and fill variant, or why the banded path does not take it.
int banded_pair_plan(sa_ctx* c, int algo, const sa_scoring* sc, uint64_t m, uint64_t n, uint32_t band, BandGeom* g,
                     int* variant, const BandSeed* seed) {
    if (m >= (1u << 24) || n >= (1u << 24)) return fail(c, SA_ERR_UNSUPPORTED, "sequence length >= 2^24");
    auto a = [](int32_t x) { return (int64_t)(x < 0 ? -(int64_t)x : x); };
    auto geom = [&]() {
        const int32_t w = (int32_t)std::min(band, kBandMaxW);
        return seed ? band_geom_seeded((int32_t)m, (int32_t)n, w, seed->diag) : band_geom((int32_t)m, (int32_t)n, w);
    };
    // (the linear calls never get here with the affine algorithms; the affine bound keeps the Gotoh borders' 10000)
    const bool affine = is_affine(algo);
    const int64_t gap = affine ? a(sc->gap_open) + a(sc->gap_extend) : a(sc->gap);
    const int64_t big = std::max(std::max(gap, a(sc->match)), sc->allow_mismatch ? a(sc->mismatch) : 0);
    if ((int64_t)(m + n + 1) * big + (affine ? 10000 : 0) >= kBandScoreLimit)
        return fail(c, SA_ERR_UNSUPPORTED,
                    affine ? "banded affine calls need (m + n + 1) * max(|gap_open| + |gap_extend|, |match|, |mismatch|) + 10000 < 2^29"
                           : "banded calls need (m + n + 1) * max(|gap|, |match|, |mismatch|) < 2^29");
    *g = geom();
    *variant = affine ? band_affine_variant(g->beff) : band_variant(g->beff);
    if (*variant < 0)
        return fail(c, SA_ERR_UNSUPPORTED,
                    "band of " + std::to_string(g->beff) + " diagonals inside the matrix exceeds the " +
                        (affine ? std::to_string(kBandAffineMaxDiagonals) + " one wave holds with three values per cell"
                                : std::to_string(kBandMaxDiagonals) + " one wave holds"));
    if ((algo == SA_SW || algo == SA_LOCAL_GOTOH) && (m + 1) * (uint64_t)g->beff >= (1ull << 31))
        return fail(c, SA_ERR_UNSUPPORTED, affine ? "banded LocalGotoh needs (m + 1) * band diagonals < 2^31"
                                                  : "banded SW needs (m + 1) * band diagonals < 2^31");
    if (seed && seed->extend)
        return (m + 1) * (uint64_t)g->beff >= (1ull << 31)
                   ? fail(c, SA_ERR_UNSUPPORTED, "banded extension needs (m + 1) * band diagonals < 2^31")
                   : SA_OK;
    return seed ? banded_seed_legal(c, *seed, *g, (int64_t)m, (int64_t)n) : SA_OK;
}

// The band algorithm of a call: Hirschberg's global alignment is NW's.
int band_algo(int algo) { return algo == SA_HIRSCHBERG ? SA_NW : algo; }

// Every pair's limits, in pair order (with the offsets' order, which the lengths rest on).
int banded_pair_limits(sa_ctx* c, const BandCall& k) {
    for (uint32_t p = 0; p < k.npairs; ++p) {
        if (k.off1[p + 1] < k.off1[p] || k.off2[p + 1] < k.off2[p]) return fail(c, SA_ERR_ARG, "offsets must be non-decreasing");
        const BandSeed sd{k.seeded ? k.diag[p] : 0, k.free_ends, p, k.extend};
        BandGeom g;
        int v = 0;
        if (int rc = banded_pair_plan(c, band_algo(k.algo), k.sc, k.off1[p + 1] - k.off1[p], k.off2[p + 1] - k.off2[p], k.band,
                                      &g, &v, k.seeded || k.extend ? &sd : nullptr))
            return rc;
    }
    return SA_OK;
}

// ------------------------------------------------------------------------------------ phases
// The linear corridor calls leave their per-pair limits to the context (banded_plan); every other
// family's answer without one as well.
bool early_limits(const BandCall& k) { return k.affine || k.sub || k.ends_free || k.extend; }

// The checks that need no context, so they answer without a device too.
int banded_checks(sa_ctx* c, const BandCall& k) {
    if (k.rules)
        if (int rc = check_call(c, *k.rules, k.algo, k.sc, k.band, k.free_ends)) return rc;
    return early_limits(k) && k.off1 && k.off2 ? banded_pair_limits(c, k) : SA_OK;
}

// The context's and the buffers' checks; *ops_total: the bytes of ops the call writes.
int banded_buffers(sa_ctx* c, const BandCall& k, uint64_t* ops_total) {
    if (!c) return fail(nullptr, SA_ERR_ARG, "ctx is NULL");
    if (int rc = check_batch_buffers(c, k.seq1, k.off1, k.seq2, k.off2, k.npairs, k.results, k.ops, k.notb)) return rc;
    *ops_total = k.notb ? 0 : k.off1[k.npairs] + k.off2[k.npairs] + k.npairs;
    if (k.ops_cap < *ops_total) return fail(c, SA_ERR_CAPACITY, "ops buffer needs " + std::to_string(*ops_total) + " bytes");
    return SA_OK;
}

// The call's launches (sa_band_group.h) and a workspace that holds the largest one's records.
int banded_plan(sa_ctx* c, const BandCall& k, const BandFamily& fam, BandGroups* grp) {
    if (!early_limits(k))
        if (int rc = banded_pair_limits(c, k)) return rc;
    const std::vector<int32_t> zero_diag(k.extend ? k.npairs : 0, 0);   // the extension band: every pair round diagonal 0
    BandGroupIn in{k.off1, k.off2, k.npairs, k.extend ? zero_diag.data() : k.seeded ? k.diag : nullptr, (int32_t)std::min(k.band, kBandMaxW),
                   fam.nvariants, fam.rec_words, k.notb, 0, 0, true};
    in.budget_words = k.notb ? 0 : ws_budget(c) / 4;
    const char* merge_env = getenv("SEQALIB_BAND_MERGE");
    in.merge = !(merge_env && merge_env[0] == '0');
    if (in.merge) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) cus = 256;
        in.simds = 4ull * (uint64_t)cus;
    }
    if (!band_group(in, grp))
        return fail(c, SA_ERR_NOMEM, "the band records of one pair (" + std::to_string(grp->too_big_words * 4) +
                                         " bytes) exceed the workspace limit");
    if (!k.notb)
        if (int rc = ensure_ws(c, std::max<uint64_t>(grp->ws_words * 4, 256))) return rc;
    if (k.seeded) grp->idx = band_idx_with_diagonals(*grp, k.diag);
    return SA_OK;
}

// The call's device buffers, all inside the context's I/O cache.
struct BandDevice {
    uint8_t* d1;
    uint8_t* d2;
    uint64_t* do1;
    uint64_t* do2;
    sa_result* dres;
    uint8_t* dops;
    uint32_t* dbits;   // the label table, when the call has one that is not byte equality (use_lut)
    uint32_t* didx;
    uint64_t* dro;
    int16_t* dtab;     // the matrix band calls' table
    bool use_lut;
    uint64_t b_res;    // bytes of the result block (the staging's layout)
};

int banded_upload(sa_ctx* c, const BandCall& k, const BandGroups& grp, uint64_t ops_total, BandDevice* d) {
    const uint32_t npairs = k.npairs;
    const uint64_t t1 = k.off1[npairs], t2 = k.off2[npairs];
    const SubRecode* const sub = k.sub;
    d->use_lut = k.lut && !lut_is_identity(k.lut);
    std::vector<uint32_t> bits;
    if (d->use_lut) {
        bits.assign(2048, 0);
        if (sub) {   // the walk reads codes: the label table over codes (equality of codes is equality of bytes)
            for (int a = 0; a < sub->K; ++a)
                for (int b = 0; b < sub->K; ++b)
                    if (k.lut[sub->syms[a] * 256 + sub->syms[b]]) bits[a * 8 + b / 32] |= 1u << (b % 32);
        } else {
            for (int a = 0; a < 256; ++a)
                for (int b = 0; b < 256; ++b)
                    if (k.lut[a * 256 + b]) bits[a * 8 + b / 32] |= 1u << (b % 32);
        }
    }
    auto al = [](uint64_t x) { return (x + 255) & ~(uint64_t)255; };
    const uint64_t b_s1 = al(t1 + 1), b_s2 = al(t2 + 1), b_o = al(8ull * (npairs + 1)), b_res = al(sizeof(sa_result) * (uint64_t)npairs);
    const uint64_t b_ops = al(ops_total + 1), b_bits = al(8192), b_idx = al(4ull * grp.idx.size()), b_ro = al(8ull * npairs);
    const uint64_t b_tab = sub ? al(2ull * kSubMaxSyms * kSubMaxSyms) : 0;
    if (int rc = ensure_io(c, b_s1 + b_s2 + 2 * b_o + b_res + b_ops + b_bits + b_idx + b_ro + b_tab)) return rc;
    uint8_t* q = c->io;
    d->d1 = q; q += b_s1;
    d->d2 = q; q += b_s2;
    d->do1 = reinterpret_cast<uint64_t*>(q); q += b_o;
    d->do2 = reinterpret_cast<uint64_t*>(q); q += b_o;
    d->dres = reinterpret_cast<sa_result*>(q); q += b_res;
    d->dops = q; q += b_ops;
    d->dbits = reinterpret_cast<uint32_t*>(q); q += b_bits;
    d->didx = reinterpret_cast<uint32_t*>(q); q += b_idx;
    d->dro = reinterpret_cast<uint64_t*>(q); q += b_ro;
    d->dtab = reinterpret_cast<int16_t*>(q);
    d->b_res = b_res;
    hipStream_t st = c->stream;
    if (sub) {   // pinned staging: [Seq1 codes][Seq2 codes][table]
        SA_HIP(c, c->stage.alloc(b_s1 + b_s2 + b_tab));
        uint8_t* const h1 = c->stage.data();
        uint8_t* const h2 = h1 + b_s1;
        const uint8_t* const code = sub->code;
        const uint8_t* const seq1 = k.seq1;
        const uint8_t* const seq2 = k.seq2;
        par_for(t1, 1u << 20, [&](uint64_t lo, uint64_t hi) { for (uint64_t i = lo; i < hi; ++i) h1[i] = code[seq1[i]]; });
        par_for(t2, 1u << 20, [&](uint64_t lo, uint64_t hi) { for (uint64_t i = lo; i < hi; ++i) h2[i] = code[seq2[i]]; });
        memcpy(h2 + b_s2, sub->tab.data(), 2ull * kSubMaxSyms * kSubMaxSyms);
        if (t1) SA_HIP(c, hipMemcpyAsync(d->d1, h1, t1, hipMemcpyHostToDevice, st));
        if (t2) SA_HIP(c, hipMemcpyAsync(d->d2, h2, t2, hipMemcpyHostToDevice, st));
        SA_HIP(c, hipMemcpyAsync(d->dtab, h2 + b_s2, 2ull * kSubMaxSyms * kSubMaxSyms, hipMemcpyHostToDevice, st));
    } else {
        if (t1) SA_HIP(c, hipMemcpyAsync(d->d1, k.seq1, t1, hipMemcpyHostToDevice, st));
        if (t2) SA_HIP(c, hipMemcpyAsync(d->d2, k.seq2, t2, hipMemcpyHostToDevice, st));
    }
    SA_HIP(c, hipMemcpyAsync(d->do1, k.off1, 8ull * (npairs + 1), hipMemcpyHostToDevice, st));
    SA_HIP(c, hipMemcpyAsync(d->do2, k.off2, 8ull * (npairs + 1), hipMemcpyHostToDevice, st));
    if (d->use_lut) SA_HIP(c, hipMemcpyAsync(d->dbits, bits.data(), 8192, hipMemcpyHostToDevice, st));
    SA_HIP(c, hipMemcpyAsync(d->didx, grp.idx.data(), 4ull * grp.idx.size(), hipMemcpyHostToDevice, st));
    SA_HIP(c, hipMemcpyAsync(d->dro, grp.recoff.data(), 8ull * npairs, hipMemcpyHostToDevice, st));
    return SA_OK;
}

// Fill and walk of every launch, with the context's timing events round them, and the call's plan.
int banded_launch(sa_ctx* c, const BandCall& k, const BandFamily& fam, const BandGroups& grp, const BandDevice& d) {
    hipStream_t st = c->stream;
    const sa_scoring* const sc = k.sc;
    const bool kernel_timing = getenv("SEQALIB_KERNEL_TIMING") != nullptr;
    c->launches = 0;
    c->kvars.clear();
    c->timed_stream = st;
    c->tb_kernels = 0;
    const int algo = band_algo(k.algo);
    const int mm = k.sub ? kMatchSub : d.use_lut ? kMatchLut : kMatchEq;
    const uint32_t idx_stride = k.seeded ? 2 : 1;
    for (const BandLaunch& ln : grp.launches) {
        while ((int)c->events.size() < 3 * (c->launches + 1)) {
            hipEvent_t ev;
            SA_HIP(c, hipEventCreate(&ev));
            c->events.push_back(ev);
        }
        hipEvent_t* ev = &c->events[3 * c->launches];
        hipEvent_t* kev = nullptr;
        if (kernel_timing) {
            while ((int)c->kevents.size() < kKEv * (c->launches + 1)) {
                hipEvent_t e;
                SA_HIP(c, hipEventCreate(&e));
                c->kevents.push_back(e);
            }
            c->kvars.resize(c->launches + 1);
            c->kvars[c->launches] = 1;
            kev = &c->kevents[kKEv * c->launches];
        }
        BandAffineParams bp;   // (the linear launchers take its BandParams base)
        bp.seq1 = d.d1;
        bp.off1 = d.do1;
        bp.seq2 = d.d2;
        bp.off2 = d.do2;
        bp.lutbits = d.use_lut ? d.dbits : nullptr;
        bp.idx = d.didx + (uint64_t)idx_stride * ln.first;
        bp.recoff = d.dro + ln.first;
        bp.rec = reinterpret_cast<uint32_t*>(c->ws);
        bp.res = d.dres;
        bp.ops = d.dops;
        bp.count = ln.count;
        bp.band = std::min(k.band, kBandMaxW);
        bp.gap = sc->gap;
        bp.match = sc->match;
        bp.mismatch = sc->allow_mismatch ? sc->mismatch : kBandNeg;
        bp.allow = sc->allow_mismatch;
        bp.R = kBandR[ln.v];
        bp.L = kBandL[ln.v];
        bp.submat = k.sub ? d.dtab : nullptr;
        bp.sub_k = k.sub ? (uint32_t)k.sub->K : 0;
        bp.free_ends = k.extend ? (uint32_t)k.xdrop : k.free_ends;
        bp.gap_open = sc->gap_open;
        bp.gap_extend = sc->gap_extend;
        SA_HIP(c, hipEventRecord(ev[0], st));
        if (kev) SA_HIP(c, hipEventRecord(kev[0], st));
        SA_HIP(c, fam.fill(algo, ln.v, mm, !k.notb, bp, st));
        if (kev) SA_HIP(c, hipEventRecord(kev[1], st));
        SA_HIP(c, hipEventRecord(ev[1], st));
        if (!k.notb) {
            SA_HIP(c, fam.walk(algo, d.use_lut, bp, st));
            c->tb_kernels++;
        }
        SA_HIP(c, hipEventRecord(ev[2], st));
        c->launches++;
    }
    c->nvar = 1;
    c->host_sel = -1;
    c->var_kernel[0] = SA_KERNEL_BANDED;
    c->var_R[0] = kBandR[grp.top_v];
    c->var_W[0] = 1;
    c->var_records[0] = k.notb ? SA_RECORDS_NONE : fam.records;
    return SA_OK;
}

// Outputs through the context's pinned staging, as the other host paths: [results][ops].
int banded_download(sa_ctx* c, const BandCall& k, const BandDevice& d, uint64_t ops_total) {
    hipStream_t st = c->stream;
    const uint32_t npairs = k.npairs;
    SA_HIP(c, c->ostage.alloc(d.b_res + ops_total));
    sa_result* const sres = reinterpret_cast<sa_result*>(c->ostage.data());
    uint8_t* const sops = c->ostage.data() + d.b_res;
    SA_HIP(c, hipMemcpyAsync(sres, d.dres, sizeof(sa_result) * (uint64_t)npairs, hipMemcpyDeviceToHost, st));
    if (!k.notb && ops_total) SA_HIP(c, hipMemcpyAsync(sops, d.dops, ops_total, hipMemcpyDeviceToHost, st));
    if (int rc = mark_last(c, st)) return rc;
    SA_HIP(c, hipStreamSynchronize(st));
    memcpy(k.results, sres, sizeof(sa_result) * (uint64_t)npairs);
    for (uint32_t p = 0; p < npairs && !k.notb; ++p) {
        const uint64_t o = k.off1[p] + k.off2[p] + p;
        memcpy(k.ops + o, sops + o, k.results[p].nops);
    }
    return SA_OK;
}

int banded_batch(sa_ctx* c, const BandCall& k) {
    int rc = banded_checks(c, k);
    if (rc) return rc;
    uint64_t ops_total = 0;
    if ((rc = banded_buffers(c, k, &ops_total))) return rc;
    if (!k.npairs) return SA_OK;
    SA_HIP(c, hipSetDevice(c->device));
    if ((rc = order_after_last(c, c->stream))) return rc;
    const BandFamily& fam = band_family(k.extend, k.seeded, k.ends_free, k.affine);
    BandGroups grp;
    if ((rc = banded_plan(c, k, fam, &grp))) return rc;
    BandDevice dev;
    if ((rc = banded_upload(c, k, grp, ops_total, &dev))) return rc;
    if ((rc = banded_launch(c, k, fam, grp, dev))) return rc;
    return banded_download(c, k, dev, ops_total);
}

// --------------------------------------------------------------------------- the entry points' bodies
// The descriptor of an align call and of a score call (no ops buffer), before the family's fields.
BandCall align_call(int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const uint8_t* seq2,
                    const uint64_t* off2, uint32_t npairs, const uint8_t* lut, uint32_t band, sa_result* results, uint8_t* ops,
                    uint64_t ops_cap) {
    return BandCall{algo, sc, seq1, off1, seq2, off2, npairs, lut, band, results, ops, ops_cap, false};
}
BandCall score_call(int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const uint8_t* seq2,
                    const uint64_t* off2, uint32_t npairs, const uint8_t* lut, uint32_t band, sa_result* results) {
    return BandCall{algo, sc, seq1, off1, seq2, off2, npairs, lut, band, results, nullptr, 0, true};
}

int banded_plain_batch(sa_ctx* c, BandCall k, bool affine) {
    k.rules = affine ? &kAffineRules : &kLinearRules;
    k.affine = affine;
    return banded_batch(c, k);
}

// The algorithm picks the band (NW's or GlobalGotoh's, whose rules make the remaining checks).
int banded_ends_free_batch(sa_ctx* c, BandCall k, uint32_t free_ends) {
    if (int rc = check_call(c, kEndsFreeRules, k.algo, k.sc, k.band, free_ends)) return rc;
    k.affine = k.algo == SA_GLOBAL_GOTOH;
    k.rules = k.affine ? &kAffineRules : &kLinearRules;
    k.ends_free = true;
    k.free_ends = free_ends;
    return banded_batch(c, k);
}

// The ends-free calls with every pair's band round its seed diagonal: their own checks (what the seed
// adds), then banded_batch, whose per-pair limits apply the legality rule.
int banded_seeded_batch(sa_ctx* c, BandCall k, const int32_t* diag, uint32_t free_ends) {
    if (int rc = check_call(c, kSeededRules, k.algo, k.sc, k.band, free_ends)) return rc;
    if (k.npairs && !diag) return fail(c, SA_ERR_ARG, "diag is NULL");
    if (k.off1 && k.off2) {
        for (uint32_t p = 0; p < k.npairs; ++p) {
            if (k.off1[p + 1] < k.off1[p] || k.off2[p + 1] < k.off2[p]) return fail(c, SA_ERR_ARG, "offsets must be non-decreasing");
            if (int rc = banded_seed_in_matrix(c, p, k.off1[p + 1] - k.off1[p], k.off2[p + 1] - k.off2[p], diag[p])) return rc;
        }
    }
    k.affine = k.algo == SA_GLOBAL_GOTOH;
    k.rules = k.affine ? &kAffineRules : &kLinearRules;
    k.ends_free = k.seeded = true;
    k.free_ends = free_ends;
    k.diag = diag;
    return banded_batch(c, k);
}

// The extension calls: their own checks, then banded_batch with the band round diagonal 0, whose per-pair
// limits apply SW's key limit in place of the legality rule.
int banded_extend_batch(sa_ctx* c, BandCall k, int32_t xdrop) {
    if (xdrop < SA_XDROP_OFF) return fail(c, SA_ERR_ARG, "xdrop must be SA_XDROP_OFF or >= 0");
    if (int rc = check_call(c, kExtendRules, k.algo, k.sc, k.band, 0)) return rc;
    k.affine = k.algo == SA_GLOBAL_GOTOH;
    k.rules = k.affine ? &kAffineRules : &kLinearRules;
    k.extend = true;
    k.xdrop = xdrop;
    return banded_batch(c, k);
}

// The symbol scan, codes and dense table of the matrix calls (sub_recode), then banded_batch (linear or
// affine by algorithm) with the kMatchSub fills.  The per-pair score bounds are the banded calls' own,
// with the table's extremes in place of match / mismatch -- for the affine algorithms the stricter
// |gap_open| + |gap_extend| form, which the sentinel argument of the affine band needs.
// (The table and buffer checks, and the scan that reads the sequences, come before the context's.)
int banded_matrix_batch(sa_ctx* c, BandCall k, const int16_t* submat) {
    int rc = check_call(c, kBandedMatrixRules, k.algo, k.sc, k.band, 0);
    if (rc) return rc;
    if (!submat) return fail(c, SA_ERR_ARG, "submat is NULL");
    if ((rc = check_batch_buffers(c, k.seq1, k.off1, k.seq2, k.off2, k.npairs, k.results, k.ops, k.notb))) return rc;
    SubRecode sub;
    if ((rc = sub_recode(c, k.seq1, k.off1[k.npairs], k.seq2, k.off2[k.npairs], submat, &sub))) return rc;
    const sa_scoring sc2 = sub_scoring(*k.sc, sub);   // what banded_pair_plan reads of the scoring
    k.sc = &sc2;
    k.affine = is_affine(k.algo);
    k.sub = &sub;
    return banded_batch(c, k);
}

// The answer of the three plan queries: one pair's variant and records.  (The scoring-dependent checks
// are the calls'; a permissive scoring stands in for them here.)
const sa_scoring kAnyScoring{0, 0, 0, 0, 0, 1};
int banded_plan_answer(int algo, bool affine, uint64_t m, uint64_t n, uint32_t band, const BandSeed* seed, int* cells_per_lane,
                       int* pairs_per_wave, uint64_t* ws_bytes_per_pair) {
    BandGeom g;
    int v = 0;
    if (int rc = banded_pair_plan(nullptr, algo, &kAnyScoring, m, n, band, &g, &v, seed)) return rc;
    if (cells_per_lane) *cells_per_lane = kBandR[v];
    if (pairs_per_wave) *pairs_per_wave = kWave / kBandL[v];
    if (ws_bytes_per_pair) *ws_bytes_per_pair = band_family(false, false, false, affine).rec_words(g, v) * 4;
    return SA_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------ C ABI
extern "C" {

int sa_align_batch_banded(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const uint8_t*
                          seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t band, sa_result*
                          results, uint8_t* ops, uint64_t ops_cap) {
    const BandCall k = align_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results, ops, ops_cap);
    return banded_plain_batch(c, k, false);
}
int sa_score_batch_banded(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const uint8_t*
                          seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t band, sa_result*
                          results) {
    return banded_plain_batch(c, score_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results), false);
}
int sa_align_batch_banded_affine(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t band,
                                 sa_result* results, uint8_t* ops, uint64_t ops_cap) {
    const BandCall k = align_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results, ops, ops_cap);
    return banded_plain_batch(c, k, true);
}
int sa_score_batch_banded_affine(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t band,
                                 sa_result* results) {
    return banded_plain_batch(c, score_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results), true);
}
int sa_align_batch_banded_ends_free(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                    uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t
                                    band, uint32_t free_ends, sa_result* results, uint8_t* ops, uint64_t ops_cap) {
    const BandCall k = align_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results, ops, ops_cap);
    return banded_ends_free_batch(c, k, free_ends);
}
int sa_score_batch_banded_ends_free(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                    uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t
                                    band, uint32_t free_ends, sa_result* results) {
    return banded_ends_free_batch(c, score_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results), free_ends);
}
int sa_align_batch_banded_seeded(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, const int32_t*
                                 diag, uint32_t band, uint32_t free_ends, sa_result* results, uint8_t* ops, uint64_t ops_cap) {
    const BandCall k = align_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results, ops, ops_cap);
    return banded_seeded_batch(c, k, diag, free_ends);
}
int sa_score_batch_banded_seeded(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, const int32_t*
                                 diag, uint32_t band, uint32_t free_ends, sa_result* results) {
    const BandCall k = score_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results);
    return banded_seeded_batch(c, k, diag, free_ends);
}
int sa_align_batch_banded_matrix(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const int16_t* submat, const uint8_t*
                                 match_lut, uint32_t band, sa_result* results, uint8_t* ops, uint64_t ops_cap) {
    const BandCall k = align_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results, ops, ops_cap);
    return banded_matrix_batch(c, k, submat);
}
int sa_score_batch_banded_matrix(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const int16_t* submat, const uint8_t*
                                 match_lut, uint32_t band, sa_result* results) {
    return banded_matrix_batch(c, score_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results), submat);
}

int sa_banded_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t band, uint32_t npairs, int* cells_per_lane,
                         int* pairs_per_wave, uint64_t* ws_bytes_per_pair) {
    (void)npairs;   // a pair's variant and records depend on its own shape only
    if (int rc = check_call(nullptr, kLinearRules, algo, &kAnyScoring, band, 0)) return rc;
    return banded_plan_answer(band_algo(algo), false, max_m, max_n, band, nullptr, cells_per_lane, pairs_per_wave, ws_bytes_per_pair);
}

int sa_banded_affine_plan_query(int algo, uint32_t max_m, uint32_t max_n, uint32_t band, uint32_t npairs, int* cells_per_lane,
                                int* pairs_per_wave, uint64_t* ws_bytes_per_pair) {
    (void)npairs;
    if (int rc = check_call(nullptr, kAffineRules, algo, &kAnyScoring, band, 0)) return rc;
    return banded_plan_answer(algo, true, max_m, max_n, band, nullptr, cells_per_lane, pairs_per_wave, ws_bytes_per_pair);
}

int sa_banded_seeded_plan_query(int algo, uint64_t m, uint64_t n, int32_t diag, uint32_t band, uint32_t free_ends,
                                int* cells_per_lane, int* pairs_per_wave, uint64_t* ws_bytes_per_pair) {
    int rc = check_call(nullptr, kSeededRules, algo, &kAnyScoring, band, free_ends);
    if (rc) return rc;
    if (m >= (1u << 24) || n >= (1u << 24)) return fail(nullptr, SA_ERR_UNSUPPORTED, "sequence length >= 2^24");
    if ((rc = banded_seed_in_matrix(nullptr, 0, m, n, diag))) return rc;
    const BandSeed sd{diag, free_ends, 0};
    return banded_plan_answer(band_algo(algo), algo == SA_GLOBAL_GOTOH, m, n, band, &sd, cells_per_lane, pairs_per_wave,
                              ws_bytes_per_pair);
}

int sa_align_batch_banded_extend(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t band,
                                 int32_t xdrop, sa_result* results, uint8_t* ops, uint64_t ops_cap) {
    const BandCall k = align_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results, ops, ops_cap);
    return banded_extend_batch(c, k, xdrop);
}
int sa_score_batch_banded_extend(sa_ctx* c, int algo, const sa_scoring* sc, const uint8_t* seq1, const uint64_t* off1, const
                                 uint8_t* seq2, const uint64_t* off2, uint32_t npairs, const uint8_t* match_lut, uint32_t band,
                                 int32_t xdrop, sa_result* results) {
    return banded_extend_batch(c, score_call(algo, sc, seq1, off1, seq2, off2, npairs, match_lut, band, results), xdrop);
}

int sa_banded_extend_plan_query(int algo, uint64_t m, uint64_t n, uint32_t band, int* cells_per_lane, int* pairs_per_wave,
                                uint64_t* ws_bytes_per_pair) {
    if (int rc = check_call(nullptr, kExtendRules, algo, &kAnyScoring, band, 0)) return rc;
    const BandSeed sd{0, 0, 0, true};
    return banded_plan_answer(band_algo(algo), algo == SA_GLOBAL_GOTOH, m, n, band, &sd, cells_per_lane, pairs_per_wave,
                              ws_bytes_per_pair);
}

}  // extern "C"
