// banded_emu.cpp — runs the banded fill and walk kernels' own source on the CPU, through the wave shim
// (tests/cpp/wave_emu/hip/hip_runtime.h), over buffers of exactly the size the host layer provisions.
// A stand-alone host program, linked against the twelve sa_banded*.hip units and sa_band_planner.hip, each
// compiled as C++ through the shim; tests/test_banded_emu.py builds it with the address and
// undefined-behaviour sanitizers, writes the cases and compares what comes back with the Python models.
//
//   banded_emu CASES OUT
//
// The path of a call is the host layer's (sa_api_banded.hip, sa_api_banded_device.hip): band_group /
// band_idx_with_diagonals give launch order, idx, recoff and the variant of every launch, the launchers are
// launch_banded_*_fill / _tb, and the device-planned form runs the planner's kernels.  What differs is the
// memory: every buffer a kernel receives is a heap allocation of its own of exactly the bytes the contract
// names -- no 256-byte rounding, no neighbour inside one workspace -- so a load or store a word outside it
// is a sanitizer report.  Every case runs twice with two poison patterns in records, results, ops and the
// plan blocks: the two runs must agree byte for byte in every result and in the ops each result counts,
// and a record word that still holds run A's poison in run A and run B's in run B was never written.
//
// The case file (one directive per line, `end` closes a case):
//   case NAME
//   family corridor|ends_free|seeded|extend|seeded_dev
//   algo A                     SA_SW 0, SA_NW 1, SA_LOCAL_GOTOH 2, SA_GLOBAL_GOTOH 3
//   scoring GAP MATCH MISMATCH ALLOW OPEN EXTEND
//   w W | xdrop X | free_ends BITS | merge 0|1 | simds N | budget WORDS | notb 0|1
//   lut HEX                    the 2048-word bit table (8 hex digits per word), absent: byte equality
//   submat K HEX               the matrix calls: K x K int16 entries (4 hex digits each); sequences hold codes
//   short_rec N                planted fault: the record buffer is N words short
//   walk_shift D               planted fault: the walk is told the variant D steps from the fill's
//   pair HEX1 HEX2 [DIAG]      `-` is the empty sequence
//   (seeded_dev) resident1 HEX, resident2 HEX, bounds MAX_M MAX_N, ops_bytes N, budget BYTES,
//                dpair START1 LEN1 START2 LEN2 DIAG OPSOFF
// The output: per case `case NAME`, `launch V FIRST COUNT` lines, `ws WORDS`, per pair
// `res P score end_i end_j start_i start_j nops flags reserved`, `ops P TEXT`, `rec P V WORDS UNWRITTEN`,
// then `tail CHANGED` (record words outside every pair's range that changed) and `poison SAME|DIFFER`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../seqalib_amd/csrc/sa_band_group.h"
#include "../../seqalib_amd/csrc/sa_band_plan.h"
#include "../../seqalib_amd/csrc/sa_internal.h"

using namespace sa;

namespace {

[[noreturn]] void fail(const std::string& what) {
    fprintf(stderr, "banded_emu: %s\n", what.c_str());
    exit(2);
}

// A buffer of exactly n elements of T, alone on the heap.
template <class T>
struct Exact {
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(static_cast<T*>(malloc(n_ * sizeof(T)))), n(n_) {
        if (!p) fail("out of memory");
    }
    Exact(const std::vector<T>& v) : Exact(v.size()) {
        if (n) memcpy(p, v.data(), n * sizeof(T));
    }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
    ~Exact() { free(p); }
    void fill_words(uint32_t word) {   // (every poisoned type is a whole number of 32-bit words, or bytes)
        uint8_t* b = reinterpret_cast<uint8_t*>(p);
        for (size_t k = 0; k < n * sizeof(T); ++k) b[k] = (uint8_t)(word >> (8 * (k & 3)));
    }
};

std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    if (s.size() % 2) fail("odd hex string");
    auto nib = [](char c) -> int { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
    for (size_t k = 0; k < s.size(); k += 2) {
        const int a = nib(s[k]), b = nib(s[k + 1]);
        if (a < 0 || b < 0) fail("bad hex digit");
        out.push_back((uint8_t)(a * 16 + b));
    }
    return out;
}

struct DevPair {
    uint64_t start1, start2, opsoff;
    uint32_t len1, len2;
    int32_t diag;
};

struct Case {
    std::string name, family = "corridor";
    int algo = SA_NW;
    int32_t gap = 0, match = 0, mismatch = 0, allow = 1, gap_open = 0, gap_extend = 0;
    int32_t w = 0, xdrop = SA_XDROP_OFF;
    uint32_t free_ends = 0;
    bool merge = true, notb = false;
    uint64_t simds = 1024, budget = 1ull << 40;
    std::vector<uint32_t> lut;        // 2048 words or empty
    uint32_t sub_k = 0;
    std::vector<int16_t> submat;
    uint64_t short_rec = 0;
    int walk_shift = 0;
    std::vector<std::vector<uint8_t>> s1, s2;
    std::vector<int32_t> diag;
    // seeded_dev
    std::vector<uint8_t> resident1, resident2;
    uint32_t max_m = 0, max_n = 0;
    uint64_t ops_bytes = 0;
    std::vector<DevPair> dpairs;
};

bool affine_algo(int algo) { return algo == SA_LOCAL_GOTOH || algo == SA_GLOBAL_GOTOH; }

// The launchers of a family, as kBandFamilies (sa_api_banded.hip) adapts them.
hipError_t family_fill(const Case& c, int v, int mm, bool rec, const BandAffineParams& p) {
    const bool aff = affine_algo(c.algo), lut = mm == kMatchLut;
    if (c.family == "corridor") return aff ? launch_banded_affine_fill(c.algo, v, mm, rec, p, nullptr) : launch_banded_fill(c.algo, v, mm, rec, p, nullptr);
    if (c.family == "ends_free") return aff ? launch_banded_affine_free_fill(v, lut, rec, p, nullptr) : launch_banded_free_fill(v, lut, rec, p, nullptr);
    if (c.family == "seeded") return aff ? launch_banded_affine_seeded_fill(v, lut, rec, p, nullptr) : launch_banded_seeded_fill(v, lut, rec, p, nullptr);
    if (c.family == "extend") return aff ? launch_banded_affine_extend_fill(v, lut, rec, p, nullptr) : launch_banded_extend_fill(v, lut, rec, p, nullptr);
    fail("unknown family " + c.family);
}
hipError_t family_walk(const Case& c, bool lut, const BandAffineParams& p) {
    const bool aff = affine_algo(c.algo);
    if (c.family == "corridor") return aff ? launch_banded_affine_tb(c.algo, lut, p, nullptr) : launch_banded_tb(c.algo, lut, p, nullptr);
    if (c.family == "ends_free") return aff ? launch_banded_affine_free_tb(lut, p, nullptr) : launch_banded_free_tb(lut, p, nullptr);
    if (c.family == "seeded") return aff ? launch_banded_affine_seeded_tb(lut, p, nullptr) : launch_banded_seeded_tb(lut, p, nullptr);
    if (c.family == "extend") return aff ? launch_banded_affine_extend_tb(lut, p, nullptr) : launch_banded_extend_tb(lut, p, nullptr);
    fail("unknown family " + c.family);
}

// What one run of a case leaves behind.
struct RunOut {
    std::vector<sa_result> res;
    std::vector<std::vector<uint8_t>> ops;      // per pair, the nops bytes its result counts
    std::vector<std::vector<uint32_t>> rec;     // per pair, its own record words after its launch's fill and walk
    std::vector<int> rec_v;                     // the variant that wrote them
    uint64_t tail_changed = 0;                  // record words outside every pair's range that lost the poison
    std::vector<uint8_t> opsbuf;                // seeded_dev: the whole ops buffer
    std::vector<std::string> plan;              // launch / list lines
    uint64_t ws_words = 0;
};

void scoring_params(const Case& c, BandAffineParams* bp) {
    bp->band = (uint32_t)c.w;
    bp->gap = c.gap;
    bp->match = c.match;
    bp->mismatch = c.allow ? c.mismatch : kBandNeg;
    bp->allow = c.allow;
    bp->gap_open = c.gap_open;
    bp->gap_extend = c.gap_extend;
}

// ------------------------------------------------------------------ the host-planned calls (sa_api_banded.hip)
void run_host(const Case& c, uint32_t poison, RunOut* out) {
    const uint32_t npairs = (uint32_t)c.s1.size();
    const bool aff = affine_algo(c.algo), seeded = c.family == "seeded", extend = c.family == "extend";
    std::vector<uint64_t> o1(npairs + 1, 0), o2(npairs + 1, 0);
    std::vector<uint8_t> b1, b2;
    for (uint32_t p = 0; p < npairs; ++p) {
        b1.insert(b1.end(), c.s1[p].begin(), c.s1[p].end());
        b2.insert(b2.end(), c.s2[p].begin(), c.s2[p].end());
        o1[p + 1] = b1.size();
        o2[p + 1] = b2.size();
    }
    // banded_plan
    const std::vector<int32_t> zero_diag(extend ? npairs : 0, 0);
    BandGroupIn in{o1.data(), o2.data(), npairs, extend ? zero_diag.data() : seeded ? c.diag.data() : nullptr, c.w,
                   aff ? kBandAffineVariants : kBandVariants, aff ? band_affine_rec_words : band_rec_words, c.notb,
                   c.notb ? 0 : c.budget, c.simds, c.merge};
    BandGroups grp;
    if (!band_group(in, &grp)) fail(c.name + ": the records of one pair exceed the budget");
    std::vector<uint64_t> words(grp.idx.size(), 0);   // per entry of idx, before the diagonals join it
    std::vector<int> entry_v(grp.idx.size(), 0);
    for (const BandLaunch& ln : grp.launches)
        for (uint32_t k = 0; k < ln.count; ++k) {
            const uint32_t e = ln.first + k;
            entry_v[e] = ln.v;
            if (!c.notb) words[e] = in.rec_words(band_group_geom(in, grp.idx[e]), ln.v);
        }
    const std::vector<uint32_t> pair_of = grp.idx;
    if (seeded) grp.idx = band_idx_with_diagonals(grp, c.diag.data());
    out->ws_words = grp.ws_words;
    for (const BandLaunch& ln : grp.launches) {
        char line[96];
        snprintf(line, sizeof(line), "launch %d %u %u", ln.v, ln.first, ln.count);
        out->plan.push_back(line);
    }

    // banded_upload: one allocation per array, of the bytes the call's contract names
    const uint64_t ops_total = c.notb ? 0 : o1[npairs] + o2[npairs] + npairs;
    Exact<uint8_t> d1(b1), d2(b2);
    Exact<uint64_t> do1(o1), do2(o2), dro(grp.recoff);
    Exact<uint32_t> didx(grp.idx), dbits(c.lut);
    Exact<int16_t> dtab(c.submat);
    Exact<sa_result> dres(npairs);
    Exact<uint8_t> dops(ops_total);
    if (c.short_rec > grp.ws_words) fail("short_rec above the workspace");
    Exact<uint32_t> ws(c.notb ? 0 : grp.ws_words - c.short_rec);
    dres.fill_words(poison);
    dops.fill_words(poison);

    out->res.assign(npairs, sa_result{});
    out->ops.assign(npairs, {});
    out->rec.assign(npairs, {});
    out->rec_v.assign(npairs, -1);
    const bool use_lut = !c.lut.empty();
    const int mm = c.sub_k ? kMatchSub : use_lut ? kMatchLut : kMatchEq;
    const uint32_t idx_stride = seeded ? 2 : 1;
    for (const BandLaunch& ln : grp.launches) {
        ws.fill_words(poison);
        BandAffineParams bp;
        bp.seq1 = d1.p;
        bp.off1 = do1.p;
        bp.seq2 = d2.p;
        bp.off2 = do2.p;
        bp.lutbits = use_lut ? dbits.p : nullptr;
        bp.idx = didx.p + (uint64_t)idx_stride * ln.first;
        bp.recoff = dro.p + ln.first;
        bp.rec = c.notb ? nullptr : ws.p;
        bp.res = dres.p;
        bp.ops = c.notb ? nullptr : dops.p;
        bp.count = ln.count;
        scoring_params(c, &bp);
        bp.R = kBandR[ln.v];
        bp.L = kBandL[ln.v];
        bp.submat = c.sub_k ? dtab.p : nullptr;
        bp.sub_k = c.sub_k;
        bp.free_ends = extend ? (uint32_t)c.xdrop : c.free_ends;
        if (family_fill(c, ln.v, mm, !c.notb, bp) != hipSuccess) fail(c.name + ": the fill launcher refused");
        if (!c.notb) {
            if (c.walk_shift) {
                bp.R = kBandR[ln.v + c.walk_shift];
                bp.L = kBandL[ln.v + c.walk_shift];
            }
            if (family_walk(c, use_lut, bp) != hipSuccess) fail(c.name + ": the walk launcher refused");
            uint64_t used = 0;
            for (uint32_t k = 0; k < ln.count; ++k) {
                const uint32_t e = ln.first + k, p = pair_of[e];
                if (grp.recoff[e] != used) fail(c.name + ": record ranges are not back to back");
                const uint64_t have = ws.n > used ? std::min<uint64_t>(words[e], ws.n - used) : 0;
                out->rec[p].assign(ws.p + used, ws.p + used + have);
                out->rec_v[p] = ln.v;
                used += words[e];
            }
            for (uint64_t x = used; x < ws.n; ++x) out->tail_changed += ws.p[x] != poison;
        }
    }
    for (uint32_t p = 0; p < npairs; ++p) {
        out->res[p] = dres.p[p];
        if (c.notb) continue;
        const uint64_t o = o1[p] + o2[p] + p, cap = o1[p + 1] - o1[p] + o2[p + 1] - o2[p] + 1;
        const uint64_t nops = std::min<uint64_t>(out->res[p].nops, cap);
        out->ops[p].assign(dops.p + o, dops.p + o + nops);
    }
}

// --------------------------------------------------- the device-planned seeded calls (sa_api_banded_device.hip)
void run_device(const Case& c, uint32_t poison, RunOut* out) {
    const uint32_t npairs = (uint32_t)c.dpairs.size();
    const bool aff = affine_algo(c.algo);
    const BandPlanBound bound = band_plan_bound_seeded((int32_t)c.max_m, (int32_t)c.max_n, c.w, aff);
    if (bound.vmax < 0) fail(c.name + ": the bound shape's band is too wide");
    const uint64_t rec_words = c.notb ? 0 : bound.rec_words;
    const uint64_t fixed = 4ull * kBandPlanHeadWords + 512;
    const uint32_t per = c.budget > fixed ? band_plan_chunk_pairs(rec_words + kBandPlanWords, c.budget - fixed, npairs) : 0;
    if (!per) fail(c.name + ": one pair's bound exceeds the budget");
    out->ws_words = rec_words * per;

    std::vector<uint64_t> st1, st2, oo;
    std::vector<uint32_t> l1, l2;
    std::vector<int32_t> dg;
    for (const DevPair& d : c.dpairs) {
        st1.push_back(d.start1);
        st2.push_back(d.start2);
        oo.push_back(d.opsoff);
        l1.push_back(d.len1);
        l2.push_back(d.len2);
        dg.push_back(d.diag);
    }
    Exact<uint8_t> r1(c.resident1), r2(c.resident2);
    Exact<uint64_t> dst1(st1), dst2(st2), doo(oo);
    Exact<uint32_t> dl1(l1), dl2(l2), dbits(c.lut);
    Exact<int32_t> ddg(dg);
    Exact<sa_result> dres(npairs);
    Exact<uint8_t> dops(c.notb ? 0 : c.ops_bytes);
    Exact<uint32_t> head(kBandPlanHeadWords), lists(per), recs(rec_words * per - std::min<uint64_t>(c.short_rec, rec_words * per));
    Exact<BandPlanRec> plans(per);
    dres.fill_words(poison);
    dops.fill_words(poison);
    out->res.assign(npairs, sa_result{});
    out->ops.assign(npairs, {});
    out->rec.assign(npairs, {});
    out->rec_v.assign(npairs, -1);
    const bool use_lut = !c.lut.empty();
    for (uint32_t first = 0; first < npairs; first += per) {
        const uint32_t count = std::min(per, npairs - first);
        head.fill_words(poison);
        lists.fill_words(poison);
        recs.fill_words(poison);
        plans.fill_words(poison);
        BandPlannerParams pp;
        pp.seq1 = r1.p;
        pp.seq1_bytes = r1.n;
        pp.start1 = dst1.p;
        pp.len1 = dl1.p;
        pp.seq2 = r2.p;
        pp.seq2_bytes = r2.n;
        pp.start2 = dst2.p;
        pp.len2 = dl2.p;
        pp.diag = ddg.p;
        pp.ops_off = c.notb ? nullptr : doo.p;
        pp.ops_bytes = c.ops_bytes;
        pp.res = dres.p;
        pp.first = first;
        pp.count = count;
        pp.max_m = c.max_m;
        pp.max_n = c.max_n;
        pp.w = c.w;
        pp.free_ends = c.free_ends;
        pp.affine = aff;
        pp.vmax = bound.vmax;
        pp.span = bound.span;
        pp.bound_words = rec_words;
        pp.head = head.p;
        pp.plans = plans.p;
        pp.lists = lists.p;
        BandAffineParams bp;
        bp.seq1 = r1.p;
        bp.off1 = reinterpret_cast<const uint64_t*>(plans.p);
        bp.seq2 = r2.p;
        bp.off2 = nullptr;
        bp.lutbits = use_lut ? dbits.p : nullptr;
        bp.idx = lists.p;
        bp.recoff = nullptr;
        bp.rec = c.notb ? nullptr : recs.p;
        bp.res = dres.p;
        bp.ops = c.notb ? nullptr : dops.p;
        bp.count = count;
        scoring_params(c, &bp);
        bp.R = 0;
        bp.L = 0;
        bp.submat = nullptr;
        bp.sub_k = 0;
        bp.free_ends = c.free_ends;
        if (launch_band_planner(pp, nullptr) != hipSuccess) fail(c.name + ": the planner refused");
        for (int v = 0; v <= bound.vmax; ++v) {
            bp.off2 = reinterpret_cast<const uint64_t*>(head.p + kBandPlanHeadLists + 2 * v);
            const hipError_t e = aff ? launch_banded_affine_seeded_dev_fill(v, use_lut, !c.notb, bp, nullptr)
                                     : launch_banded_seeded_dev_fill(v, use_lut, !c.notb, bp, nullptr);
            if (e != hipSuccess) fail(c.name + ": the fill launcher refused");
        }
        if (!c.notb) {
            const hipError_t e = aff ? launch_banded_affine_seeded_dev_tb(use_lut, bp, nullptr) : launch_banded_seeded_dev_tb(use_lut, bp, nullptr);
            if (e != hipSuccess) fail(c.name + ": the walk launcher refused");
        }
        // the chunk's plan: per variant its list, sorted (the order inside a bucket is the atomics')
        for (int v = 0; v <= bound.vmax; ++v) {
            const uint32_t lf = head.p[kBandPlanHeadLists + 2 * v], lc = head.p[kBandPlanHeadLists + 2 * v + 1];
            if ((uint64_t)lf + lc > count) fail(c.name + ": a list leaves the chunk");
            std::vector<uint32_t> members(lists.p + lf, lists.p + lf + lc);
            std::sort(members.begin(), members.end());
            std::ostringstream line;
            line << "list " << first << " " << v << " " << lc;
            for (uint32_t q : members) line << " " << plans.p[q].pair;
            out->plan.push_back(line.str());
        }
        for (uint32_t q = 0; q < count && !c.notb; ++q) {
            const BandPlanRec& pr = plans.p[q];
            uint64_t own = 0;
            if (pr.v >= 0) {
                own = band_plan_pair(pr.m, pr.n, c.w, pr.diag, aff, bound.span).rec_words;
                if (own > rec_words) fail(c.name + ": a pair's records exceed the bound's");
                out->rec_v[first + q] = pr.v;
            }
            const uint64_t base = (uint64_t)q * rec_words;
            for (uint64_t x = 0; x < rec_words && base + x < recs.n; ++x) {
                if (x < own) out->rec[first + q].push_back(recs.p[base + x]);
                else out->tail_changed += recs.p[base + x] != poison;
            }
        }
        for (uint64_t x = (uint64_t)count * rec_words; x < recs.n; ++x) out->tail_changed += recs.p[x] != poison;
    }
    for (uint32_t p = 0; p < npairs; ++p) {
        out->res[p] = dres.p[p];
        if (c.notb) continue;
        const uint64_t nops = out->res[p].nops;
        if (nops && (c.dpairs[p].opsoff > dops.n || nops > dops.n - c.dpairs[p].opsoff)) fail(c.name + ": nops leaves the ops buffer");
        out->ops[p].assign(dops.p + c.dpairs[p].opsoff, dops.p + c.dpairs[p].opsoff + nops);
    }
    out->opsbuf.assign(dops.p, dops.p + dops.n);
}

constexpr uint32_t kPoisonA = 0xa5c3a5c3u, kPoisonB = 0x3c5a3c5au;

void run_case(const Case& c, FILE* f) {
    RunOut a, b;
    const bool dev = c.family == "seeded_dev";
    if (dev) {
        run_device(c, kPoisonA, &a);
        run_device(c, kPoisonB, &b);
    } else {
        run_host(c, kPoisonA, &a);
        run_host(c, kPoisonB, &b);
    }
    fprintf(f, "case %s\n", c.name.c_str());
    for (const std::string& s : a.plan) fprintf(f, "%s\n", s.c_str());
    fprintf(f, "ws %llu\n", (unsigned long long)a.ws_words);
    bool same = a.plan == b.plan && a.ws_words == b.ws_words;
    const size_t npairs = a.res.size();
    for (size_t p = 0; p < npairs; ++p) {
        const sa_result& r = a.res[p];
        fprintf(f, "res %zu %d %d %d %d %d %u %u %u\n", p, r.score, r.end_i, r.end_j, r.start_i, r.start_j, r.nops, r.flags, r.reserved);
        same = same && memcmp(&a.res[p], &b.res[p], sizeof(sa_result)) == 0 && a.ops[p] == b.ops[p];
        if (c.notb) continue;
        fprintf(f, "ops %zu %s\n", p, a.ops[p].empty() ? "-" : std::string(a.ops[p].begin(), a.ops[p].end()).c_str());
        uint64_t unwritten = 0;
        for (size_t x = 0; x < a.rec[p].size() && x < b.rec[p].size(); ++x) unwritten += a.rec[p][x] == kPoisonA && b.rec[p][x] == kPoisonB;
        fprintf(f, "rec %zu %d %zu %llu\n", p, a.rec_v[p], a.rec[p].size(), (unsigned long long)unwritten);
    }
    if (dev && !c.notb) {   // the ops buffer's bytes no result counts must be untouched: poison where both runs left it
        std::string mask(a.opsbuf.size(), '0');
        for (size_t x = 0; x < a.opsbuf.size(); ++x) {
            const uint8_t pa = (uint8_t)(kPoisonA >> (8 * (x & 3))), pb = (uint8_t)(kPoisonB >> (8 * (x & 3)));
            if (!(a.opsbuf[x] == pa && b.opsbuf[x] == pb)) mask[x] = '1';
        }
        fprintf(f, "opsmask %s\n", mask.empty() ? "-" : mask.c_str());
    }
    fprintf(f, "tail %llu\n", (unsigned long long)(a.tail_changed + b.tail_changed));
    fprintf(f, "poison %s\n", same ? "SAME" : "DIFFER");
    fprintf(f, "end\n");
    fflush(f);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) fail("usage: banded_emu CASES OUT");
    std::ifstream in(argv[1]);
    if (!in) fail("cannot read the case file");
    FILE* f = fopen(argv[2], "w");
    if (!f) fail("cannot write the output file");
    Case c;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string key;
        if (!(ss >> key)) continue;
        if (key == "case") {
            c = Case{};
            ss >> c.name;
        } else if (key == "family") ss >> c.family;
        else if (key == "algo") ss >> c.algo;
        else if (key == "scoring") ss >> c.gap >> c.match >> c.mismatch >> c.allow >> c.gap_open >> c.gap_extend;
        else if (key == "w") ss >> c.w;
        else if (key == "xdrop") ss >> c.xdrop;
        else if (key == "free_ends") ss >> c.free_ends;
        else if (key == "merge") ss >> c.merge;
        else if (key == "notb") ss >> c.notb;
        else if (key == "simds") ss >> c.simds;
        else if (key == "budget") ss >> c.budget;
        else if (key == "short_rec") ss >> c.short_rec;
        else if (key == "walk_shift") ss >> c.walk_shift;
        else if (key == "bounds") ss >> c.max_m >> c.max_n;
        else if (key == "ops_bytes") ss >> c.ops_bytes;
        else if (key == "lut") {
            std::string h;
            ss >> h;
            const std::vector<uint8_t> raw = unhex(h);
            if (raw.size() != 8192) fail("lut: 2048 words expected");
            c.lut.resize(2048);
            for (int k = 0; k < 2048; ++k) c.lut[k] = (uint32_t)raw[4 * k] << 24 | (uint32_t)raw[4 * k + 1] << 16 | (uint32_t)raw[4 * k + 2] << 8 | raw[4 * k + 3];
        } else if (key == "submat") {
            std::string h;
            ss >> c.sub_k >> h;
            const std::vector<uint8_t> raw = unhex(h);
            if (raw.size() != 2ull * c.sub_k * c.sub_k) fail("submat: K * K entries expected");
            // (the host pads the dense table to a whole 32-bit word: the fill copies words)
            c.submat.assign((c.sub_k * c.sub_k + 1) / 2 * 2, 0);
            for (uint32_t k = 0; k < c.sub_k * c.sub_k; ++k) c.submat[k] = (int16_t)((uint16_t)raw[2 * k] << 8 | raw[2 * k + 1]);
        } else if (key == "pair") {
            std::string h1, h2;
            int32_t d = 0;
            ss >> h1 >> h2;
            ss >> d;
            c.s1.push_back(unhex(h1));
            c.s2.push_back(unhex(h2));
            c.diag.push_back(d);
        } else if (key == "resident1" || key == "resident2") {
            std::string h;
            ss >> h;
            (key == "resident1" ? c.resident1 : c.resident2) = unhex(h);
        } else if (key == "dpair") {
            DevPair d{};
            ss >> d.start1 >> d.len1 >> d.start2 >> d.len2 >> d.diag >> d.opsoff;
            c.dpairs.push_back(d);
        } else if (key == "end") {
            run_case(c, f);
        } else fail("unknown directive " + key);
    }
    fclose(f);
    return 0;
}
