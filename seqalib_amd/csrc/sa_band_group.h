// sa_band_group.h — how a banded call's pairs become launches (sa_api_banded.hip).  Pure host code: no
// context, no HIP call, no environment; tests/cpp/band_group_test.cpp runs it on a CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sa_internal.h"

namespace sa {

struct BandLaunch {
    int v;                   // the fill variant (kBandR[v], kBandL[v])
    uint32_t first, count;   // its pairs: idx[first .. first + count)
};

struct BandGroupIn {
    const uint64_t* off1;    // the pairs' lengths, as the calls' offsets: m = off1[p + 1] - off1[p]
    const uint64_t* off2;
    uint32_t npairs;
    const int32_t* diag;     // the seeded calls' seed diagonals, else NULL (the corridor band)
    int32_t w;               // the half-width, clamped to kBandMaxW
    int nvariants;           // kBandVariants or kBandAffineVariants; every pair's band fits one of them
    uint64_t (*rec_words)(const BandGeom&, int);
    bool notb;               // a score call: no records
    uint64_t budget_words;   // record words one launch may hold
    uint64_t simds;          // of the device
    bool merge;              // $SEQALIB_BAND_MERGE != 0
};

struct BandGroups {
    std::vector<BandLaunch> launches;
    std::vector<uint32_t> idx;      // launch by launch, the pairs of each longest (m + n) first
    std::vector<uint64_t> recoff;   // per entry of idx: the word offset of its records in its launch
    uint64_t ws_words = 0;          // the largest launch's records
    int top_v = 0;                  // the widest variant in use
    uint64_t too_big_words = 0;     // band_group() == false: one pair's records, larger than the budget
};

inline BandGeom band_group_geom(const BandGroupIn& in, uint32_t p) {
    const int32_t m = (int32_t)(in.off1[p + 1] - in.off1[p]), n = (int32_t)(in.off2[p + 1] - in.off2[p]);
    return in.diag ? band_geom_seeded(m, n, in.w, in.diag[p]) : band_geom(m, n, in.w);
}

// Every pair gets the narrowest variant its clipped band fits; the pairs of one variant are launched
// together, longest first, in as many launches as the budget leaves room for their records (record
// offsets restart at every launch).
// A launch of fewer waves than the device has SIMDs runs as long as one wave does, so two such
// launches in a row cost two of those where one launch of both costs one.  The pairs of a variant
// therefore join the NEXT variant (one step in (R, L): twice the diagonals, at most twice the
// records) when that variant is in use too, the joint launch still has at most a wave per SIMD,
// and every moved pair's records still fit the workspace budget; a pair moves at most one step
// (a variant that took pairs in stays where it is).  So a pair's records stay within twice what
// sa_banded_plan_query reports, and a call that fits the limit unmerged never fails merged.
// merge off: every pair keeps the narrowest variant that holds it (tests).
// false: the records of one pair exceed the budget (out->too_big_words).
inline bool band_group(const BandGroupIn& in, BandGroups* out) {
    std::vector<uint64_t> words(in.npairs, 0);
    std::vector<uint32_t> bucket[kBandVariants];
    for (uint32_t p = 0; p < in.npairs; ++p) {
        const BandGeom g = band_group_geom(in, p);
        const int v = band_variant(g.beff);
        if (!in.notb) words[p] = in.rec_words(g, v);
        bucket[v].push_back(p);
    }
    if (in.merge) {
        bool took_in = false;   // bucket[v] holds pairs moved up from v - 1
        for (int v = 0; v + 1 < in.nvariants; ++v) {
            const bool fixed = took_in;
            took_in = false;
            if (fixed || bucket[v].empty() || bucket[v + 1].empty()) continue;
            const uint64_t ppw = (uint64_t)(kWave / kBandL[v + 1]);
            if ((bucket[v].size() + bucket[v + 1].size() + ppw - 1) / ppw > in.simds) continue;
            std::vector<uint64_t> moved(bucket[v].size(), 0);
            bool fits = true;
            for (size_t k = 0; k < bucket[v].size() && !in.notb && fits; ++k) {
                moved[k] = in.rec_words(band_group_geom(in, bucket[v][k]), v + 1);
                fits = moved[k] <= in.budget_words;
            }
            if (!fits) continue;
            for (size_t k = 0; k < bucket[v].size(); ++k) {
                words[bucket[v][k]] = moved[k];
                bucket[v + 1].push_back(bucket[v][k]);
            }
            bucket[v].clear();
            took_in = true;
        }
    }
    out->idx.reserve(in.npairs);
    out->recoff.reserve(in.npairs);
    for (int v = 0; v < in.nvariants; ++v) {
        std::vector<uint32_t>& b = bucket[v];
        if (b.empty()) continue;
        out->top_v = v;
        std::stable_sort(b.begin(), b.end(), [&](uint32_t x, uint32_t y) {
            return in.off1[x + 1] - in.off1[x] + in.off2[x + 1] - in.off2[x] > in.off1[y + 1] - in.off1[y] + in.off2[y + 1] - in.off2[y];
        });
        BandLaunch cur{v, (uint32_t)out->idx.size(), 0};
        uint64_t used = 0;
        for (uint32_t p : b) {
            if (words[p] > in.budget_words) {   // (a score call's words are 0)
                out->too_big_words = words[p];
                return false;
            }
            if (cur.count && used + words[p] > in.budget_words) {
                out->launches.push_back(cur);
                cur = BandLaunch{v, (uint32_t)out->idx.size(), 0};
                used = 0;
            }
            out->idx.push_back(p);
            out->recoff.push_back(used);
            used += words[p];
            cur.count++;
            out->ws_words = std::max(out->ws_words, used);
        }
        out->launches.push_back(cur);
    }
    return true;
}

// The seeded calls' uploaded index array: each launch's block is [its idx entries][their diagonals]
// (sa_internal.h kBandSeeded), so launch ln's block starts at 2 * ln.first.
inline std::vector<uint32_t> band_idx_with_diagonals(const BandGroups& g, const int32_t* diag) {
    std::vector<uint32_t> both;
    both.reserve(2 * g.idx.size());
    for (const BandLaunch& ln : g.launches) {
        both.insert(both.end(), g.idx.begin() + ln.first, g.idx.begin() + ln.first + ln.count);
        for (uint32_t k = 0; k < ln.count; ++k) both.push_back((uint32_t)diag[g.idx[ln.first + k]]);
    }
    return both;
}

}  // namespace sa
