// sa_band_plan.h — what a device-resident form of the banded extension calls has to plan per pair on the
// device, and what the host can provision for it without reading a length.  __host__ __device__, so that a
// planner kernel and a CPU test (tests/cpp/band_plan_test.cpp) run the same code.  No call uses it yet:
// the device-resident calls themselves are not in the tree.
//
// The host knows the bound shape (max_m, max_n), the half-width w and the algorithm; the device knows every
// pair's lengths.  For the band round a diagonal k, clipped to the matrix (band_geom_seeded):
//   B'(m, n) = min(k + w, n) - max(k - w, -m) + 1 does not fall when m or n grows, so a pair inside the
//   bounds takes a variant no wider than the bound shape's (band_variant is monotone in B');
//   the steps a pair records, tend - tb + 1, are at most last + 2 with last = min(m + n, 2m + hi', 2n - lo')
//   (tend = last - lo', and -lo' - tb <= 1 whether the band straddles diagonal 0 or not), and for k = 0
//   last = min(m + n, 2m + min(w, n), 2n + min(w, m)) does not fall when m or n grows either;
//   a variant's record words do not fall when the steps grow, nor, for the same steps, from one variant to
//   the next (S halves or L doubles at every step of the list).
// So the record words of the bound shape's variant over last(max_m, max_n) + 2 steps bound every pair's.
#pragma once
#include "sa_internal.h"

namespace sa {

// Sweep-length buckets per variant: a variant's pairs are listed longest bucket first, so the pairs of a
// wave finish within 1 / kBandPlanBuckets of the bound shape's sweep of each other.
constexpr int kBandPlanBuckets = 64;
constexpr int kBandPlanKeys = kBandVariants * kBandPlanBuckets;
constexpr uint32_t kBandPlanNoKey = 0xffffffffu;   // a pair outside the bounds: SA_FLAG_BAD_SHAPE, in no list

__host__ __device__ inline uint64_t band_plan_rec_words(bool affine, const BandGeom& g, int v) {
    return affine ? band_affine_rec_words(g, v) : band_rec_words(g, v);
}

// What the host provisions from the bound shape (the band round diagonal 0).
struct BandPlanBound {
    int vmax;             // the widest variant a pair inside the bounds can take (-1: the band is too wide)
    int32_t span;         // every such pair's sweep length tend - tb is below it
    uint64_t rec_words;   // every such pair's record words are at most this
};
__host__ __device__ inline BandPlanBound band_plan_bound(int32_t max_m, int32_t max_n, int32_t w, bool affine) {
    const BandGeom g = band_geom_seeded(max_m, max_n, w, 0);
    BandPlanBound b;
    b.vmax = affine ? band_affine_variant(g.beff) : band_variant(g.beff);
    b.span = g.tend + g.lo + 2;   // last + 2
    const BandGeom steps{g.lo, g.hi, g.beff, 0, b.span - 1};
    b.rec_words = b.vmax < 0 ? 0 : band_plan_rec_words(affine, steps, b.vmax);
    return b;
}

// One pair: its geometry round diagonal `diag`, the fill variant the host layer picks for it (-1: none),
// its list key -- variant-major, longest sweep bucket first -- and its record words.
struct BandPlanPair {
    BandGeom g;
    int v;
    uint32_t key;
    uint64_t rec_words;
};
__host__ __device__ inline BandPlanPair band_plan_pair(int32_t m, int32_t n, int32_t w, int32_t diag, bool affine, int32_t span) {
    BandPlanPair p;
    p.g = band_geom_seeded(m, n, w, diag);
    p.v = affine ? band_affine_variant(p.g.beff) : band_variant(p.g.beff);
    p.key = kBandPlanNoKey;
    p.rec_words = 0;
    if (p.v < 0) return p;
    const int64_t sweep = (int64_t)p.g.tend - p.g.tb;
    int64_t bucket = span > 0 ? sweep * kBandPlanBuckets / span : 0;
    if (bucket < 0) bucket = 0;
    if (bucket > kBandPlanBuckets - 1) bucket = kBandPlanBuckets - 1;
    p.key = (uint32_t)(p.v * kBandPlanBuckets + (kBandPlanBuckets - 1 - (int)bucket));
    p.rec_words = band_plan_rec_words(affine, p.g, p.v);
    return p;
}

// The pairs of one chunk: as many as the budget holds records of the bound for.  0: one pair's bound
// exceeds the budget.  (A score call stores no records: bound_words = 0, one chunk.)
inline uint32_t band_plan_chunk_pairs(uint64_t bound_words, uint64_t budget_bytes, uint32_t npairs) {
    if (!bound_words) return npairs;
    const uint64_t fit = budget_bytes / 4 / bound_words;
    return (uint32_t)(fit < npairs ? fit : npairs);
}

}  // namespace sa
