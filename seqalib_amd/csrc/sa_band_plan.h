// sa_band_plan.h — what a device-resident form of a banded call has to plan per pair on the device, and
// what the host can provision for it without reading a length.  __host__ __device__, so that a planner
// kernel and the CPU tests (tests/cpp/band_plan_test.cpp, tests/cpp/band_plan_seeded_test.cpp) run the same
// code.  The device-resident seeded calls (sa_*_batch_banded_seeded_device: sa_band_planner.hip,
// sa_api_banded_device.hip) use band_plan_pair, band_plan_bound_seeded, band_seed_legality and
// band_plan_chunk_pairs; band_plan_bound (diagonal 0: the extension band) has no caller yet, the
// device-resident extension calls are not in the tree.
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
//
// Any seed diagonal (band_plan_bound_seeded).  The host does not know k either, so the bound must hold for
// every -m <= k <= n:
//   B' <= 2w + 1 (k + w - (k - w) + 1) and B' <= m + n + 1 (n - (-m) + 1), so the variant is at most that of
//   min(2w + 1, max_m + max_n + 1) diagonals;
//   steps = tend - tb + 1 = last - lo' - tb + 1 <= min(m + n, 2m + 2w, 2n + 2w) + 2, by the band's position:
//     lo' <= 0 <= hi' (it straddles diagonal 0): tb >= -lo' - 1, so steps <= last + 2; lo' <= 0 means
//       k <= w, so hi' <= 2w and last <= 2m + hi' <= 2m + 2w; hi' >= 0 means k >= -w, so -lo' <= 2w and
//       last <= 2n - lo' <= 2n + 2w; and last <= m + n;
//     lo' > 0 (it begins on row 0): tb = 0, steps = last - lo' + 1, and last - lo' is at most
//       2m + hi' - lo' <= 2m + 2w, at most 2n - 2 lo' < 2n, and below m + n;
//     hi' < 0 (it begins on column 0): tb >= -lo' - hi' - 1, so steps <= last + hi' + 2, and last + hi' is at
//       most 2m + 2 hi' < 2m, at most 2n - lo' + hi' <= 2n + 2w, and below m + n;
//   and that bound does not fall when m or n grows.
// So the record words of that variant over min(M + N, 2M + 2w, 2N + 2w) + 2 steps bound every pair's, by the
// two monotonicities of the record words above.  tests/cpp/band_plan_seeded_test.cpp checks it by brute force.
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

// The same for the seeded band: every pair with m <= max_m, n <= max_n and any seed diagonal (the argument
// is at the head of this file).  span: every such pair's steps tend - tb + 1 are at most it.
__host__ __device__ inline BandPlanBound band_plan_bound_seeded(int32_t max_m, int32_t max_n, int32_t w, bool affine) {
    const int64_t M = max_m, N = max_n, W = w;
    int64_t beff = 2 * W + 1;
    if (M + N + 1 < beff) beff = M + N + 1;
    int64_t steps = M + N;
    if (2 * M + 2 * W < steps) steps = 2 * M + 2 * W;
    if (2 * N + 2 * W < steps) steps = 2 * N + 2 * W;
    steps += 2;
    BandPlanBound b;
    b.vmax = beff > kBandMaxDiagonals ? -1 : affine ? band_affine_variant((int32_t)beff) : band_variant((int32_t)beff);
    b.span = (int32_t)steps;
    const BandGeom g{0, 0, (int32_t)beff, 0, b.span - 1};
    b.rec_words = b.vmax < 0 ? 0 : band_plan_rec_words(affine, g, b.vmax);
    return b;
}

// The seeded calls' legality rule (include/seqalib_hip.h): the band must hold a legal begin -- (0, 0), or a
// cell of row 0 / column 0 whose begin is free -- and a legal end -- (m, n), or a cell of the last row / column
// whose end is free.  Bit 0: a legal begin exists, bit 1: a legal end; kBandSeedLegal: the pair is taken.
constexpr int kBandSeedLegal = 3;
__host__ __device__ inline int band_seed_legality(const BandGeom& g, int64_t m, int64_t n, uint32_t free_ends) {
    const bool begin = (g.lo <= 0 && 0 <= g.hi) || ((free_ends & kFreeSeq2Begin) && g.hi >= 0) ||
                       ((free_ends & kFreeSeq1Begin) && g.lo <= 0);
    const int64_t d = n - m;
    const bool end = (g.lo <= d && d <= g.hi) || ((free_ends & kFreeSeq2End) && g.lo <= d) ||
                     ((free_ends & kFreeSeq1End) && g.hi >= d);
    return (begin ? 1 : 0) | (end ? 2 : 0);
}

// The plan record of one pair of a device-planned call, written by the planner (sa_band_planner.hip) and read
// by the planned fills and walks in place of off1 / off2 / idx / recoff.  v < 0: the pair is not run (its
// result holds its flag already).
struct BandPlanRec {
    const uint8_t* s1;   // the two slices
    const uint8_t* s2;
    uint64_t recoff;     // word offset of the pair's records: its slot in the chunk x the bound's words
    uint64_t opsoff;     // byte offset of its ops
    int32_t m, n, diag, v;
    uint32_t pair;       // its index in the call (results)
    uint32_t key;        // its list key (band_plan_pair), kBandPlanNoKey when v < 0
    uint32_t pad[2];
};
static_assert(sizeof(BandPlanRec) == 64, "sixteen words per pair");
// 32-bit words of plan per pair: the record and the pair's entry in its variant's list.
constexpr uint64_t kBandPlanWords = sizeof(BandPlanRec) / 4 + 1;

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

// The planner of one chunk (sa_band_planner.hip).  head: kBandPlanHeadWords words of the workspace -- the key
// counters, their exclusive prefix sums, the scatter's cursors, and per variant the {first entry, length} of its
// list in `lists` (what a planned fill reads through BandParams::off2).
constexpr int kBandPlanHeadCounts = 0, kBandPlanHeadOffsets = kBandPlanKeys, kBandPlanHeadCursors = 2 * kBandPlanKeys;
constexpr int kBandPlanHeadLists = 3 * kBandPlanKeys, kBandPlanHeadWords = 2048;
static_assert(kBandPlanHeadWords % 64 == 0 && kBandPlanHeadWords >= kBandPlanHeadLists + 2 * kBandVariants,
              "8 KiB hold the four tables, and what follows the head stays 256-byte aligned");
struct BandPlannerParams {
    const uint8_t* seq1;        // the two resident buffers and the pairs' slices of them
    uint64_t seq1_bytes;
    const uint64_t* start1;
    const uint32_t* len1;
    const uint8_t* seq2;
    uint64_t seq2_bytes;
    const uint64_t* start2;
    const uint32_t* len2;
    const int32_t* diag;
    const uint64_t* ops_off;    // NULL: a score call (no ops, no records, no record guard)
    uint64_t ops_bytes;
    sa_result* res;
    uint32_t first, count;      // the chunk: pairs first .. first + count - 1 of the call
    uint32_t max_m, max_n;
    int32_t w;
    uint32_t free_ends;
    int affine;
    int vmax;                   // the bound's variant
    int32_t span;               // the bound's steps (the sweep buckets' scale)
    uint64_t bound_words;       // the bound's record words: the stride of the chunk's record slots
    uint32_t* head;
    BandPlanRec* plans;         // count records
    uint32_t* lists;            // count entries: plan record numbers, variant by variant
};
hipError_t launch_band_planner(const BandPlannerParams& p, hipStream_t s);
hipError_t launch_band_lut_bits(const uint8_t* d_lut, uint32_t* bits, hipStream_t s);

// The pairs of one chunk: as many as the budget holds records of the bound for.  0: one pair's bound
// exceeds the budget.  (A score call stores no records: bound_words = 0, one chunk.)
inline uint32_t band_plan_chunk_pairs(uint64_t bound_words, uint64_t budget_bytes, uint32_t npairs) {
    if (!bound_words) return npairs;
    const uint64_t fit = budget_bytes / 4 / bound_words;
    return (uint32_t)(fit < npairs ? fit : npairs);
}

}  // namespace sa
