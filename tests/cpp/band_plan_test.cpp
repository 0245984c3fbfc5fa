// band_plan_test.cpp — the per-pair function of the device planner (seqalib_amd/csrc/sa_band_plan.h), compiled
// for the host: against the host layer's variant and record words for every pair inside a bound shape, the
// bound the host provisions from that shape alone, the list keys, and the chunk arithmetic.  Host only: no
// device is touched.  Prints "ok"; built and run by tests/test_band_plan.py.
#include <stdio.h>
#include <stdlib.h>

#include "../../seqalib_amd/csrc/sa_band_group.h"
#include "../../seqalib_amd/csrc/sa_band_plan.h"

using namespace sa;

static int32_t g_m, g_n, g_w, g_mm, g_mn;
#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            fprintf(stderr, "%s:%d: %s (m %d n %d w %d, bounds %d x %d)\n", __FILE__, __LINE__, #cond, g_m, g_n, g_w, \
                    g_mm, g_mn);                                                                           \
            exit(1);                                                                                       \
        }                                                                                                  \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*, [0, n)
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull >> 33) % n);
}

// The narrowest variant, restated: the first whose 2 R L diagonals hold the clipped band.
static int narrowest(int32_t beff, bool affine) {
    for (int v = 0; v < (affine ? kBandAffineVariants : kBandVariants); ++v)
        if (beff <= 2 * kBandR[v] * kBandL[v]) return v;
    return -1;
}

// What the host layer computes for one pair (sa_band_group.h with the extension calls' zero diagonals).
struct HostPair {
    BandGeom g;
    int v;
    uint64_t words;
};
static HostPair host_pair(int32_t m, int32_t n, int32_t w, bool affine) {
    g_m = m;
    g_n = n;
    const uint64_t off1[2] = {0, (uint64_t)m}, off2[2] = {0, (uint64_t)n};
    const int32_t zero = 0;
    const BandGroupIn in{off1, off2, 1, &zero, w, affine ? kBandAffineVariants : kBandVariants,
                         affine ? band_affine_rec_words : band_rec_words, false, ~0ull, 1024, false};
    HostPair h;
    h.g = band_group_geom(in, 0);
    BandGroups grp;
    CHECK(band_group(in, &grp) && grp.launches.size() == 1);
    h.v = grp.launches[0].v;
    h.words = grp.ws_words;
    CHECK(h.v == narrowest(h.g.beff, affine));
    CHECK(h.v == (affine ? band_affine_variant(h.g.beff) : band_variant(h.g.beff)));
    CHECK(h.words == (affine ? band_affine_rec_words(h.g, h.v) : band_rec_words(h.g, h.v)));
    return h;
}

// One pair inside one bound shape: the shared function against the host layer, and the bound against both.
static void check_pair(int32_t m, int32_t n, int32_t w, bool affine, const BandPlanBound& b, const HostPair& h) {
    g_m = m;
    g_n = n;
    const BandPlanPair p = band_plan_pair(m, n, w, 0, affine, b.span);
    const BandGeom& g = h.g;
    CHECK(p.g.lo == g.lo && p.g.hi == g.hi && p.g.beff == g.beff && p.g.tb == g.tb && p.g.tend == g.tend);
    CHECK(p.v == h.v);
    CHECK(p.rec_words == h.words);
    // the bound holds it: variant, sweep, records
    CHECK(p.v >= 0 && p.v <= b.vmax);
    CHECK(g.tend - g.tb >= 0 && g.tend - g.tb < b.span);
    CHECK(b.rec_words >= p.rec_words);
    // the key: the variant's block, longest bucket first
    CHECK(p.key < (uint32_t)kBandPlanKeys && (int)(p.key / kBandPlanBuckets) == p.v);
    const int bucket = kBandPlanBuckets - 1 - (int)(p.key % kBandPlanBuckets);
    CHECK((int64_t)bucket * b.span <= (int64_t)(g.tend - g.tb) * kBandPlanBuckets);
    CHECK((int64_t)(bucket + 1) * b.span > (int64_t)(g.tend - g.tb) * kBandPlanBuckets);
}

// The bound of one shape; false: the calls refuse the shape.
static bool check_bound(int32_t mm, int32_t mn, int32_t w, bool affine, BandPlanBound* b) {
    g_mm = mm;
    g_mn = mn;
    g_w = w;
    g_m = g_n = -1;
    *b = band_plan_bound(mm, mn, w, affine);
    const BandGeom gb = band_geom_seeded(mm, mn, w, 0);
    CHECK(b->vmax == narrowest(gb.beff, affine));
    if (b->vmax < 0) return false;
    // the bound shape itself is the tightest case: at most one step of the widest record more than its own
    const uint64_t own = affine ? band_affine_rec_words(gb, b->vmax) : band_rec_words(gb, b->vmax);
    CHECK(b->rec_words >= own && b->rec_words <= own + 2ull * kBandL[b->vmax]);
    return true;
}

static void check_chunks() {
    g_m = g_n = g_w = g_mm = g_mn = -1;
    for (int k = 0; k < 2000; ++k) {
        const uint64_t bound = 1 + rnd(1u << 20), limit = rnd(1u << 30);
        const uint32_t npairs = 1 + rnd(100000);
        const uint32_t per = band_plan_chunk_pairs(bound, limit, npairs);
        CHECK(per <= npairs);
        CHECK((uint64_t)per * bound * 4 <= limit);
        if (per < npairs) CHECK((uint64_t)(per + 1) * bound * 4 > limit);   // as many as fit
        CHECK((per == 0) == (bound * 4 > limit));                           // one pair over the limit is reported
    }
    CHECK(band_plan_chunk_pairs(16, 64, 10) == 1);
    CHECK(band_plan_chunk_pairs(16, 63, 10) == 0);
    CHECK(band_plan_chunk_pairs(16, 127, 10) == 1);
    CHECK(band_plan_chunk_pairs(16, 128, 10) == 2);
    CHECK(band_plan_chunk_pairs(16, 1 << 20, 10) == 10);
    CHECK(band_plan_chunk_pairs(0, 0, 10) == 10);   // a score call: no records, one chunk
}

int main() {
    const int32_t widths[] = {0, 1, 3, 8, 17, 40};
    constexpr int32_t N = 40;
    static HostPair host[N + 1][N + 1];
    // every pair inside every bound shape up to 40 x 40
    for (int affine = 0; affine < 2; ++affine)
        for (int32_t w : widths) {
            g_w = w;
            g_mm = g_mn = -1;
            for (int32_t m = 0; m <= N; ++m)
                for (int32_t n = 0; n <= N; ++n) host[m][n] = host_pair(m, n, w, affine != 0);
            for (int32_t mm = 0; mm <= N; ++mm)
                for (int32_t mn = 0; mn <= N; ++mn) {
                    BandPlanBound b;
                    CHECK(check_bound(mm, mn, w, affine != 0, &b));
                    for (int32_t m = 0; m <= mm; ++m)
                        for (int32_t n = 0; n <= mn; ++n) check_pair(m, n, w, affine != 0, b, host[m][n]);
                }
        }
    // random bound shapes up to 5000 with w up to 2047 (affine: 1023), their corners and random pairs inside
    int taken = 0;
    for (int k = 0; k < 400; ++k) {
        const bool affine = (k & 1) != 0;
        const int32_t w = (int32_t)rnd(affine ? 1024 : 2048), mm = (int32_t)rnd(5001), mn = (int32_t)rnd(5001);
        BandPlanBound b;
        if (!check_bound(mm, mn, w, affine, &b)) continue;
        ++taken;
        const int32_t pairs[][2] = {{mm, mn}, {0, 0}, {mm, 0}, {0, mn}, {(int32_t)rnd(mm + 1), (int32_t)rnd(mn + 1)},
                                    {(int32_t)rnd(mm + 1), (int32_t)rnd(mn + 1)}, {(int32_t)rnd(mm + 1), mn}, {mm, (int32_t)rnd(mn + 1)}};
        for (const auto& q : pairs) check_pair(q[0], q[1], w, affine, b, host_pair(q[0], q[1], w, affine));
    }
    g_m = g_n = -1;
    CHECK(taken == 400);   // (2w + 1 diagonals at most: within 4096 / 2048)
    check_chunks();
    printf("ok\n");
    return 0;
}
