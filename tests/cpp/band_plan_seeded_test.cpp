// band_plan_seeded_test.cpp — what the device-resident seeded band calls rest on (seqalib_amd/csrc/sa_band_plan.h),
// compiled for the host: the bound the host provisions from (max_m, max_n, band, algorithm) alone holds every
// pair inside it at every seed diagonal -- variant, steps and record words -- and is tight at the bound shape;
// the per-pair function gives the variant, key and record words the host layer gives; and the shared legality
// function agrees with the header's rule restated over the band's cells, for all 16 free_ends sets.  Host only:
// no device is touched.  Prints "ok"; built and run by tests/test_band_plan_seeded.py.
#include <stdio.h>
#include <stdlib.h>

#include "../../seqalib_amd/csrc/sa_band_plan.h"

using namespace sa;

static int32_t g_m, g_n, g_k, g_w, g_mm, g_mn;
#define CHECK(cond)                                                                                                  \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            fprintf(stderr, "%s:%d: %s (m %d n %d diag %d w %d, bounds %d x %d)\n", __FILE__, __LINE__, #cond, g_m, g_n, \
                    g_k, g_w, g_mm, g_mn);                                                                           \
            exit(1);                                                                                                 \
        }                                                                                                            \
    } while (0)

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*, [0, n)
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull >> 33) % n);
}

// The narrowest variant, restated: the first whose 2 R L diagonals hold the clipped band.
static int narrowest(int64_t beff, bool affine) {
    for (int v = 0; v < (affine ? kBandAffineVariants : kBandVariants); ++v)
        if (beff <= 2 * kBandR[v] * kBandL[v]) return v;
    return -1;
}

// The bound, restated from the issue's two inequalities.
static int64_t min3(int64_t a, int64_t b, int64_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
static int64_t bound_steps(int64_t M, int64_t N, int64_t w) { return min3(M + N, 2 * M + 2 * w, 2 * N + 2 * w) + 2; }
static int64_t bound_beff(int64_t M, int64_t N, int64_t w) { return 2 * w + 1 < M + N + 1 ? 2 * w + 1 : M + N + 1; }

static uint64_t g_max_steps;   // per bound shape: the most steps a pair inside it took

// One pair at one diagonal inside one bound shape.
static void check_pair(int32_t m, int32_t n, int32_t k, int32_t w, bool affine, const BandPlanBound& b) {
    g_m = m;
    g_n = n;
    g_k = k;
    const BandPlanPair p = band_plan_pair(m, n, w, k, affine, b.span);
    const BandGeom g = band_geom_seeded(m, n, w, k);
    CHECK(p.g.lo == g.lo && p.g.hi == g.hi && p.g.beff == g.beff && p.g.tb == g.tb && p.g.tend == g.tend);
    CHECK(g.beff >= 1 && g.tend >= g.tb);
    // what the host layer gives the pair (SEQALIB_BAND_MERGE=0): the narrowest variant and its record words
    CHECK(p.v == narrowest(g.beff, affine));
    CHECK(p.v >= 0);
    CHECK(p.rec_words == (affine ? band_affine_rec_words(g, p.v) : band_rec_words(g, p.v)));
    // the bound holds it
    const uint64_t steps = (uint64_t)(g.tend - g.tb) + 1;
    CHECK(g.beff <= bound_beff(g_mm, g_mn, w));
    CHECK(p.v <= b.vmax);
    CHECK((int64_t)steps <= (int64_t)b.span);
    CHECK(p.rec_words <= b.rec_words);
    if (steps > g_max_steps) g_max_steps = steps;
    // the key: the variant's block, a bucket inside it
    CHECK(p.key < (uint32_t)kBandPlanKeys && (int)(p.key / kBandPlanBuckets) == p.v);
}

static bool check_bound(int32_t mm, int32_t mn, int32_t w, bool affine, BandPlanBound* b) {
    g_mm = mm;
    g_mn = mn;
    g_w = w;
    g_m = g_n = g_k = -1;
    *b = band_plan_bound_seeded(mm, mn, w, affine);
    CHECK(b->vmax == narrowest(bound_beff(mm, mn, w), affine));
    if (b->vmax < 0) return false;
    CHECK(b->span == bound_steps(mm, mn, w));
    const BandGeom steps{0, 0, 0, 0, b->span - 1};
    CHECK(b->rec_words == (affine ? band_affine_rec_words(steps, b->vmax) : band_rec_words(steps, b->vmax)));
    return true;
}

// The header's legality rule over the band's cells: a legal begin is (0, 0), a row-0 cell under
// SA_FREE_SEQ2_BEGIN or a column-0 cell under SA_FREE_SEQ1_BEGIN; a legal end is (m, n), a last-row cell under
// SA_FREE_SEQ2_END or a last-column cell under SA_FREE_SEQ1_END.
static int legality_by_cells(int32_t m, int32_t n, int32_t w, int32_t k, uint32_t fe) {
    bool begin = false, end = false;
    for (int32_t i = 0; i <= m; ++i)
        for (int32_t j = 0; j <= n; ++j) {
            if (j - i < k - w || j - i > k + w) continue;
            if ((i == 0 && j == 0) || (i == 0 && (fe & 4u)) || (j == 0 && (fe & 1u))) begin = true;
            if ((i == m && j == n) || (i == m && (fe & 8u)) || (j == n && (fe & 2u))) end = true;
        }
    return (begin ? 1 : 0) | (end ? 2 : 0);
}

int main() {
    const int32_t widths[] = {0, 1, 3, 8, 17, 40};
    constexpr int32_t N = 12;
    // every (m, n, k) inside every bound shape up to 12 x 12
    for (int affine = 0; affine < 2; ++affine)
        for (int32_t w : widths)
            for (int32_t mm = 0; mm <= N; ++mm)
                for (int32_t mn = 0; mn <= N; ++mn) {
                    BandPlanBound b;
                    CHECK(check_bound(mm, mn, w, affine != 0, &b));
                    g_max_steps = 0;
                    for (int32_t m = 0; m <= mm; ++m)
                        for (int32_t n = 0; n <= mn; ++n)
                            for (int32_t k = -m; k <= n; ++k) check_pair(m, n, k, w, affine != 0, b);
                    g_m = g_n = g_k = -1;
                    CHECK(g_max_steps + 2 >= (uint64_t)b.span);   // tight: within the even start's step and one more
                }
    // the legality function against the rule over cells: the same triples, all 16 flag sets
    for (int32_t w : widths) {
        g_w = w;
        g_mm = g_mn = N;
        for (int32_t m = 0; m <= N; ++m)
            for (int32_t n = 0; n <= N; ++n)
                for (int32_t k = -m; k <= n; ++k) {
                    g_m = m;
                    g_n = n;
                    g_k = k;
                    const BandGeom g = band_geom_seeded(m, n, w, k);
                    for (uint32_t fe = 0; fe < 16; ++fe) CHECK(band_seed_legality(g, m, n, fe) == legality_by_cells(m, n, w, k, fe));
                    CHECK((band_seed_legality(g, m, n, 15) == kBandSeedLegal));   // every end free: every band in the matrix is legal
                }
    }
    // random bound shapes up to 3000 with w up to 2047 (affine: 1023): corners, extreme and random diagonals
    int taken = 0;
    for (int t = 0; t < 300; ++t) {
        const bool affine = (t & 1) != 0;
        const int32_t w = (int32_t)rnd(affine ? 1024 : 2048), mm = (int32_t)rnd(3001), mn = (int32_t)rnd(3001);
        BandPlanBound b;
        if (!check_bound(mm, mn, w, affine, &b)) continue;
        ++taken;
        const int32_t shapes[][2] = {{mm, mn}, {0, 0}, {mm, 0}, {0, mn}, {(int32_t)rnd(mm + 1), (int32_t)rnd(mn + 1)},
                                     {(int32_t)rnd(mm + 1), (int32_t)rnd(mn + 1)}, {(int32_t)rnd(mm + 1), mn}, {mm, (int32_t)rnd(mn + 1)}};
        for (const auto& q : shapes) {
            const int32_t m = q[0], n = q[1];
            const int32_t ks[] = {-m, n, 0 < -m ? -m : (0 > n ? n : 0), n - m < -m ? -m : n - m, (n - m) / 2, -m + (int32_t)rnd(m + n + 1),
                                  -m + (int32_t)rnd(m + n + 1), -m + (w < m + n ? w : m + n), n - (w < m + n ? w : m + n)};
            for (int32_t k : ks) check_pair(m, n, k, w, affine, b);
        }
    }
    g_m = g_n = g_k = -1;
    CHECK(taken == 300);   // (2w + 1 diagonals at most: within 4096 / 2048)
    // the two shapes of the measured cases at w = 16: at some diagonal the bound shape itself takes all but at
    // most one step of the bound
    {
        BandPlanBound b = band_plan_bound_seeded(2000, 2000, 16, false);
        BandGeom g;
        int32_t most = 0;
        for (int32_t k = -2000; k <= 2000; ++k) {
            g = band_geom_seeded(2000, 2000, 16, k);
            if (g.tend - g.tb + 1 > most) most = g.tend - g.tb + 1;
        }
        CHECK(b.span == 4002 && most == 4002);
        b = band_plan_bound_seeded(150, 100000, 16, false);
        most = 0;
        for (int32_t k = -150; k <= 100000; ++k) {
            g = band_geom_seeded(150, 100000, 16, k);
            if (g.tend - g.tb + 1 > most) most = g.tend - g.tb + 1;
        }
        CHECK(b.span == 334 && most == 333);
    }
    printf("ok\n");
    return 0;
}
