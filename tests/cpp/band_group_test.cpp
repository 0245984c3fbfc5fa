// band_group_test.cpp — the banded calls' grouping of pairs into launches (seqalib_amd/csrc/sa_band_group.h)
// against the rule as its comment states it, on random batches and three hand-worked ones.  Host only:
// no device is touched.  Prints "ok"; built and run by tests/test_band_group.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../seqalib_amd/csrc/sa_band_group.h"

using namespace sa;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: %s (batch %d)\n", __FILE__, __LINE__, #cond, g_batch); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)
static int g_batch = -1;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*, [0, n)
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull >> 33) % n);
}

struct Batch {
    std::vector<uint64_t> off1{0}, off2{0};
    std::vector<int32_t> diag;
    uint32_t n() const { return (uint32_t)off1.size() - 1; }
    void add(uint32_t m, uint32_t nn) {
        off1.push_back(off1.back() + m);
        off2.push_back(off2.back() + nn);
    }
    int64_t len(uint32_t p) const { return (int64_t)(off1[p + 1] - off1[p] + off2[p + 1] - off2[p]); }
};

static BandGroupIn input(const Batch& b, bool seeded, int32_t w, bool affine, bool notb, uint64_t budget, uint64_t simds, bool merge) {
    return BandGroupIn{b.off1.data(), b.off2.data(), b.n(), seeded ? b.diag.data() : nullptr, w,
                       affine ? kBandAffineVariants : kBandVariants, affine ? band_affine_rec_words : band_rec_words,
                       notb, notb ? 0 : budget, simds, merge};
}

// The narrowest variant of a pair, restated: the first whose 2 R L diagonals hold the clipped band.
static int narrowest(const BandGroupIn& in, uint32_t p, BandGeom* g) {
    *g = band_group_geom(in, p);
    for (int v = 0; v < in.nvariants; ++v)
        if (g->beff <= 2 * kBandR[v] * kBandL[v]) return v;
    return -1;
}

static void check_rule(const BandGroupIn& in) {
    const uint32_t np = in.npairs;
    std::vector<int> nv(np);
    std::vector<BandGeom> geom(np);
    std::vector<uint32_t> own[kBandVariants];
    bool too_big = false;
    for (uint32_t p = 0; p < np; ++p) {
        nv[p] = narrowest(in, p, &geom[p]);
        CHECK(nv[p] >= 0);
        own[nv[p]].push_back(p);
        if (!in.notb && in.rec_words(geom[p], nv[p]) > in.budget_words) too_big = true;
    }
    // the merges the rule allows, lowest variant first: both variants in use, the lower one took no pairs
    // in, the joint launch has at most one wave per SIMD, every moved pair's records fit the budget
    std::vector<int> at(np);
    for (uint32_t p = 0; p < np; ++p) at[p] = nv[p];
    bool took_in = false;
    for (int v = 0; v + 1 < in.nvariants; ++v) {
        const bool fixed = took_in;
        took_in = false;
        if (!in.merge || fixed || own[v].empty() || own[v + 1].empty()) continue;
        const uint64_t ppw = 64 / kBandL[v + 1];
        if ((own[v].size() + own[v + 1].size() + ppw - 1) / ppw > in.simds) continue;
        bool fits = true;
        for (uint32_t p : own[v])
            if (!in.notb && in.rec_words(geom[p], v + 1) > in.budget_words) fits = false;
        if (!fits) continue;
        for (uint32_t p : own[v]) at[p] = v + 1;
        took_in = true;
    }

    BandGroups g;
    const bool ok = band_group(in, &g);
    CHECK(ok == !too_big);   // a pair larger than the budget is the error (a moved pair always fits)
    if (!ok) {
        CHECK(g.too_big_words > in.budget_words);
        bool found = false;
        for (uint32_t p = 0; p < np; ++p) found = found || in.rec_words(geom[p], at[p]) == g.too_big_words;
        CHECK(found);
        return;
    }
    // every pair exactly once, in its narrowest variant or the next one up -- where the rule puts it
    CHECK(g.idx.size() == np && g.recoff.size() == np);
    std::vector<int> seen(np, 0), where(np, -1);
    uint32_t next = 0;
    uint64_t largest = 0;
    int top = 0, prev_v = -1;
    for (size_t l = 0; l < g.launches.size(); ++l) {
        const BandLaunch& ln = g.launches[l];
        CHECK(ln.first == next && ln.count > 0 && ln.v >= prev_v && ln.v < in.nvariants);
        uint64_t used = 0;
        for (uint32_t k = ln.first; k < ln.first + ln.count; ++k) {
            const uint32_t p = g.idx[k];
            CHECK(p < np && !seen[p]++);
            where[p] = ln.v;
            CHECK(ln.v == nv[p] || ln.v == nv[p] + 1);
            CHECK(ln.v == at[p]);
            CHECK(g.recoff[k] == used);   // the running sum of words, restarting at each launch
            used += in.notb ? 0 : in.rec_words(geom[p], ln.v);
        }
        CHECK(used <= in.budget_words);   // no launch exceeds the budget
        if (ln.v == prev_v) {             // a second launch of a variant: its first pair did not fit the one before
            CHECK(!in.notb);
            const BandLaunch& before = g.launches[l - 1];
            uint64_t sum = 0;
            for (uint32_t k = before.first; k < before.first + before.count; ++k) sum += in.rec_words(geom[g.idx[k]], ln.v);
            CHECK(sum + in.rec_words(geom[g.idx[ln.first]], ln.v) > in.budget_words);
        }
        largest = std::max(largest, used);
        top = std::max(top, ln.v);
        prev_v = ln.v;
        next += ln.count;
    }
    CHECK(next == np);
    CHECK(g.ws_words == largest && g.top_v == top);
    // a variant that took pairs in moves none out; merging off: every pair in its narrowest variant
    for (int v = 1; v < in.nvariants; ++v) {
        bool took = false;
        for (uint32_t p = 0; p < np; ++p) took = took || (nv[p] == v - 1 && where[p] == v);
        for (uint32_t p = 0; p < np && took; ++p) CHECK(nv[p] != v || where[p] == v);
    }
    for (uint32_t p = 0; p < np && !in.merge; ++p) CHECK(where[p] == nv[p]);
    // within a variant's launches: m + n descending, stably (its own pairs, then the pairs moved in, by index)
    for (size_t k = 1; k < g.idx.size(); ++k) {
        const uint32_t x = g.idx[k - 1], y = g.idx[k];
        if (where[x] != where[y]) continue;
        const int64_t lx = (int64_t)(in.off1[x + 1] - in.off1[x] + in.off2[x + 1] - in.off2[x]);
        const int64_t ly = (int64_t)(in.off1[y + 1] - in.off1[y] + in.off2[y + 1] - in.off2[y]);
        CHECK(lx >= ly);
        if (lx == ly) {
            const bool mx = nv[x] != where[x], my = nv[y] != where[y];
            CHECK(mx < my || (mx == my && x < y));
        }
    }
    if (in.notb) {   // all words 0, one launch per used variant
        CHECK(g.ws_words == 0);
        for (uint64_t r : g.recoff) CHECK(r == 0);
        for (size_t l = 1; l < g.launches.size(); ++l) CHECK(g.launches[l].v > g.launches[l - 1].v);
    }
    if (in.diag) {   // the seeded calls' array: per launch [idx entries][their diagonals]
        const std::vector<uint32_t> both = band_idx_with_diagonals(g, in.diag);
        CHECK(both.size() == 2 * (size_t)np);
        for (const BandLaunch& ln : g.launches)
            for (uint32_t k = 0; k < ln.count; ++k) {
                CHECK(both[2 * ln.first + k] == g.idx[ln.first + k]);
                CHECK((int32_t)both[2 * ln.first + ln.count + k] == in.diag[g.idx[ln.first + k]]);
            }
    }
}

static void random_batches() {
    const int32_t widths[4] = {0, 3, 40, 300};
    const uint64_t simd_counts[3] = {1, 2, 1024};
    int merged = 0, refused = 0, split = 0, nomem = 0;
    for (g_batch = 0; g_batch < 600; ++g_batch) {
        Batch b;
        const uint32_t np = 1 + rnd(40);
        const uint32_t top = (g_batch % 3 == 0) ? 60 : 601;   // (short batches: several pairs per variant)
        for (uint32_t p = 0; p < np; ++p) b.add(rnd(top), rnd(top));
        for (uint32_t p = 0; p < np; ++p) {
            const int32_t m = (int32_t)(b.off1[p + 1] - b.off1[p]), n = (int32_t)(b.off2[p + 1] - b.off2[p]);
            b.diag.push_back(-m + (int32_t)rnd((uint32_t)(m + n + 1)));
        }
        const int32_t w = widths[rnd(4)];
        const bool affine = rnd(2), seeded = rnd(2), notb = rnd(4) == 0;
        const uint64_t simds = simd_counts[rnd(3)];
        // budgets: ample, about one pair's records (splits, refused merges, the error), in between
        BandGroupIn probe = input(b, seeded, w, affine, false, 0, simds, false);
        uint64_t most = 1, total = 0;
        for (uint32_t p = 0; p < np; ++p) {
            BandGeom g;
            const int v = narrowest(probe, p, &g);
            most = std::max(most, probe.rec_words(g, v));
            total += probe.rec_words(g, v);
        }
        const uint64_t budgets[5] = {~0ull >> 2, most, most * 2, most - most / 4, std::max<uint64_t>(total / 3, 1)};
        const uint64_t budget = budgets[rnd(5)];
        for (int merge = 0; merge < 2; ++merge) {
            const BandGroupIn in = input(b, seeded, w, affine, notb, budget, simds, merge);
            check_rule(in);
            BandGroups g, g0;
            if (!band_group(in, &g)) {
                nomem++;
                continue;
            }
            for (size_t l = 1; l < g.launches.size(); ++l) split += g.launches[l].v == g.launches[l - 1].v;
            if (merge && band_group(input(b, seeded, w, affine, notb, budget, simds, false), &g0)) {
                std::vector<int> used0(kBandVariants, 0), used1(kBandVariants, 0);
                for (const BandLaunch& ln : g0.launches) used0[ln.v] = 1;
                for (const BandLaunch& ln : g.launches) used1[ln.v] = 1;
                bool any = false, adjacent = false;
                for (int v = 0; v < kBandVariants; ++v) any = any || used0[v] != used1[v];
                for (int v = 0; v + 1 < kBandVariants; ++v) adjacent = adjacent || (used0[v] && used0[v + 1]);
                merged += any;
                refused += !any && adjacent;
            }
        }
    }
    g_batch = -1;
    // the inputs took every branch of the rule
    CHECK(merged > 20 && refused > 20 && split > 20 && nomem > 20);
}

static void expect(const BandGroups& g, std::vector<BandLaunch> launches, std::vector<uint32_t> idx, std::vector<uint64_t> recoff,
                   uint64_t ws_words, int top_v) {
    CHECK(g.launches.size() == launches.size());
    for (size_t l = 0; l < launches.size(); ++l)
        CHECK(g.launches[l].v == launches[l].v && g.launches[l].first == launches[l].first && g.launches[l].count == launches[l].count);
    CHECK(g.idx == idx && g.recoff == recoff && g.ws_words == ws_words && g.top_v == top_v);
}

// w = 3, the linear family (2-bit records).  An m x m pair has 7 diagonals (variant 0: R 1, L 16, up to 32),
// m x (m + 40) has 47 (variant 1: R 2, L 16, up to 64), m x (m + 100) has 107 (variant 2: R 4, L 16); four
// pairs per wave in all three.  Records run over steps tb = 2 .. tend = m + n + 3, m + n + 2 of them:
// variant 0 stores ceil(steps / 16) * 16 words, variant 1 ceil(steps / 8) * 16, variant 2 ceil(steps / 4) * 16.
static void hand_worked() {
    const uint64_t ample = 1ull << 40;
    {   // one merge: variant 0's pair joins variant 1 (one wave); variant 1 took pairs in, so it stays below 2
        g_batch = -2;
        Batch b;
        b.add(100, 100);   // variant 0; in variant 1: 202 steps -> 26 * 16 = 416 words
        b.add(100, 140);   // variant 1: 242 steps -> 31 * 16 = 496
        b.add(100, 200);   // variant 2: 302 steps -> 76 * 16 = 1216
        BandGroups g;
        CHECK(band_group(input(b, false, 3, false, false, ample, 1024, true), &g));
        expect(g, {{1, 0, 2}, {2, 2, 1}}, {1, 0, 2}, {0, 496, 0}, 1216, 2);
        check_rule(input(b, false, 3, false, false, ample, 1024, true));
    }
    {   // a refused merge: one SIMD, and variants 0 and 1 together hold five pairs -- two waves
        g_batch = -3;
        Batch b;
        b.add(100, 100);   // variant 0: 202 steps -> 13 * 16 = 208
        b.add(90, 90);     //            182       -> 12 * 16 = 192
        b.add(80, 80);     //            162       -> 11 * 16 = 176
        b.add(100, 140);   // variant 1: 242 -> 496
        b.add(90, 130);    //            222 -> 28 * 16 = 448
        BandGroups g;
        CHECK(band_group(input(b, false, 3, false, false, ample, 1, true), &g));
        expect(g, {{0, 0, 3}, {1, 3, 2}}, {0, 1, 2, 3, 4}, {0, 208, 400, 0, 496}, 944, 1);
        check_rule(input(b, false, 3, false, false, ample, 1, true));
    }
    {   // a budget split: 400 words hold the first two pairs exactly, the third opens a launch; 175 hold none
        g_batch = -4;
        Batch b;
        b.add(80, 80);
        b.add(100, 100);
        b.add(90, 90);
        BandGroups g;
        CHECK(band_group(input(b, false, 3, false, false, 400, 1024, true), &g));
        expect(g, {{0, 0, 2}, {0, 2, 1}}, {1, 2, 0}, {0, 208, 0}, 400, 0);
        BandGroups none;
        CHECK(!band_group(input(b, false, 3, false, false, 175, 1024, true), &none) && none.too_big_words == 208);
        BandGroups score;   // a score call: no records, so no budget either
        CHECK(band_group(input(b, false, 3, false, true, 0, 1024, true), &score));
        expect(score, {{0, 0, 3}}, {1, 2, 0}, {0, 0, 0}, 0, 0);
    }
    g_batch = -1;
}

int main() {
    hand_worked();
    random_batches();
    printf("ok\n");
    return 0;
}
