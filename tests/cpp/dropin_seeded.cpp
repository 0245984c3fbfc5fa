// Drop-in check of the seeded extensions of include/seqalib/ (sa_align_batch_banded_seeded /
// sa_score_batch_banded_seeded): getAlignments(pairs, diags, band, freeEnds) and getScores(pairs, diags,
// band, freeEnds) on NeedlemanWunschSA, HirschbergSA and GlobalGotohSA, for std::string sequences.  Each
// class
//   aligns, at band 6, the pairs of a fixed batch whose seeded band is legal under the fit, overlap,
//   all-free and no-free flag sets and prints, per pair, the inputs, the seed diagonal and the three
//   printed rows (Seq1 row, bars, Seq2 row), then getScores of the batch;
//   must throw std::runtime_error for freeEnds > 15, for a diags of another size than pairs, for a band
//   that holds no legal begin (with the engine's message) and (where there is one) after setSubstitution().
// tests/test_dropin_seeded.py recomputes the printed rows and scores with the Python classes.
// Output: "pair <class> <freeEnds> <index> <diag>" followed by "s1 ..", "s2 ..", "r0 ..", "bars ..",
// "r1 .." lines (each value between '[' and ']'), "scores <class> <freeEnds> ..", and "ok ..." /
// "FAIL ..." lines; returns the number of failures.
#include <cstdint>
#include <functional>
#include <iostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "seqalib/SequenceAlignment.h"

static uint64_t lcg(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

static int failures = 0;
static const size_t kBand = 6;
using Str = std::string;
using Ptrs = std::vector<std::pair<Str*, Str*>>;

static void report(const std::string& what, bool ok) {
    std::cout << (ok ? "ok " : "FAIL ") << what << '\n';
    if (!ok) ++failures;
}

struct Case {
    unsigned free_ends;
    std::vector<size_t> pairs;       // indices into the batch
    std::vector<int32_t> diags;      // their seed diagonals
};

template <typename Fn>
static bool throws(Fn fn, const char* needle = nullptr) {
    try {
        fn();
    } catch (const std::runtime_error& e) {
        return !needle || std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

template <typename Aligner>
static void print_class(const std::string& cls, Aligner al, std::vector<std::pair<Str, Str>>& seqs, const std::vector<Case>& cases) {
    for (const Case& c : cases) {
        Ptrs ptrs;
        for (size_t p : c.pairs) ptrs.push_back({&seqs[p].first, &seqs[p].second});
        auto got = al.getAlignments(ptrs, c.diags, kBand, c.free_ends);
        const ScoreSystemType last = al.getScore();
        for (size_t q = 0; q < ptrs.size(); ++q) {
            std::string r0, bars, r1;
            for (auto e = got[q].begin(); e != got[q].end(); ++e) {
                r0.push_back(e->get(0));
                bars.push_back(e->match() ? '|' : ' ');
                r1.push_back(e->get(1));
            }
            std::cout << "pair " << cls << ' ' << c.free_ends << ' ' << q << ' ' << c.diags[q] << "\ns1 [" << *ptrs[q].first << "]\ns2 ["
                      << *ptrs[q].second << "]\nr0 [" << r0 << "]\nbars [" << bars << "]\nr1 [" << r1 << "]\n";
        }
        const std::vector<ScoreSystemType> scores = al.getScores(ptrs, c.diags, kBand, c.free_ends);
        std::cout << "scores " << cls << ' ' << c.free_ends;
        for (auto s : scores) std::cout << ' ' << s;
        std::cout << '\n';
        report(cls + " " + std::to_string(c.free_ends) + " getScore() is the last pair's", !scores.empty() && last == scores.back());
    }
    const Case& fit = cases[0];
    Ptrs ptrs;
    for (size_t p : fit.pairs) ptrs.push_back({&seqs[p].first, &seqs[p].second});
    report(cls + " freeEnds 16 throws", throws([&] { al.getAlignments(ptrs, fit.diags, kBand, 16u); }) &&
                                            throws([&] { al.getScores(ptrs, fit.diags, kBand, 16u); }));
    std::vector<int32_t> fewer(fit.diags.begin(), fit.diags.end() - 1);
    report(cls + " a diags of another size throws", throws([&] { al.getAlignments(ptrs, fewer, kBand, fit.free_ends); }, "seed diagonals") &&
                                                        throws([&] { al.getScores(ptrs, fewer, kBand, fit.free_ends); }, "seed diagonals"));
    // the fit's seeds without SA_FREE_SEQ2_BEGIN: the band begins on row 0, where nothing may begin
    report(cls + " a band with no legal begin throws",
           throws([&] { al.getAlignments(ptrs, fit.diags, kBand, (unsigned)SA_FREE_SEQ2_END); }, "no legal begin") &&
               throws([&] { al.getScores(ptrs, fit.diags, kBand, (unsigned)SA_FREE_SEQ2_END); }, "no legal begin"));
}

template <typename Aligner>
static void check_substitution(const std::string& cls, Aligner al, std::vector<std::pair<Str, Str>>& seqs, const Case& c) {
    Ptrs ptrs;
    for (size_t p : c.pairs) ptrs.push_back({&seqs[p].first, &seqs[p].second});
    al.setSubstitution([](char a, char b) { return a == b ? 2 : -1; });
    report(cls + " substitution scoring with a seeded band throws",
           throws([&] { al.getAlignments(ptrs, c.diags, kBand, c.free_ends); }) && throws([&] { al.getScores(ptrs, c.diags, kBand, c.free_ends); }));
}

int main() {
    uint64_t seed = 4343;
    const std::string letters = "ACGT";
    auto rnd = [&](int len) {
        std::string s;
        for (int k = 0; k < len; ++k) s.push_back(letters[lcg(seed) % letters.size()]);
        return s;
    };
    auto mutate = [&](const std::string& a) {
        std::string b;
        for (char c : a) {
            const int r = (int)(lcg(seed) % 100);
            if (r < 4) b.push_back(letters[lcg(seed) % letters.size()]);
            else if (r < 6) continue;
            else b.push_back(c);
        }
        return b;
    };
    std::vector<std::pair<Str, Str>> seqs;
    const Str window = rnd(160), other = rnd(120);
    seqs.push_back({mutate(window.substr(40, 60)), window});                 // 0: a read in a window, on diagonal 40
    seqs.push_back({mutate(window.substr(0, 50)), window.substr(0, 110)});   // 1: at the window's start, diagonal 0
    seqs.push_back({other, mutate(other.substr(70)) + rnd(5)});              // 2: two overlapping reads, diagonal -70
    seqs.push_back({rnd(7), Str()});                                         // 3: an empty side
    seqs.push_back({Str(), rnd(3)});                                         // 4
    seqs.push_back({mutate(window.substr(100, 40)), window.substr(60)});     // 5: a read at the window's end, diagonal 40
    seqs.push_back({rnd(30), rnd(34)});                                      // 6: unrelated
    const unsigned fit = SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END, overlap = SA_FREE_SEQ1_BEGIN | SA_FREE_SEQ2_END;
    const std::vector<Case> cases = {
        {fit, {0, 1, 5}, {38, 2, 43}},
        {overlap, {2, 1}, {-68, 0}},
        {15u, {0, 1, 2, 3, 4, 5, 6}, {41, -1, -71, -3, 1, 39, 20}},
        {0u, {6, 3, 4}, {2, -3, 1}},
    };

    const ScoringSystem lin(-2, 2, -3), aff(-3, -1, 2, -3);
    print_class("NeedlemanWunschSA", NeedlemanWunschSA<Str, char, '-'>(lin), seqs, cases);
    print_class("HirschbergSA", HirschbergSA<Str, char, '-'>(lin), seqs, cases);
    print_class("GlobalGotohSA", GlobalGotohSA<Str, char, '-'>(aff), seqs, cases);
    check_substitution("NeedlemanWunschSA", NeedlemanWunschSA<Str, char, '-'>(lin), seqs, cases[0]);
    check_substitution("GlobalGotohSA", GlobalGotohSA<Str, char, '-'>(aff), seqs, cases[0]);
    return failures;
}
