// Drop-in check of the ends-free extensions of include/seqalib/ (sa_align_batch_banded_ends_free /
// sa_score_batch_banded_ends_free): getAlignments(pairs, band, freeEnds) and getScores(pairs, band,
// freeEnds) on NeedlemanWunschSA, HirschbergSA and GlobalGotohSA, for std::string sequences.  Each class
//   aligns a fixed batch at band 8 with the fit, overlap, all-free and no-free flag sets and prints, per
//   pair, the inputs and the three printed rows (Seq1 row, bars, Seq2 row), then getScores of the batch;
//   must give getAlignments(pairs, band) entry for entry with freeEnds = 0 (NeedlemanWunschSA and
//   GlobalGotohSA, which have that overload);
//   must throw std::runtime_error for freeEnds > 15 and (where there is one) after setSubstitution().
// tests/test_dropin_ends_free.py recomputes the printed rows and scores with the Python classes.
// Output: "pair <class> <freeEnds> <index>" followed by "s1 ..", "s2 ..", "r0 ..", "bars ..", "r1 .."
// lines (each value between '[' and ']'), "scores <class> <freeEnds> ..", and "ok ..." / "FAIL ..."
// lines; returns the number of failures.
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
static const size_t kBand = 8;
using Str = std::string;
using Ptrs = std::vector<std::pair<Str*, Str*>>;

static void report(const std::string& what, bool ok) {
    std::cout << (ok ? "ok " : "FAIL ") << what << '\n';
    if (!ok) ++failures;
}

template <typename A>
static bool same_alignment(A& x, A& y) {
    if (x.Data.size() != y.Data.size()) return false;
    auto q = y.begin();
    for (auto e = x.begin(); e != x.end(); ++e, ++q)
        if (e->get(0) != q->get(0) || e->get(1) != q->get(1) || e->match() != q->match()) return false;
    return true;
}

template <typename Aligner>
static void print_class(const std::string& cls, Aligner al, std::vector<std::pair<Str, Str>>& seqs, Ptrs& ptrs) {
    for (unsigned fe : {(unsigned)(SA_FREE_SEQ2_BEGIN | SA_FREE_SEQ2_END), (unsigned)(SA_FREE_SEQ1_BEGIN | SA_FREE_SEQ2_END), 15u, 0u}) {
        auto got = al.getAlignments(ptrs, kBand, fe);
        const ScoreSystemType last = al.getScore();
        for (size_t p = 0; p < seqs.size(); ++p) {
            std::string r0, bars, r1;
            for (auto e = got[p].begin(); e != got[p].end(); ++e) {
                r0.push_back(e->get(0));
                bars.push_back(e->match() ? '|' : ' ');
                r1.push_back(e->get(1));
            }
            std::cout << "pair " << cls << ' ' << fe << ' ' << p << "\ns1 [" << seqs[p].first << "]\ns2 [" << seqs[p].second
                      << "]\nr0 [" << r0 << "]\nbars [" << bars << "]\nr1 [" << r1 << "]\n";
        }
        const std::vector<ScoreSystemType> scores = al.getScores(ptrs, kBand, fe);
        std::cout << "scores " << cls << ' ' << fe;
        for (auto s : scores) std::cout << ' ' << s;
        std::cout << '\n';
        report(cls + " " + std::to_string(fe) + " getScore() is the last pair's", !scores.empty() && last == scores.back());
    }
    bool thrown = false;
    try {
        al.getAlignments(ptrs, kBand, 16u);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    try {
        al.getScores(ptrs, kBand, 16u);
        thrown = false;
    } catch (const std::runtime_error&) {
    }
    report(cls + " freeEnds 16 throws", thrown);
}

// freeEnds = 0 is the banded global form; substitution scoring has no ends-free form
template <typename Aligner>
static void check_banded(const std::string& cls, Aligner al, Ptrs& ptrs) {
    auto want = al.getAlignments(ptrs, kBand);
    auto got = al.getAlignments(ptrs, kBand, 0u);
    bool same = want.size() == got.size();
    for (size_t p = 0; same && p < want.size(); ++p) same = same_alignment(want[p], got[p]);
    report(cls + " freeEnds 0 equals getAlignments(pairs, band)", same && al.getScores(ptrs, kBand) == al.getScores(ptrs, kBand, 0u));
    al.setSubstitution([](char a, char b) { return a == b ? 2 : -1; });
    int thrown = 0;
    try {
        al.getAlignments(ptrs, kBand, 12u);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    try {
        al.getScores(ptrs, kBand, 12u);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    report(cls + " substitution scoring with free ends throws", thrown == 2);
}

int main() {
    uint64_t seed = 4242;
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
    seqs.push_back({mutate(window.substr(40, 60)), window});                 // a read in a window
    seqs.push_back({mutate(window.substr(0, 50)), window.substr(0, 110)});   // at the window's start
    seqs.push_back({other, mutate(other.substr(70)) + rnd(5)});              // two overlapping reads
    seqs.push_back({rnd(30), rnd(34)});                                      // unrelated
    seqs.push_back({rnd(7), Str()});                                         // an empty side
    seqs.push_back({Str(), rnd(3)});
    seqs.push_back({mutate(window.substr(100, 40)), window.substr(60)});     // a read at the window's end
    Ptrs ptrs;
    for (auto& p : seqs) ptrs.push_back({&p.first, &p.second});

    const ScoringSystem lin(-2, 2, -3), aff(-3, -1, 2, -3);
    print_class("NeedlemanWunschSA", NeedlemanWunschSA<Str, char, '-'>(lin), seqs, ptrs);
    print_class("HirschbergSA", HirschbergSA<Str, char, '-'>(lin), seqs, ptrs);
    print_class("GlobalGotohSA", GlobalGotohSA<Str, char, '-'>(aff), seqs, ptrs);
    check_banded("NeedlemanWunschSA", NeedlemanWunschSA<Str, char, '-'>(lin), ptrs);
    check_banded("GlobalGotohSA", GlobalGotohSA<Str, char, '-'>(aff), ptrs);
    return failures;
}
