// Drop-in check of the extension doors of include/seqalib/ (sa_align_batch_banded_extend /
// sa_score_batch_banded_extend): getExtensions(pairs, band, xdrop), getExtensionScores and
// getExtensionEndCells on NeedlemanWunschSA, HirschbergSA and GlobalGotohSA, for std::string sequences.
// Each class
//   extends, at band 6, a fixed batch (a pair that diverges after a related head, a pair related
//   throughout, an unrelated pair, two pairs with an empty side) under xdrop 8 and SA_XDROP_OFF and prints,
//   per pair, the inputs and the three printed rows (Seq1 row, bars, Seq2 row), then the scores and the
//   end cells of the batch;
//   must throw std::runtime_error for xdrop = -2 (with the engine's message) and (where there is one)
//   after setSubstitution().
// tests/test_dropin_extend.py recomputes the printed rows, scores and end cells with the Python classes.
// Output: "pair <class> <xdrop> <index>" followed by "s1 ..", "s2 ..", "r0 ..", "bars ..", "r1 .." lines
// (each value between '[' and ']'), "scores <class> <xdrop> ..", "ends <class> <xdrop> i j ..", and
// "ok ..." / "FAIL ..." lines; returns the number of failures.
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
static void print_class(const std::string& cls, Aligner al, std::vector<std::pair<Str, Str>>& seqs) {
    Ptrs ptrs;
    for (auto& s : seqs) ptrs.push_back({&s.first, &s.second});
    for (int xdrop : {8, SA_XDROP_OFF}) {
        auto got = al.getExtensions(ptrs, kBand, xdrop);
        const ScoreSystemType last = al.getScore();
        for (size_t q = 0; q < ptrs.size(); ++q) {
            std::string r0, bars, r1;
            for (auto e = got[q].begin(); e != got[q].end(); ++e) {
                r0.push_back(e->get(0));
                bars.push_back(e->match() ? '|' : ' ');
                r1.push_back(e->get(1));
            }
            std::cout << "pair " << cls << ' ' << xdrop << ' ' << q << "\ns1 [" << *ptrs[q].first << "]\ns2 [" << *ptrs[q].second
                      << "]\nr0 [" << r0 << "]\nbars [" << bars << "]\nr1 [" << r1 << "]\n";
        }
        const std::vector<ScoreSystemType> scores = al.getExtensionScores(ptrs, kBand, xdrop);
        std::cout << "scores " << cls << ' ' << xdrop;
        for (auto s : scores) std::cout << ' ' << s;
        std::cout << '\n';
        report(cls + " " + std::to_string(xdrop) + " getScore() is the last pair's", !scores.empty() && last == scores.back());
        std::cout << "ends " << cls << ' ' << xdrop;
        for (auto& e : al.getExtensionEndCells(ptrs, kBand, xdrop)) std::cout << ' ' << e.first << ' ' << e.second;
        std::cout << '\n';
    }
    report(cls + " xdrop -2 throws", throws([&] { al.getExtensions(ptrs, kBand, -2); }, "xdrop") &&
                                         throws([&] { al.getExtensionScores(ptrs, kBand, -2); }, "xdrop") &&
                                         throws([&] { al.getExtensionEndCells(ptrs, kBand, -2); }, "xdrop"));
    Ptrs none;
    report(cls + " an empty batch gives nothing", al.getExtensions(none, kBand, 8).empty() && al.getExtensionScores(none, kBand, 8).empty());
}

template <typename Aligner>
static void check_substitution(const std::string& cls, Aligner al, std::vector<std::pair<Str, Str>>& seqs) {
    Ptrs ptrs;
    for (auto& s : seqs) ptrs.push_back({&s.first, &s.second});
    al.setSubstitution([](char a, char b) { return a == b ? 2 : -1; });
    report(cls + " substitution scoring with an extension throws",
           throws([&] { al.getExtensions(ptrs, kBand, 8); }) && throws([&] { al.getExtensionScores(ptrs, kBand, 8); }));
}

int main() {
    uint64_t seed = 5151;
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
    const Str head = rnd(40), whole = rnd(120);
    seqs.push_back({head + rnd(90), mutate(head) + rnd(90)});   // 0: diverges after a related head
    seqs.push_back({whole, mutate(whole)});                     // 1: related throughout
    seqs.push_back({rnd(50), rnd(45)});                         // 2: unrelated
    seqs.push_back({rnd(7), Str()});                            // 3: an empty side
    seqs.push_back({Str(), rnd(3)});                            // 4

    const ScoringSystem lin(-2, 1, -3), aff(-4, -1, 1, -3);
    print_class("NeedlemanWunschSA", NeedlemanWunschSA<Str, char, '-'>(lin), seqs);
    print_class("HirschbergSA", HirschbergSA<Str, char, '-'>(lin), seqs);
    print_class("GlobalGotohSA", GlobalGotohSA<Str, char, '-'>(aff), seqs);
    check_substitution("NeedlemanWunschSA", NeedlemanWunschSA<Str, char, '-'>(lin), seqs);
    check_substitution("GlobalGotohSA", GlobalGotohSA<Str, char, '-'>(aff), seqs);
    return failures;
}
