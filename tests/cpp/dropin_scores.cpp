// Drop-in check of the score-only extensions of include/seqalib/: getScores() (all five DP classes)
// and getEndCells() (SmithWatermanSA, LocalGotohSA) must report, for every pair of a batch, what
// getScore() / getEndCell() report after getAlignment() of that pair alone -- for std::string
// sequences, std::vector<int> with a lambda match, and a batch with more than 256 distinct
// symbols (the match-bitmap path).  Prints one line per check, "ok ..." or "FAIL ...", and
// returns the number of failures.
#include <cstdint>
#include <functional>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "seqalib/SequenceAlignment.h"

static uint64_t lcg(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

static int failures = 0;

static void report(const std::string& what, bool ok) {
    std::cout << (ok ? "ok " : "FAIL ") << what << '\n';
    if (!ok) ++failures;
}

template <typename C>
static std::vector<std::pair<C*, C*>> pointers(std::vector<std::pair<C, C>>& seqs) {
    std::vector<std::pair<C*, C*>> out;
    for (auto& p : seqs) out.push_back({&p.first, &p.second});
    return out;
}

// getScores of the batch against getScore() after getAlignment() pair by pair (a fresh aligner
// each, so both see the same member history); getScore() after getScores is the last pair's
template <typename Aligner, typename C>
static void check_scores(const std::string& what, Aligner batch, Aligner single, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    const std::vector<ScoreSystemType> got = batch.getScores(ptrs);
    std::vector<ScoreSystemType> want;
    for (auto& p : seqs) {
        single.getAlignment(p.first, p.second);
        want.push_back(single.getScore());
    }
    report(what + " getScores", got == want);
    report(what + " getScore after getScores", !got.empty() && batch.getScore() == got.back());
}

template <typename Aligner, typename C>
static void check_cells(const std::string& what, Aligner batch, Aligner single, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    const std::vector<std::pair<size_t, size_t>> got = batch.getEndCells(ptrs);
    std::vector<std::pair<size_t, size_t>> want;
    for (auto& p : seqs) {
        single.getAlignment(p.first, p.second);
        want.push_back(single.getEndCell());
    }
    report(what + " getEndCells", got == want);
    report(what + " getEndCell after getEndCells", !got.empty() && batch.getEndCell() == got.back());
}

template <typename C, typename Ty, Ty Blank, typename Fn>
static void check_all(const std::string& kind, std::vector<std::pair<C, C>>& seqs, Fn fn) {
    const ScoringSystem lin(-1, 2, -1), sw(-1, 1, -1), aff(-3, -1, 1, -1);
    using SW = SmithWatermanSA<C, Ty, Blank, Fn>;
    using NW = NeedlemanWunschSA<C, Ty, Blank, Fn>;
    using LG = LocalGotohSA<C, Ty, Blank, Fn>;
    using GG = GlobalGotohSA<C, Ty, Blank, Fn>;
    using HB = HirschbergSA<C, Ty, Blank, Fn>;
    check_scores(kind + " SmithWatermanSA", SW(sw, fn), SW(sw, fn), seqs);
    check_cells(kind + " SmithWatermanSA", SW(sw, fn), SW(sw, fn), seqs);
    check_scores(kind + " NeedlemanWunschSA", NW(lin, fn), NW(lin, fn), seqs);
    check_scores(kind + " LocalGotohSA", LG(aff, fn), LG(aff, fn), seqs);
    check_cells(kind + " LocalGotohSA", LG(aff, fn), LG(aff, fn), seqs);
    check_scores(kind + " GlobalGotohSA", GG(aff, fn), GG(aff, fn), seqs);
    check_scores(kind + " HirschbergSA", HB(lin, fn), HB(lin, fn), seqs);
}

int main() {
    uint64_t seed = 2024;
    // std::string over 20 letters: related and unrelated pairs, an empty side, sizes across the
    // small-call limit and a LocalGotoh hack size (60 x 57)
    const std::string letters = "ACDEFGHIKLMNPQRSTVWY";
    auto rnd_str = [&](int len) {
        std::string s;
        for (int k = 0; k < len; ++k) s.push_back(letters[lcg(seed) % letters.size()]);
        return s;
    };
    auto mutate = [&](const std::string& a) {
        std::string b;
        for (char c : a) {
            const int r = (int)(lcg(seed) % 100);
            if (r < 10) b.push_back(letters[lcg(seed) % letters.size()]);
            else if (r < 13) continue;
            else b.push_back(c);
        }
        return b;
    };
    std::vector<std::pair<std::string, std::string>> strs;
    const int lens[][2] = {{11, 8}, {300, 280}, {60, 57}, {700, 90}, {33, 1000}, {257, 129}, {1, 1}, {520, 515}};
    for (auto& l : lens) {
        std::string a = rnd_str(l[0]);
        std::string b = (l[0] > 200 && l[1] > 200) ? mutate(a) : rnd_str(l[1]);
        strs.push_back({a, b});
    }
    strs.push_back({rnd_str(40), std::string()});   // an empty side, after a pair (member history)
    strs.push_back({rnd_str(90), rnd_str(75)});
    check_all<std::string, char, '-'>("string", strs, std::function<bool(char, char)>(nullptr));

    // std::vector<int> with a lambda match ("same residue mod 50"), <= 256 distinct symbols
    auto rnd_vec = [&](int len, int vocab) {
        std::vector<int> v;
        for (int k = 0; k < len; ++k) v.push_back(1 + (int)(lcg(seed) % (uint64_t)vocab));
        return v;
    };
    std::vector<std::pair<std::vector<int>, std::vector<int>>> vecs;
    for (auto& l : lens) vecs.push_back({rnd_vec(l[0], 200), rnd_vec(l[1], 200)});
    std::function<bool(int, int)> mod50 = [](int x, int y) { return x % 50 == y % 50; };
    check_all<std::vector<int>, int, 0>("vector<int> lambda", vecs, mod50);

    // more than 256 distinct symbols: the match-bitmap path, with a "within 1" predicate
    std::vector<std::pair<std::vector<int>, std::vector<int>>> wide;
    for (auto& l : lens) {
        std::vector<int> a = rnd_vec(l[0], 3000), b = rnd_vec(l[1], 3000);
        for (size_t k = 0; k < a.size() && k < b.size(); ++k)
            if (k % 3) b[k] = a[k] + (int)(k % 2);
        wide.push_back({a, b});
    }
    std::function<bool(int, int)> near = [](int x, int y) { return x - y <= 1 && y - x <= 1; };
    check_all<std::vector<int>, int, 0>("vector<int> wide", wide, near);
    return failures;
}
