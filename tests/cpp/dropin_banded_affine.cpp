// Drop-in check of the banded affine extensions of include/seqalib/: on LocalGotohSA and GlobalGotohSA,
// getAlignments(pairs, band) with a whole-matrix band must equal getAlignments(pairs) entry for entry
// (no pair has a size the LocalGotoh size hack fires on: the banded calls are the raw path),
// getScores(pairs, 8) must equal the scores collected from getAlignments(pairs, 8) pair by pair
// (LocalGotohSA: getEndCells likewise) -- for std::string sequences and std::vector<int> with a lambda
// match over at most 256 distinct symbols -- a batch with more than 256 distinct symbols must throw
// std::runtime_error, and so must a band that does not fit 32 bits.  Prints one line per check,
// "ok ..." or "FAIL ...", and returns the number of failures.
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

template <typename A>
static bool same(std::vector<A>& x, std::vector<A>& y) {
    if (x.size() != y.size()) return false;
    for (size_t p = 0; p < x.size(); ++p) {
        if (x[p].Data.size() != y[p].Data.size()) return false;
        auto a = x[p].begin();
        auto b = y[p].begin();
        for (; a != x[p].end(); ++a, ++b)
            if (a->get(0) != b->get(0) || a->get(1) != b->get(1) || a->match() != b->match()) return false;
    }
    return true;
}

template <typename Aligner, typename C>
static void check_whole(const std::string& what, Aligner plain, Aligner banded, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    auto want = plain.getAlignments(ptrs);
    auto got = banded.getAlignments(ptrs, (size_t)4096);
    report(what + " whole-matrix band", same(got, want));
}

// getScores(pairs, 8) against getScore() after getAlignments({pair}, 8), pair by pair
template <typename Aligner, typename C>
static void check_scores(const std::string& what, Aligner batch, Aligner single, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    const std::vector<ScoreSystemType> got = batch.getScores(ptrs, (size_t)8);
    std::vector<ScoreSystemType> want;
    for (auto& p : ptrs) {
        std::vector<std::pair<C*, C*>> one{p};
        single.getAlignments(one, (size_t)8);
        want.push_back(single.getScore());
    }
    report(what + " getScores band 8", got == want);
}

template <typename Aligner, typename C>
static void check_cells(const std::string& what, Aligner batch, Aligner single, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    const std::vector<std::pair<size_t, size_t>> got = batch.getEndCells(ptrs, (size_t)8);
    std::vector<std::pair<size_t, size_t>> want;
    for (auto& p : ptrs) {
        std::vector<std::pair<C*, C*>> one{p};
        single.getAlignments(one, (size_t)8);
        want.push_back(single.getEndCell());
    }
    report(what + " getEndCells band 8", got == want);
}

template <typename C, typename Ty, Ty Blank, typename Fn>
static void check_all(const std::string& kind, std::vector<std::pair<C, C>>& seqs, Fn fn) {
    const ScoringSystem aff(-3, -1, 1, -1);
    using LG = LocalGotohSA<C, Ty, Blank, Fn>;
    using GG = GlobalGotohSA<C, Ty, Blank, Fn>;
    check_whole(kind + " LocalGotohSA", LG(aff, fn), LG(aff, fn), seqs);
    check_whole(kind + " GlobalGotohSA", GG(aff, fn), GG(aff, fn), seqs);
    check_scores(kind + " LocalGotohSA", LG(aff, fn), LG(aff, fn), seqs);
    check_scores(kind + " GlobalGotohSA", GG(aff, fn), GG(aff, fn), seqs);
    check_cells(kind + " LocalGotohSA", LG(aff, fn), LG(aff, fn), seqs);
}

// a band that does not fit 32 bits (SIZE_MAX included) is refused, never taken for "no band"
template <typename Aligner, typename C>
static void check_huge_band(const std::string& what, Aligner al, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    int thrown = 0;
    for (size_t band : {(size_t)SIZE_MAX, (size_t)1 << 32, (size_t)1 << 63}) {
        try {
            al.getAlignments(ptrs, band);
        } catch (const std::runtime_error&) {
            ++thrown;
        }
        try {
            al.getScores(ptrs, band);
        } catch (const std::runtime_error&) {
            ++thrown;
        }
    }
    report(what + " huge band throws", thrown == 6);
}

template <typename Aligner, typename C>
static void check_throws(const std::string& what, Aligner al, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    bool a = false, s = false;
    try {
        al.getAlignments(ptrs, (size_t)8);
    } catch (const std::runtime_error& e) {
        a = std::string(e.what()).find("256") != std::string::npos;
    }
    try {
        al.getScores(ptrs, (size_t)8);
    } catch (const std::runtime_error& e) {
        s = std::string(e.what()).find("256") != std::string::npos;
    }
    report(what + " wide batch throws", a && s);
}

int main() {
    uint64_t seed = 777;
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
    const int lens[][2] = {{11, 8}, {300, 280}, {64, 57}, {700, 90}, {33, 1000}, {257, 129}, {1, 1}, {520, 515}};
    for (auto& l : lens) {
        std::string a = rnd_str(l[0]);
        std::string b = (l[0] > 200 && l[1] > 200) ? mutate(a) : rnd_str(l[1]);
        strs.push_back({a, b});
    }
    strs.push_back({rnd_str(40), std::string()});   // an empty side, after a pair (member history)
    strs.push_back({rnd_str(90), rnd_str(75)});
    check_all<std::string, char, '-'>("string", strs, std::function<bool(char, char)>(nullptr));
    for (auto& p : strs) {   // (the whole-matrix comparison needs unhacked sizes and at most 2048 diagonals)
        const size_t m = p.first.size(), n = p.second.size();
        if ((m == 314 && n == 288) || (m == 60 && n == 57) || (m == 61 && n == 58) || m + n + 1 > 2048) {
            report("input sizes", false);
            return failures;
        }
    }
    check_huge_band("string LocalGotohSA", LocalGotohSA<std::string, char, '-'>(ScoringSystem(-3, -1, 1, -1)), strs);
    check_huge_band("string GlobalGotohSA", GlobalGotohSA<std::string, char, '-'>(ScoringSystem(-3, -1, 1, -1)), strs);

    auto rnd_vec = [&](int len, int vocab) {
        std::vector<int> v;
        for (int k = 0; k < len; ++k) v.push_back(1 + (int)(lcg(seed) % (uint64_t)vocab));
        return v;
    };
    std::vector<std::pair<std::vector<int>, std::vector<int>>> vecs;
    for (auto& l : lens) vecs.push_back({rnd_vec(l[0], 200), rnd_vec(l[1], 200)});
    std::function<bool(int, int)> mod50 = [](int x, int y) { return x % 50 == y % 50; };
    check_all<std::vector<int>, int, 0>("vector<int> lambda", vecs, mod50);

    std::vector<std::pair<std::vector<int>, std::vector<int>>> wide;
    for (auto& l : lens) wide.push_back({rnd_vec(l[0], 3000), rnd_vec(l[1], 3000)});
    std::function<bool(int, int)> near = [](int x, int y) { return x - y <= 1 && y - x <= 1; };
    check_throws("vector<int> wide LocalGotohSA",
                 LocalGotohSA<std::vector<int>, int, 0, std::function<bool(int, int)>>(ScoringSystem(-3, -1, 1, -1), near), wide);
    check_throws("vector<int> wide GlobalGotohSA",
                 GlobalGotohSA<std::vector<int>, int, 0, std::function<bool(int, int)>>(ScoringSystem(-3, -1, 1, -1), near), wide);
    return failures;
}
