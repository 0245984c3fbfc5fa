// Drop-in check of setSubstitution() combined with a band on the four DP aligners of include/seqalib/
// (sa_align_batch_banded_matrix / sa_score_batch_banded_matrix): for std::string sequences (equality
// labels) and std::vector<int> sequences (a lambda match that labels pairs), each class
//   aligns a fixed batch at a whole-matrix band and compares it entry for entry with getAlignments(pairs)
//   (the unbanded matrix call), scores included;
//   aligns it at band 8 and prints, per pair, the inputs and the aligned rows, then getScores(pairs, 8)
//   (SW / LocalGotoh: getEndCells(pairs, 8)) of the batch.
// tests/test_dropin_banded_matrix.py recomputes the band-8 output with the Python model from the
// printed inputs.  A batch with more than 64 distinct symbols must throw std::runtime_error naming the
// limit, with a band as without.
// Output: "pair <kind> <class> <index>" followed by "s1 ..", "s2 ..", "rows .." lines (symbols as
// integers; a row entry is a:b:m), "scores <kind> <class> ..", "cells <kind> <class> ..", and
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
static const size_t kNarrow = 8, kWhole = 4096;

static void report(const std::string& what, bool ok) {
    std::cout << (ok ? "ok " : "FAIL ") << what << '\n';
    if (!ok) ++failures;
}

// The score rules (restated in tests/test_dropin_banded_matrix.py): asymmetric, positive off the diagonal.
static int score_char(char a, char b) {
    const int x = (unsigned char)a, y = (unsigned char)b;
    return x == y ? 5 + x % 3 : (x * 7 + y * 3) % 11 - 6;
}
static int score_int(int x, int y) { return x == y ? 6 : (x * 5 + y) % 9 - 5; }

template <typename C>
static std::vector<std::pair<C*, C*>> pointers(std::vector<std::pair<C, C>>& seqs) {
    std::vector<std::pair<C*, C*>> out;
    for (auto& p : seqs) out.push_back({&p.first, &p.second});
    return out;
}

template <typename C>
static void print_seq(const char* tag, const C& s) {
    std::cout << tag;
    for (auto v : s) std::cout << ' ' << (int)v;
    std::cout << '\n';
}

template <typename A>
static bool same_alignment(A& x, A& y) {
    if (x.Data.size() != y.Data.size()) return false;
    auto q = y.begin();
    for (auto e = x.begin(); e != x.end(); ++e, ++q)
        if (e->get(0) != q->get(0) || e->get(1) != q->get(1) || e->match() != q->match()) return false;
    return true;
}

template <typename Aligner, typename C>
static void run_class(const std::string& kind, const std::string& cls, Aligner al, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    // a whole-matrix band is the unbanded matrix call
    auto full = al.getAlignments(ptrs);
    auto whole = al.getAlignments(ptrs, kWhole);
    bool same = full.size() == whole.size();
    for (size_t p = 0; same && p < full.size(); ++p) same = same_alignment(full[p], whole[p]);
    report(kind + " " + cls + " whole-matrix band equals getAlignments(pairs)", same);
    report(kind + " " + cls + " whole-matrix band scores", al.getScores(ptrs) == al.getScores(ptrs, kWhole));
    // a narrow band, for the model
    auto got = al.getAlignments(ptrs, kNarrow);
    for (size_t p = 0; p < seqs.size(); ++p) {
        std::cout << "pair " << kind << ' ' << cls << ' ' << p << '\n';
        print_seq("s1", seqs[p].first);
        print_seq("s2", seqs[p].second);
        std::cout << "rows";
        for (auto e = got[p].begin(); e != got[p].end(); ++e)
            std::cout << ' ' << (int)e->get(0) << ':' << (int)e->get(1) << ':' << (e->match() ? 1 : 0);
        std::cout << '\n';
    }
    std::cout << "scores " << kind << ' ' << cls;
    for (auto s : al.getScores(ptrs, kNarrow)) std::cout << ' ' << s;
    std::cout << '\n';
}

template <typename Aligner, typename C>
static void print_cells(const std::string& kind, const std::string& cls, Aligner al, std::vector<std::pair<C, C>>& seqs) {
    auto ptrs = pointers(seqs);
    report(kind + " " + cls + " whole-matrix band end cells", al.getEndCells(ptrs) == al.getEndCells(ptrs, kWhole));
    std::cout << "cells " << kind << ' ' << cls;
    for (auto& c : al.getEndCells(ptrs, kNarrow)) std::cout << ' ' << c.first << ',' << c.second;
    std::cout << '\n';
}

template <typename C, typename Ty, Ty Blank, typename Fn, typename Sub>
static void run_all(const std::string& kind, std::vector<std::pair<C, C>>& seqs, Fn fn, Sub sub) {
    const ScoringSystem lin(-2, 1, -1), aff(-4, -1, 1, -1);
    SmithWatermanSA<C, Ty, Blank, Fn> sw(lin, fn);
    NeedlemanWunschSA<C, Ty, Blank, Fn> nw(lin, fn);
    LocalGotohSA<C, Ty, Blank, Fn> lg(aff, fn);
    GlobalGotohSA<C, Ty, Blank, Fn> gg(aff, fn);
    sw.setSubstitution(sub);
    nw.setSubstitution(sub);
    lg.setSubstitution(sub);
    gg.setSubstitution(sub);
    run_class(kind, "SmithWatermanSA", sw, seqs);
    run_class(kind, "NeedlemanWunschSA", nw, seqs);
    run_class(kind, "LocalGotohSA", lg, seqs);
    run_class(kind, "GlobalGotohSA", gg, seqs);
    print_cells(kind, "SmithWatermanSA", sw, seqs);
    print_cells(kind, "LocalGotohSA", lg, seqs);
}

template <typename Aligner, typename C>
static void check_throws(const std::string& what, Aligner al, std::vector<std::pair<C, C>>& seqs) {
    al.setSubstitution(score_int);
    auto ptrs = pointers(seqs);
    bool a = false, s = false;
    try {
        al.getAlignments(ptrs, kNarrow);
    } catch (const std::runtime_error& e) {
        a = std::string(e.what()).find("64") != std::string::npos;
    }
    try {
        al.getScores(ptrs, kNarrow);
    } catch (const std::runtime_error& e) {
        s = std::string(e.what()).find("64") != std::string::npos;
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
    // (second length 0: a mutated copy of the first sequence; 60 x 57 is a LocalGotoh size-hack shape:
    // substitution scoring aligns it as LocalGotoh, banded or not)
    const int lens[][2] = {{11, 8}, {120, 0}, {60, 57}, {200, 33}, {1, 1}, {70, 150}, {300, 0}};
    std::vector<std::pair<std::string, std::string>> strs;
    for (auto& l : lens) {
        std::string a = rnd_str(l[0]);
        strs.push_back({a, l[1] ? rnd_str(l[1]) : mutate(a)});
    }
    run_all<std::string, char, '-'>("string", strs, std::function<bool(char, char)>(nullptr), score_char);

    auto rnd_vec = [&](int len, int vocab) {
        std::vector<int> v;
        for (int k = 0; k < len; ++k) v.push_back(1 + (int)(lcg(seed) % (uint64_t)vocab));
        return v;
    };
    std::vector<std::pair<std::vector<int>, std::vector<int>>> vecs;
    for (auto& l : lens) vecs.push_back({rnd_vec(l[0], 40), rnd_vec(l[1] ? l[1] : l[0] - 7, 40)});
    std::function<bool(int, int)> mod10 = [](int x, int y) { return x % 10 == y % 10; };
    run_all<std::vector<int>, int, 0>("vector<int>", vecs, mod10, score_int);

    std::vector<std::pair<std::vector<int>, std::vector<int>>> wide;
    for (auto& l : lens) wide.push_back({rnd_vec(l[0] + 40, 100), rnd_vec(l[1] + 40, 100)});
    check_throws("vector<int> wide NeedlemanWunschSA",
                 NeedlemanWunschSA<std::vector<int>, int, 0, std::function<bool(int, int)>>(ScoringSystem(-1, 2, -1), mod10), wide);
    check_throws("vector<int> wide LocalGotohSA",
                 LocalGotohSA<std::vector<int>, int, 0, std::function<bool(int, int)>>(ScoringSystem(-3, -1, 1, -1), mod10), wide);
    return failures;
}
