// seqalib/SAGlobalGotoh.h — GlobalGotohSA (affine-gap global alignment) on the MI355X engine.
// Reference behaviour restated: SAGlobalGotoh.h:33-459 (borders M = GO + i*GE, Ix = Iy = -10000
// :75-88, fill :98-126, traceback from (m, n) with j == 0 -> up, i == 0 -> left :235-422).
#pragma once

template <typename ContainerType, typename Ty = typename ContainerType::value_type, Ty Blank = Ty(0),
          typename MatchFnTy = std::function<bool(Ty, Ty)>>
class GlobalGotohSA : public SequenceAligner<ContainerType, Ty, Blank, MatchFnTy> {
    using BaseType = SequenceAligner<ContainerType, Ty, Blank, MatchFnTy>;
    ScoreSystemType LastScore = 0;

public:
    static ScoringSystem getDefaultScoring() { return ScoringSystem(-1, 2, -1); }

    GlobalGotohSA() : BaseType(getDefaultScoring(), nullptr) {}
    GlobalGotohSA(ScoringSystem Scoring, MatchFnTy Match = nullptr) : BaseType(Scoring, Match) {}

    // Extension: substitution scoring (sa_align_batch_matrix).  Once set, getAlignment(s), getScores
    // and getEndCells score a diagonal move with Fn(Seq1 symbol, Seq2 symbol) instead of the scoring's
    // match / mismatch; the match function still decides Entry::IsMatchingPair.  A batch may use at
    // most 64 distinct symbols and scores must fit 16 bits (std::runtime_error otherwise); an empty
    // function returns to match / mismatch scoring.  The banded forms (getAlignments / getScores /
    // getEndCells with a band) then take the banded matrix calls (sa_align_batch_banded_matrix).
    void setSubstitution(std::function<ScoreSystemType(Ty, Ty)> Fn) { BaseType::setSubstitutionFn(std::move(Fn)); }

    virtual AlignedSequence<Ty, Blank> getAlignment(ContainerType& Seq1, ContainerType& Seq2) {
        std::vector<std::pair<ContainerType*, ContainerType*>> one{{&Seq1, &Seq2}};
        return std::move(getAlignments(one)[0]);
    }

    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty, Blank>(*this, pairs, res);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    // Extension: the getScore() of every pair in one GPU pass with no traceback (no AlignedSequence is
    // built, no op buffer allocated); getScore() afterwards returns the last pair's.
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty>(*this, pairs, res);
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }

    // Extension: banded GlobalGotoh (sa_align_batch_banded_affine / sa_score_batch_banded_affine): only
    // the cells within `band` diagonals of each pair's corner-to-corner corridor, O((m + n) * band) work
    // and memory per pair.  With band >= max(m, n) the result is getAlignments(pairs).  Needs
    // gap_extend <= 0 and at most 2048 band diagonals inside a pair's matrix.  Byte-sized symbols, or
    // batches of at most 256 distinct symbols; a band that does not fit 32 bits throws
    // std::runtime_error.  After setSubstitution() the banded forms go to the banded matrix calls
    // (sa_align_batch_banded_matrix / sa_score_batch_banded_matrix): the same band with the diagonal
    // term Fn(a, b), at most 64 distinct symbols in a batch.
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty, Blank>(*this, pairs, res,
                                                                                                 seqalib::detail::band_of(band));
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty>(*this, pairs, res,
                                                                                      seqalib::detail::band_of(band));
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }

    // Extension: ends-free (semi-global) banded GlobalGotoh (sa_align_batch_banded_ends_free /
    // sa_score_batch_banded_ends_free): as the banded forms, but the heads / tails of the sequences that
    // freeEnds names (an OR of SA_FREE_SEQ1_BEGIN, SA_FREE_SEQ1_END, SA_FREE_SEQ2_BEGIN, SA_FREE_SEQ2_END)
    // stay unaligned at no cost -- a read in a window: SEQ2_BEGIN | SEQ2_END with the read as Seq1; two
    // overlapping reads: SEQ1_BEGIN | SEQ2_END.  The aligned core is padded to both whole sequences the
    // way forceGlobal pads a local alignment; getScore() is the core's score.  Not combinable with
    // setSubstitution() (std::runtime_error).
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band, unsigned freeEnds) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty, Blank>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                                (long long)freeEnds);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band,
                                           unsigned freeEnds) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                       (long long)freeEnds);
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }

    // Extension: seeded ends-free banded GlobalGotoh (sa_align_batch_banded_seeded / sa_score_batch_banded_seeded): the
    // ends-free forms above with pair p's band `band` diagonals either side of its seed diagonal diags[p]
    // (k = j - i: a read, Seq1, that starts at position s of its window lies on k = s), so the band's width
    // does not grow with the longer sequence.  std::runtime_error after setSubstitution(), when diags.size()
    // is not pairs.size(), and for every status but SA_OK (a band with no legal begin or end among them),
    // with the engine's message.
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          const std::vector<int32_t>& diags, size_t band, unsigned freeEnds) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty, Blank>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                                (long long)freeEnds, &diags);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                           const std::vector<int32_t>& diags, size_t band, unsigned freeEnds) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                       (long long)freeEnds, &diags);
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }

    // Extension: banded X-drop extension (sa_align_batch_banded_extend / sa_score_batch_banded_extend): banded GlobalGotoh
    // anchored at the first symbols of both sequences, inside `band` diagonals either side of the main one,
    // ending at the cell of its best score; a pair whose score falls more than xdrop below its best is
    // abandoned there (SA_XDROP_OFF: never).  The aligned prefix is padded with the unextended tails the way
    // forceGlobal pads a local alignment; getScore() is the extension's score.  Names of their own, because
    // (pairs, band, int) would collide with the ends-free overload.  std::runtime_error after setSubstitution()
    // and for every status but SA_OK (xdrop < -1 among them).
    std::vector<AlignedSequence<Ty, Blank>> getExtensions(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band, int xdrop) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty, Blank>(
            *this, pairs, res, seqalib::detail::band_of(band), seqalib::detail::kNoFreeEnds, nullptr, (long long)xdrop);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    std::vector<ScoreSystemType> getExtensionScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band,
                                                    int xdrop) {
        std::vector<ScoreSystemType> out;
        for (auto& r : extensionResults(pairs, band, xdrop)) out.push_back(r.score);
        return out;
    }
    // (end_i, end_j) of every pair: the last row-major cell holding the extension's maximum, (0, 0) if none is positive.
    std::vector<std::pair<size_t, size_t>> getExtensionEndCells(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                                size_t band, int xdrop) {
        std::vector<std::pair<size_t, size_t>> out;
        for (auto& r : extensionResults(pairs, band, xdrop)) out.emplace_back((size_t)r.end_i, (size_t)r.end_j);
        return out;
    }

    ScoreSystemType getScore() const { return LastScore; }

private:
    std::vector<sa_result> extensionResults(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band, int xdrop) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_GLOBAL_GOTOH, GlobalGotohSA, ContainerType, Ty>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                     seqalib::detail::kNoFreeEnds, nullptr, (long long)xdrop);
        if (!res.empty()) LastScore = res.back().score;
        return res;
    }
};
