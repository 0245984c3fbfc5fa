// seqalib/SANeedlemanWunsch.h — NeedlemanWunschSA (linear-gap global alignment) on the MI355X engine.
// Reference behaviour restated: SANeedlemanWunsch.h:22-264 (borders i*Gap / j*Gap :59-62, fill
// :69-86, traceback from (m, n) diag > up > left :155-231, default scoring (-1,2,-1) :244-247).
#pragma once

template <typename ContainerType, typename Ty = typename ContainerType::value_type, Ty Blank = Ty(0),
          typename MatchFnTy = std::function<bool(Ty, Ty)>>
class NeedlemanWunschSA : public SequenceAligner<ContainerType, Ty, Blank, MatchFnTy> {
    using BaseType = SequenceAligner<ContainerType, Ty, Blank, MatchFnTy>;
    ScoreSystemType LastScore = 0;

public:
    static ScoringSystem getDefaultScoring() { return ScoringSystem(-1, 2, -1); }

    NeedlemanWunschSA() : BaseType(getDefaultScoring(), nullptr) {}
    NeedlemanWunschSA(ScoringSystem Scoring, MatchFnTy Match = nullptr) : BaseType(Scoring, Match) {}

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
        return alignBatch(pairs, seqalib::detail::kNoBand);
    }
    // Extension: banded NW (sa_align_batch_banded): only the cells within `band` diagonals of each
    // pair's corner-to-corner corridor, O((m + n) * band) work and memory per pair.  With
    // band >= max(m, n) the result is getAlignments(pairs).  Byte-sized symbols, or batches of at most
    // 256 distinct symbols; others throw std::runtime_error.
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band) {
        return alignBatch(pairs, seqalib::detail::band_of(band));
    }

    // Extension: the getScore() of every pair in one GPU pass with no traceback (no AlignedSequence is
    // built, no op buffer allocated); getScore() afterwards returns the last pair's.
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        return scoreBatch(pairs, seqalib::detail::kNoBand);
    }
    // Extension: the banded scores (sa_score_batch_banded), as getAlignments(pairs, band).
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band) {
        return scoreBatch(pairs, seqalib::detail::band_of(band));
    }

    // Extension: ends-free (semi-global) banded NW (sa_align_batch_banded_ends_free /
    // sa_score_batch_banded_ends_free): as the banded forms, but the heads / tails of the sequences that
    // freeEnds names (an OR of SA_FREE_SEQ1_BEGIN, SA_FREE_SEQ1_END, SA_FREE_SEQ2_BEGIN, SA_FREE_SEQ2_END)
    // stay unaligned at no cost -- a read in a window: SEQ2_BEGIN | SEQ2_END with the read as Seq1; two
    // overlapping reads: SEQ1_BEGIN | SEQ2_END.  The aligned core is padded to both whole sequences the
    // way forceGlobal pads a local alignment; getScore() is the core's score.  Not combinable with
    // setSubstitution() (std::runtime_error).
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band, unsigned freeEnds) {
        return alignBatch(pairs, seqalib::detail::band_of(band), (long long)freeEnds);
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band,
                                           unsigned freeEnds) {
        return scoreBatch(pairs, seqalib::detail::band_of(band), (long long)freeEnds);
    }

    // Extension: seeded ends-free banded NW (sa_align_batch_banded_seeded / sa_score_batch_banded_seeded): the
    // ends-free forms above with pair p's band `band` diagonals either side of its seed diagonal diags[p]
    // (k = j - i: a read, Seq1, that starts at position s of its window lies on k = s), so the band's width
    // does not grow with the longer sequence.  std::runtime_error after setSubstitution(), when diags.size()
    // is not pairs.size(), and for every status but SA_OK (a band with no legal begin or end among them),
    // with the engine's message.
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          const std::vector<int32_t>& diags, size_t band, unsigned freeEnds) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_NW, NeedlemanWunschSA, ContainerType, Ty, Blank>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                                (long long)freeEnds, &diags);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                           const std::vector<int32_t>& diags, size_t band, unsigned freeEnds) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_NW, NeedlemanWunschSA, ContainerType, Ty>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                       (long long)freeEnds, &diags);
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }

    // Extension: H[m][n] of the last alignment.
    ScoreSystemType getScore() const { return LastScore; }

    // Extension: banded X-drop extension (sa_align_batch_banded_extend / sa_score_batch_banded_extend): banded NW
    // anchored at the first symbols of both sequences, inside `band` diagonals either side of the main one,
    // ending at the cell of its best score; a pair whose score falls more than xdrop below its best is
    // abandoned there (SA_XDROP_OFF: never).  The aligned prefix is padded with the unextended tails the way
    // forceGlobal pads a local alignment; getScore() is the extension's score.  Names of their own, because
    // (pairs, band, int) would collide with the ends-free overload.  std::runtime_error after setSubstitution()
    // and for every status but SA_OK (xdrop < -1 among them).
    std::vector<AlignedSequence<Ty, Blank>> getExtensions(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band, int xdrop) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_NW, NeedlemanWunschSA, ContainerType, Ty, Blank>(
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

private:
    std::vector<sa_result> extensionResults(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band, int xdrop) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_NW, NeedlemanWunschSA, ContainerType, Ty>(*this, pairs, res, seqalib::detail::band_of(band),
                                                                     seqalib::detail::kNoFreeEnds, nullptr, (long long)xdrop);
        if (!res.empty()) LastScore = res.back().score;
        return res;
    }
    std::vector<AlignedSequence<Ty, Blank>> alignBatch(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                       long long band, long long free_ends = seqalib::detail::kNoFreeEnds) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_NW, NeedlemanWunschSA, ContainerType, Ty, Blank>(*this, pairs, res, band, free_ends);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
    std::vector<ScoreSystemType> scoreBatch(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, long long band,
                                            long long free_ends = seqalib::detail::kNoFreeEnds) {
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_NW, NeedlemanWunschSA, ContainerType, Ty>(*this, pairs, res, band, free_ends);
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        if (!res.empty()) LastScore = res.back().score;
        return out;
    }
};
