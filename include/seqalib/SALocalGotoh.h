// seqalib/SALocalGotoh.h — LocalGotohSA (affine-gap local alignment, M/Ix/Iy) on the MI355X engine.
// Reference behaviour restated: SALocalGotoh.h:36-526 (borders M = 0, Ix = Iy = -10000 :77-90,
// fill :102-139, 3-state traceback :275-470, forceGlobal :473, and the size hack :484-488 that
// re-aligns (314,288), (60,57), (61,58) with StaticFuncs::useNW — done inside the engine).
#pragma once

template <typename ContainerType, typename Ty = typename ContainerType::value_type, Ty Blank = Ty(0),
          typename MatchFnTy = std::function<bool(Ty, Ty)>>
class LocalGotohSA : public SequenceAligner<ContainerType, Ty, Blank, MatchFnTy> {
    using BaseType = SequenceAligner<ContainerType, Ty, Blank, MatchFnTy>;
    size_t MaxRow = 0;
    size_t MaxCol = 0;
    ScoreSystemType MaxScore = 0;

public:
    // As in the reference (:509) this 3-argument default leaves the affine penalties unset (0 here).
    static ScoringSystem getDefaultScoring() { return ScoringSystem(-1, 2, -1); }

    LocalGotohSA() : BaseType(getDefaultScoring(), nullptr) {}
    LocalGotohSA(ScoringSystem Scoring, MatchFnTy Match = nullptr) : BaseType(Scoring, Match) {}

    // Extension: substitution scoring (sa_align_batch_matrix).  Once set, getAlignment(s), getScores
    // and getEndCells score a diagonal move with Fn(Seq1 symbol, Seq2 symbol) instead of the scoring's
    // match / mismatch; the match function still decides Entry::IsMatchingPair.  A batch may use at
    // most 64 distinct symbols and scores must fit 16 bits (std::runtime_error otherwise); an empty
    // function returns to match / mismatch scoring.  The banded forms (getAlignments / getScores /
    // getEndCells with a band) then take the banded matrix calls (sa_align_batch_banded_matrix).  The size-hack shapes
    // (314 x 288, 60 x 57, 61 x 58) are aligned as LocalGotoh like every other shape.
    void setSubstitution(std::function<ScoreSystemType(Ty, Ty)> Fn) { BaseType::setSubstitutionFn(std::move(Fn)); }

    virtual AlignedSequence<Ty, Blank> getAlignment(ContainerType& Seq1, ContainerType& Seq2) {
        std::vector<std::pair<ContainerType*, ContainerType*>> one{{&Seq1, &Seq2}};
        return std::move(getAlignments(one)[0]);
    }

    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_LOCAL_GOTOH, LocalGotohSA, ContainerType, Ty, Blank>(*this, pairs, res);
        if (!res.empty()) {
            MaxRow = res.back().end_i;
            MaxCol = res.back().end_j;
            MaxScore = res.back().score;
        }
        return out;
    }

    // Extensions: scores / end cells of every pair in one GPU pass with no traceback (no
    // AlignedSequence is built, no op buffer allocated); getScore() / getEndCell() afterwards return
    // the last pair's.  The three hack sizes report the NW score at (m, n), as getAlignment does.
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<sa_result> res;
        scoreBatch(pairs, res);
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        return out;
    }
    std::vector<std::pair<size_t, size_t>> getEndCells(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<sa_result> res;
        scoreBatch(pairs, res);
        std::vector<std::pair<size_t, size_t>> out;
        out.reserve(res.size());
        for (auto& r : res) out.emplace_back((size_t)r.end_i, (size_t)r.end_j);
        return out;
    }

    // Extension: banded LocalGotoh (sa_align_batch_banded_affine / sa_score_batch_banded_affine): only
    // the cells within `band` diagonals of each pair's corner-to-corner corridor, O((m + n) * band) work
    // and memory per pair; the end cell is the last in-band maximum.  This is the raw path: the size-hack
    // shapes are aligned as LocalGotoh like every other shape, so with band >= max(m, n) the result is
    // getAlignments(pairs) for every other shape.  Needs gap_extend <= 0 and at most 2048 band diagonals
    // inside a pair's matrix.  Byte-sized symbols, or batches of at most 256 distinct symbols; a band
    // that does not fit 32 bits throws std::runtime_error.  After setSubstitution() the banded forms go
    // to the banded matrix calls (sa_align_batch_banded_matrix / sa_score_batch_banded_matrix): the
    // same band with the diagonal term Fn(a, b), at most 64 distinct symbols in a batch.
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band) {
        std::vector<sa_result> res;
        auto out = seqalib::detail::run<SA_LOCAL_GOTOH, LocalGotohSA, ContainerType, Ty, Blank>(*this, pairs, res,
                                                                                               seqalib::detail::band_of(band));
        if (!res.empty()) {
            MaxRow = res.back().end_i;
            MaxCol = res.back().end_j;
            MaxScore = res.back().score;
        }
        return out;
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band) {
        std::vector<sa_result> res;
        scoreBatch(pairs, res, seqalib::detail::band_of(band));
        std::vector<ScoreSystemType> out;
        out.reserve(res.size());
        for (auto& r : res) out.push_back(r.score);
        return out;
    }
    std::vector<std::pair<size_t, size_t>> getEndCells(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                       size_t band) {
        std::vector<sa_result> res;
        scoreBatch(pairs, res, seqalib::detail::band_of(band));
        std::vector<std::pair<size_t, size_t>> out;
        out.reserve(res.size());
        for (auto& r : res) out.emplace_back((size_t)r.end_i, (size_t)r.end_j);
        return out;
    }

    ScoreSystemType getScore() const { return MaxScore; }
    std::pair<size_t, size_t> getEndCell() const { return {MaxRow, MaxCol}; }

private:
    void scoreBatch(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, std::vector<sa_result>& res,
                    long long band = seqalib::detail::kNoBand) {
        seqalib::detail::run_scores<SA_LOCAL_GOTOH, LocalGotohSA, ContainerType, Ty>(*this, pairs, res, band);
        if (!res.empty()) {
            MaxRow = res.back().end_i;
            MaxCol = res.back().end_j;
            MaxScore = res.back().score;
        }
    }
};
