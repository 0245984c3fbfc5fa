// seqalib/SASmithWaterman.h — SmithWatermanSA (linear-gap local alignment) on the MI355X engine.
// Reference behaviour restated: SASmithWaterman.h:20-366 (fill :89-117, max cell = last
// row-major maximum :110, traceback :220-339, forceGlobal :337, default scoring (-1,1,-1) :352).
#pragma once

template <typename ContainerType, typename Ty = typename ContainerType::value_type, Ty Blank = Ty(0),
          typename MatchFnTy = std::function<bool(Ty, Ty)>>
class SmithWatermanSA : public SequenceAligner<ContainerType, Ty, Blank, MatchFnTy> {
    using BaseType = SequenceAligner<ContainerType, Ty, Blank, MatchFnTy>;
    // The reference keeps the max cell in members that survive between calls (:14-16); an empty
    // input re-uses them in forceGlobal.  Kept here with the same lifetime.
    size_t MaxRow = 0;
    size_t MaxCol = 0;
    ScoreSystemType MaxScore = std::numeric_limits<ScoreSystemType>::min();

    AlignedSequence<Ty, Blank> emptyResult(ContainerType& Seq1, ContainerType& Seq2) {
        AlignedSequence<Ty, Blank> r;
        MaxScore = std::numeric_limits<ScoreSystemType>::min();
        BaseType::forceGlobal(Seq1, Seq2, r, 0, 0, (int)MaxRow, (int)MaxCol);
        return r;
    }

public:
    static ScoringSystem getDefaultScoring() { return ScoringSystem(-1, 1, -1); }

    SmithWatermanSA() : BaseType(getDefaultScoring(), nullptr) {}
    SmithWatermanSA(ScoringSystem Scoring, MatchFnTy Match = nullptr) : BaseType(Scoring, Match) {}

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

    // Batch extension: one GPU pass over many pairs (configs 3/5 of BASELINE.json).
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        return alignBatch(pairs, seqalib::detail::kNoBand);
    }
    // Extension: banded SW (sa_align_batch_banded): only the cells within `band` diagonals of each
    // pair's corner-to-corner corridor; the end cell is the last in-band maximum.  With
    // band >= max(m, n) the result is getAlignments(pairs).  Byte-sized symbols, or batches of at most
    // 256 distinct symbols; others throw std::runtime_error.  getScores / getEndCells likewise.
    std::vector<AlignedSequence<Ty, Blank>> getAlignments(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                          size_t band) {
        return alignBatch(pairs, seqalib::detail::band_of(band));
    }
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs, size_t band) {
        std::vector<std::pair<size_t, size_t>> cells;
        return scoreBatch(pairs, cells, seqalib::detail::band_of(band));
    }
    std::vector<std::pair<size_t, size_t>> getEndCells(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                       size_t band) {
        std::vector<std::pair<size_t, size_t>> cells;
        scoreBatch(pairs, cells, seqalib::detail::band_of(band));
        return cells;
    }

private:
    std::vector<AlignedSequence<Ty, Blank>> alignBatch(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                                       long long band) {
        std::vector<std::pair<ContainerType*, ContainerType*>> work;
        for (auto& p : pairs)
            if (p.first->size() && p.second->size()) work.push_back(p);
        std::vector<sa_result> res;
        std::vector<AlignedSequence<Ty, Blank>> done;
        if (!work.empty()) done = seqalib::detail::run<SA_SW, SmithWatermanSA, ContainerType, Ty, Blank>(*this, work, res, band);
        std::vector<AlignedSequence<Ty, Blank>> out;
        out.reserve(pairs.size());
        size_t k = 0;
        for (auto& p : pairs) {
            if (p.first->size() && p.second->size()) {
                MaxRow = res[k].end_i;
                MaxCol = res[k].end_j;
                MaxScore = res[k].score;
                out.push_back(std::move(done[k++]));
            } else {
                out.push_back(emptyResult(*p.first, *p.second));
            }
        }
        return out;
    }

public:
    // Extensions: scores / end cells of every pair in one GPU pass with no traceback (no
    // AlignedSequence is built, no op buffer allocated).  The members move as in getAlignments: a
    // pair with an empty side scores INT_MIN and keeps the end cell of the pair before it.
    std::vector<ScoreSystemType> getScores(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<std::pair<size_t, size_t>> cells;
        return scoreBatch(pairs, cells);
    }
    std::vector<std::pair<size_t, size_t>> getEndCells(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs) {
        std::vector<std::pair<size_t, size_t>> cells;
        scoreBatch(pairs, cells);
        return cells;
    }

    // Extensions (the reference keeps these private): score and end cell of the last alignment.
    ScoreSystemType getScore() const { return MaxScore; }
    std::pair<size_t, size_t> getEndCell() const { return {MaxRow, MaxCol}; }

private:
    std::vector<ScoreSystemType> scoreBatch(const std::vector<std::pair<ContainerType*, ContainerType*>>& pairs,
                                            std::vector<std::pair<size_t, size_t>>& cells,
                                            long long band = seqalib::detail::kNoBand) {
        std::vector<std::pair<ContainerType*, ContainerType*>> work;
        for (auto& p : pairs)
            if (p.first->size() && p.second->size()) work.push_back(p);
        std::vector<sa_result> res;
        seqalib::detail::run_scores<SA_SW, SmithWatermanSA, ContainerType, Ty>(*this, work, res, band);
        std::vector<ScoreSystemType> out;
        out.reserve(pairs.size());
        cells.clear();
        cells.reserve(pairs.size());
        size_t k = 0;
        for (auto& p : pairs) {
            if (p.first->size() && p.second->size()) {
                MaxRow = res[k].end_i;
                MaxCol = res[k].end_j;
                MaxScore = res[k++].score;
            } else {
                MaxScore = std::numeric_limits<ScoreSystemType>::min();
            }
            out.push_back(MaxScore);
            cells.emplace_back(MaxRow, MaxCol);
        }
        return out;
    }
};
