"""A NumPy float16 model of the 4-op scaled-f16 Smith-Waterman cell (sa_fill_so2.hip X4) and of its
sampling rule, against an integer Smith-Waterman (SASmithWaterman.h:89-117), on the CPU.

The cell holds H / 2048 and F = max(H + Gap, 0) / 2048 in f16:
    H(i, j) = max(H(i-1, j-1) + s, F(i-1, j), F(i, j-1)),   F = clamp(H + Gap, 0, 1)
so every value below 2048 is exact (k 2^-11, k < 2048, is an f16).  The fill flags a pair for the
int32 re-run when (sampled maximum - 6 Gap) > 2000, where the sampled cells are those of rows
3 mod 4 at wavefront steps 3 mod 4 (step = column + row / R), rows past m (substitution 0) and
columns past n (substitution -128) included.  Claim ("The 4-op cell"): a pair is either
exact in every cell or flagged, and a pair whose true maximum is below 2000 + 6 Gap is exact.

Cases: identical pairs with 3 point mutations whose true maxima run from about 1,912 to 2,294, at
six f16-eligible scorings (gap, match, mismatch).
"""
import numpy as np
import pytest

SCORINGS = [(-1, 1, -1), (-2, 2, -3), (-8, 8, -8), (-16, 4, -4), (-3, 1, -1), (-5, 4, -4)]
TARGETS = [1912, 1950, 1985, 2000, 2020, 2047, 2052, 2110, 2200, 2294]   # true maxima, about
RETRY_ABOVE, SLACK = 2000, 6    # kSo2F16RetryAbove, kSoSlack


def make_pair(seed, length):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, length).astype(np.int64)
    b = a.copy()
    for p in rng.choice(length, 3, replace=False):
        b[p] = (b[p] + 1 + rng.integers(0, 3)) % 4
    return a, b


def run_model(a, b, gap, match, mismatch):
    """Both recurrences over the anti-diagonals of the padded matrix.  Returns (true maximum, exact
    in every cell of the matrix, {R: sampled maximum of the f16 model as the integer the fill
    reports -- 2048 stands for any value that left [0, 1)})."""
    m, n = len(a), len(b)
    mp, np_ = m + 4, n + 4 + 3          # rows / columns past the matrix that a sampled cell may lie in
    f16 = np.float16
    sc = f16(2.0 ** -11)
    ap = np.concatenate([a, np.full(mp - m, 4)])          # 4: a row past m (substitution 0)
    bp = np.concatenate([b, np.full(np_ - n, 5)])         # 5: a column past n (substitution -128)
    tab_i = np.zeros((5, 6), np.int32)
    tab_i[:4, :4] = np.where(np.eye(4, dtype=bool), match, mismatch)
    tab_i[:, 5] = -128
    tab_i[4, :5] = 0
    tab_i[4, 5] = -128
    tab_f = (tab_i.astype(np.float32) * np.float32(2.0 ** -11)).astype(f16)
    assert (tab_f.astype(np.float64) * 2048 == tab_i).all()
    gf = f16(gap * 2.0 ** -11)
    assert float(gf) * 2048 == gap
    rows = np.arange(mp)
    # diagonal d holds cells (i, d - i); arrays are indexed by i + 1 (index 0: the top border)
    hf1 = np.zeros(mp + 1, f16); hf2 = np.zeros(mp + 1, f16); ff1 = np.zeros(mp + 1, f16)
    hi1 = np.zeros(mp + 1, np.int32); hi2 = np.zeros(mp + 1, np.int32)
    true_max, exact = 0, True
    samp = {16: f16(0), 32: f16(0)}
    for d in range(mp + np_ - 1):
        lo, hi = max(0, d - np_ + 1), min(mp - 1, d)      # rows of this diagonal
        i = rows[lo:hi + 1]
        j = d - i
        ai, bj = ap[i], bp[j]
        # integer cell
        hn_i = np.maximum(np.maximum(hi2[lo:hi + 1] + tab_i[ai, bj], 0),
                          np.maximum(hi1[lo:hi + 1], hi1[lo + 1:hi + 2]) + gap)
        # f16 cell: diagonal d - 2 at i - 1; F of the row above (d - 1 at i - 1) and of the left (d - 1 at i)
        dg = (hf2[lo:hi + 1] + tab_f[ai, bj]).astype(f16)
        hn_f = np.maximum(np.maximum(dg, ff1[lo:hi + 1]), ff1[lo + 1:hi + 2]).astype(f16)
        fn_f = np.clip((hn_f + gf).astype(f16), f16(0), f16(1)).astype(f16)
        inside = (i < m) & (j < n)
        if inside.any():
            true_max = max(true_max, int(hn_i[inside].max()))
            exact = exact and bool((hn_f[inside].astype(np.float64) * 2048 == hn_i[inside]).all())
        for R in samp:
            s = (i % 4 == 3) & ((j + i // R) % 4 == 3)
            if s.any():
                samp[R] = max(samp[R], hn_f[s].max())
        # shift: d - 1 -> d - 2, d -> d - 1 (cells outside this diagonal's rows are borders: 0)
        hf2, hi2 = hf1, hi1
        hf1 = np.zeros(mp + 1, f16); ff1 = np.zeros(mp + 1, f16); hi1 = np.zeros(mp + 1, np.int32)
        hf1[lo + 1:hi + 2] = hn_f
        ff1[lo + 1:hi + 2] = fn_f
        hi1[lo + 1:hi + 2] = hn_i
    sampled = {R: (int(round(float(v) * 2048)) if float(v) < 1.0 else 2048) for R, v in samp.items()}
    return true_max, exact, sampled


CASES = [(sc, t) for sc in SCORINGS for t in TARGETS]


@pytest.mark.parametrize("scoring,target", CASES)
def test_scaled_f16_cell_exact_or_flagged(scoring, target):
    gap, match, mismatch = scoring
    # 3 point mutations cost about 3 (match - mismatch) of the identical pair's length * match
    length = -(-(target + 3 * (match - mismatch)) // match)
    a, b = make_pair(1000 * match - gap + target, length)
    true_max, exact, sampled = run_model(a, b, gap, match, mismatch)
    assert 1800 <= true_max <= 2400, true_max
    for R, smax in sampled.items():
        flagged = smax - SLACK * gap > RETRY_ABOVE
        print(f"scoring {scoring} length {length} true max {true_max} R {R} sampled {smax} "
              f"exact {exact} flagged {flagged}")
        assert exact or flagged, (scoring, length, true_max, R, smax)
        if true_max < RETRY_ABOVE + SLACK * gap:
            assert exact and not flagged, (scoring, length, true_max, R, smax)
