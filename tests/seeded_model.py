"""A plain-dict restatement of the seeded ends-free banded semantics of include/seqalib_hip.h
(sa_align_batch_banded_seeded) for both algorithms: the ends-free banded recurrence and walk of
tests/ends_free_model.py with the band lo = k - w, hi = k + w round the seed diagonal k, a legality
rule (the band must hold a legal begin and a legal end), and (m, n) a candidate only when it is in the
band.  Only in-band cells are visited, so the cost is O(min(m, n) * (2w + 1)) whatever the longer
sequence's length.  Written from the header text, not from the kernels."""
from util import scoring_fields

SEQ1_BEGIN, SEQ1_END, SEQ2_BEGIN, SEQ2_END = 1, 2, 4, 8   # SA_FREE_*
NW, GLOBAL_GOTOH, HIRSCHBERG = 1, 3, 4
BORDER_XY = -10000


def seeded_band(m, n, k, w):
    """(lo', hi'): the band clipped to the matrix."""
    return max(k - w, -m), min(k + w, n)


def seeded_legal(m, n, k, w, free_ends):
    """(has a legal begin, has a legal end); the calls take the pair only when both hold."""
    lo, hi = seeded_band(m, n, k, w)
    begin = lo <= 0 <= hi or bool(free_ends & SEQ2_BEGIN and hi >= 0) or bool(free_ends & SEQ1_BEGIN and lo <= 0)
    end = lo <= n - m <= hi or bool(free_ends & SEQ2_END and lo <= n - m) or bool(free_ends & SEQ1_END and hi >= n - m)
    return begin, end


def seeded_steps(m, n, k, w):
    """(tb, tend): the first (rounded down to even) and last sweep step t = i + j - lo' holding a cell."""
    lo, hi = seeded_band(m, n, k, w)
    return (max(-lo, 0) + max(-hi, 0)) & ~1, min(m + n, 2 * m + hi, 2 * n - lo) - lo


def _end_cell(V, m, n, free_ends):
    """The last candidate in row-major order holding the maximum: (m, n) when in band, with SEQ1_END
    every in-band (i, n), with SEQ2_END every in-band (m, j)."""
    cands = {(m, n)} & V.keys()
    if free_ends & SEQ1_END:
        cands |= {c for c in V if c[1] == n}
    if free_ends & SEQ2_END:
        cands |= {c for c in V if c[0] == m}
    best = max(V[c] for c in cands)
    return max(c for c in cands if V[c] == best)   # tuples order row-major


def seeded_model(algo, args, s1, s2, k, w, free_ends, lut=None):
    """(score, end_i, end_j, start_i, start_j, ops) of the seeded banded recurrence and walk."""
    assert 0 <= free_ends <= 15
    g, ma, mi, go, ge, allow = scoring_fields(args)
    affine = algo == GLOBAL_GOTOH
    assert affine or algo in (NW, HIRSCHBERG)
    m, n = len(s1), len(s2)
    assert -m <= k <= n
    assert seeded_legal(m, n, k, w, free_ends) == (True, True)
    lo, hi = k - w, k + w
    free_col0, free_row0 = bool(free_ends & SEQ1_BEGIN), bool(free_ends & SEQ2_BEGIN)

    def match(i, j):
        return bool(lut[s1[i - 1], s2[j - 1]]) if lut is not None else s1[i - 1] == s2[j - 1]

    def diag(i, j):   # the diagonal neighbour is on the same diagonal: always in band
        v = match(i, j)
        return v, (M[i - 1, j - 1] + (ma if v else mi)) if (v or allow) else None

    def border(i, j):
        if i + j == 0 or (free_col0 if j == 0 else free_row0):
            return 0
        return go + (i + j) * ge if affine else (i + j) * g

    M, X, Y = {}, {}, {}   # linear: M is H, X / Y stay empty
    for i in range(max(0, -hi), min(m, n - lo) + 1):   # the rows that hold an in-band cell
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 or j == 0:
                M[i, j] = border(i, j)
                if affine:
                    X[i, j] = Y[i, j] = BORDER_XY
                continue
            cands = []
            _, d = diag(i, j)
            if d is not None:
                cands.append(d)
            if (i - 1, j) in M:
                if affine:
                    x = M[i - 1, j] + go + ge
                    if (i - 1, j) in X:
                        x = max(x, X[i - 1, j] + ge)
                    X[i, j] = x
                else:
                    x = M[i - 1, j] + g
                cands.append(x)
            if (i, j - 1) in M:
                if affine:
                    y = M[i, j - 1] + go + ge
                    if (i, j - 1) in Y:
                        y = max(y, Y[i, j - 1] + ge)
                    Y[i, j] = y
                else:
                    y = M[i, j - 1] + g
                cands.append(y)
            M[i, j] = max(cands)

    end_i, end_j = _end_cell(M, m, n, free_ends)
    ops = bytearray()
    i, j, typ = end_i, end_j, 0
    while i > 0 or j > 0:
        if j == 0:
            if free_col0:
                break
            ops.append(ord("U"))
            i -= 1
            continue
        if i == 0:
            if free_row0:
                break
            ops.append(ord("L"))
            j -= 1
            continue
        assert (i, j) in M, ("the walk left the band", i, j)
        if typ == 0:
            v, d = diag(i, j)
            if d is not None and M[i, j] == d:
                ops.append(ord(("M" if v else "S") if (v or allow) else "X"))
                i, j = i - 1, j - 1
                continue
        if not affine:
            if (i - 1, j) in M and M[i, j] == M[i - 1, j] + g:
                ops.append(ord("U"))
                i -= 1
            else:
                assert (i, j - 1) in M and M[i, j] == M[i, j - 1] + g, ("dead end", i, j)
                ops.append(ord("L"))
                j -= 1
            continue
        # GlobalGotoh: the reference's state machine (type 0 in M, 1 vertical gap, 2 horizontal gap)
        if typ == 0:
            if (i, j) in X and M[i, j] == X[i, j]:
                typ = 1
            else:
                assert (i, j) in Y and M[i, j] == Y[i, j], ("dead end", i, j)
                typ = 2
        if typ == 1:
            ops.append(ord("U"))
            if not ((i - 1, j) in X and X[i, j] == X[i - 1, j] + ge):   # the extend term is tried first
                assert X[i, j] == M[i - 1, j] + go + ge
                typ = 0
            i -= 1
        else:
            ops.append(ord("L"))
            if not ((i, j - 1) in Y and Y[i, j] == Y[i, j - 1] + ge):
                assert Y[i, j] == M[i, j - 1] + go + ge
                typ = 0
            j -= 1
    return M[end_i, end_j], end_i, end_j, i, j, bytes(ops)
