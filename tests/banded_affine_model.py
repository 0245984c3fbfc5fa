"""A plain-dict restatement of the banded affine semantics of include/seqalib_hip.h
(sa_align_batch_banded_affine): only in-band cells exist, a term that would read a missing cell is no
candidate, a comparison against a missing value is false.  The walk is the reference's state machine
(oracle/sa_oracle.c:align_gotoh) over dictionaries; it asserts that it never dead-ends and never
emits 'u' / 'l' (gap_extend <= 0)."""
from util import scoring_fields

BORDER_XY = -10000
LOCAL, GLOBAL = 2, 3   # SA_LOCAL_GOTOH, SA_GLOBAL_GOTOH


def banded_affine_model(algo, args, s1, s2, w, lut=None):
    """(score, end_i, end_j, start_i, start_j, ops) of the banded Gotoh recurrence and walk."""
    _, ma, mi, go, ge, allow = scoring_fields(args)
    assert ge <= 0
    m, n = len(s1), len(s2)
    lo, hi = min(0, n - m) - w, max(0, n - m) + w
    local = algo == LOCAL

    def match(i, j):
        return bool(lut[s1[i - 1], s2[j - 1]]) if lut is not None else s1[i - 1] == s2[j - 1]

    def diag(i, j):   # the diagonal neighbour is on the same diagonal: always in band
        v = match(i, j)
        return v, (M[i - 1, j - 1] + (ma if v else mi)) if (v or allow) else None

    M, X, Y = {}, {}, {}
    best, maxr, maxc = None, 0, 0
    for i in range(m + 1):
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 or j == 0:
                M[i, j] = 0 if local or i + j == 0 else go + (i + j) * ge
                X[i, j] = Y[i, j] = BORDER_XY
                continue
            cands = []
            _, d = diag(i, j)
            if d is not None:
                cands.append(d)
            if (i - 1, j) in M:
                x = M[i - 1, j] + go + ge
                if (i - 1, j) in X:
                    x = max(x, X[i - 1, j] + ge)
                X[i, j] = x
                cands.append(x)
            if (i, j - 1) in M:
                y = M[i, j - 1] + go + ge
                if (i, j - 1) in Y:
                    y = max(y, Y[i, j - 1] + ge)
                Y[i, j] = y
                cands.append(y)
            if local:
                cands.append(0)
            h = M[i, j] = max(cands)
            if local and (best is None or h >= best):
                best, maxr, maxc = h, i, j
    ops = bytearray()
    typ = 0
    i, j = (maxr, maxc) if local else (m, n)
    while i > 0 or j > 0:
        if local and (i <= 0 or j <= 0):
            break
        if i > 0 and j > 0 and typ == 0:
            v, d = diag(i, j)
            s = d if not local else (max(d, 0) if d is not None else 0)
            if s is not None and M[i, j] == s:
                if local and s <= 0:
                    break
                ops.append(ord(("M" if v else "S") if (v or allow) else "X"))
                i, j = i - 1, j - 1
                continue
        if i > 0:
            if j == 0:
                ops.append(ord("U"))
                i -= 1
                continue
            if (i, j) in X:
                mup = M[i - 1, j] + go + ge
                if local:
                    mup = max(mup, 0)
                if typ == 1 and (i - 1, j) in X and X[i, j] == X[i - 1, j] + ge:
                    ops.append(ord("U"))
                    i -= 1
                    continue
                if typ == 1 and X[i, j] == mup:
                    assert not (local and mup <= 0), "'u'"
                    ops.append(ord("U"))
                    typ = 0
                    i -= 1
                    continue
                if typ == 0 and M[i, j] == X[i, j]:
                    typ = 1
                    continue
        if j > 0:
            if i == 0:
                ops.append(ord("L"))
                j -= 1
                continue
            if (i, j) in Y:
                mleft = M[i, j - 1] + go + ge
                if local:
                    mleft = max(mleft, 0)
                if typ == 2 and (i, j - 1) in Y and Y[i, j] == Y[i, j - 1] + ge:
                    ops.append(ord("L"))
                    j -= 1
                    continue
                if typ == 2 and Y[i, j] == mleft:
                    assert not (local and mleft <= 0), "'l'"
                    ops.append(ord("L"))
                    typ = 0
                    j -= 1
                    continue
                if typ == 0 and M[i, j] == Y[i, j]:
                    typ = 2
                    continue
        raise AssertionError(("dead end", algo, args, w, i, j, typ))
    if local:
        return (M[maxr, maxc], maxr, maxc, i, j, bytes(ops))
    return M[m, n], m, n, i, j, bytes(ops)


def affine_rescore(args, ops):
    """Score of an op stream: match / mismatch per diagonal op, gap_open + len * gap_extend per maximal
    run of one gap letter."""
    _, ma, mi, go, ge, _ = scoring_fields(args)
    total, k = 0, 0
    while k < len(ops):
        c = ops[k:k + 1]
        if c == b"M":
            total += ma
            k += 1
        elif c == b"S":
            total += mi
            k += 1
        else:
            assert c in (b"U", b"L"), c
            e = k
            while e < len(ops) and ops[e:e + 1] == c:
                e += 1
            total += go + (e - k) * ge
            k = e
    return total
