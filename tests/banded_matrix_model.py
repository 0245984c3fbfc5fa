"""A plain-dict restatement of the banded matrix semantics of include/seqalib_hip.h
(sa_align_batch_banded_matrix): the banded recurrences and walks of test_gpu_banded.banded_model
(SW / NW) and banded_affine_model (LocalGotoh / GlobalGotoh) with the diagonal term S[a][b] in place
of match / mismatch.  Only in-band cells exist, a term that would read a missing cell is no
candidate, a comparison against a missing value is false; mismatches are always allowed, so 'X' never
appears.  The walks assert that they never dead-end and never emit 'u' / 'l'.
tests/test_banded_matrix_model.py pins it against those two models (two-valued S) and against
submat_model.model_align (whole-matrix band): the model is only as good as those pins.

banded_matrix_model(algo, gaps, S, s1, s2, w, match=None) -> (score, end_i, end_j, start_i, start_j, ops).
gaps: the gap penalty (SW / NW) or (gap_open, gap_extend) (Gotoh).  S: a callable on two byte values
or a 256 x 256 table.  match: the op label ('M' when match(a, b), else 'S'), a callable, a 256 x 256
table, or None for byte equality.
"""
INT_MIN = -(2 ** 31)
SW, NW, LOCAL_GOTOH, GLOBAL_GOTOH = 0, 1, 2, 3
BORDER_XY = -10000


def _fn(t, default):
    if t is None:
        return default
    if callable(t):
        return t
    rows = [list(map(int, r)) for r in t]
    return lambda a, b: rows[a][b]


def _linear(sw, g, sub, lab, s1, s2, w):
    m, n = len(s1), len(s2)
    lo, hi = min(0, n - m) - w, max(0, n - m) + w
    H = {}
    best, maxr, maxc = None, 0, 0
    for i in range(m + 1):
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 or j == 0:
                H[i, j] = 0 if sw else (i + j) * g
                continue
            cands = [H[i - 1, j - 1] + sub(s1[i - 1], s2[j - 1])]   # the diagonal neighbour is always in band
            if (i - 1, j) in H:
                cands.append(H[i - 1, j] + g)
            if (i, j - 1) in H:
                cands.append(H[i, j - 1] + g)
            if sw:
                cands.append(0)
            h = H[i, j] = max(cands)
            if sw and (best is None or h >= best):
                best, maxr, maxc = h, i, j
    ops = bytearray()
    if sw:
        i, j = (maxr, maxc) if m and n else (0, 0)
        while i > 0 and j > 0:
            s = max(H[i - 1, j - 1] + sub(s1[i - 1], s2[j - 1]), 0)
            if H[i, j] == s:
                if s == 0:
                    break
                ops.append(ord("M" if lab(s1[i - 1], s2[j - 1]) else "S"))
                i, j = i - 1, j - 1
            elif (i - 1, j) in H and H[i, j] == H[i - 1, j] + g:
                if H[i - 1, j] + g <= 0:
                    break
                ops.append(ord("U"))
                i -= 1
            else:
                assert (i, j - 1) in H and H[i, j] == H[i, j - 1] + g, ("dead end", i, j)
                if H[i, j - 1] + g <= 0:
                    break
                ops.append(ord("L"))
                j -= 1
        return (best if m and n else INT_MIN), maxr, maxc, i, j, bytes(ops)
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and H[i, j] == H[i - 1, j - 1] + sub(s1[i - 1], s2[j - 1]):
            ops.append(ord("M" if lab(s1[i - 1], s2[j - 1]) else "S"))
            i, j = i - 1, j - 1
            continue
        if i > 0 and (i - 1, j) in H and H[i, j] == H[i - 1, j] + g:
            ops.append(ord("U"))
            i -= 1
        else:
            assert j > 0 and (i, j - 1) in H and H[i, j] == H[i, j - 1] + g, ("dead end", i, j)
            ops.append(ord("L"))
            j -= 1
    return H[m, n], m, n, 0, 0, bytes(ops)


def _affine(local, go, ge, sub, lab, s1, s2, w):
    assert ge <= 0
    m, n = len(s1), len(s2)
    lo, hi = min(0, n - m) - w, max(0, n - m) + w
    M, X, Y = {}, {}, {}
    best, maxr, maxc = None, 0, 0
    for i in range(m + 1):
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 or j == 0:
                M[i, j] = 0 if local or i + j == 0 else go + (i + j) * ge
                X[i, j] = Y[i, j] = BORDER_XY
                continue
            cands = [M[i - 1, j - 1] + sub(s1[i - 1], s2[j - 1])]
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
            d = M[i - 1, j - 1] + sub(s1[i - 1], s2[j - 1])
            s = max(d, 0) if local else d
            if M[i, j] == s:
                if local and s <= 0:
                    break
                ops.append(ord("M" if lab(s1[i - 1], s2[j - 1]) else "S"))
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
        raise AssertionError(("dead end", local, go, ge, w, i, j, typ))
    if local:
        return M[maxr, maxc], maxr, maxc, i, j, bytes(ops)
    return M[m, n], m, n, i, j, bytes(ops)


def banded_matrix_model(algo, gaps, S, s1, s2, w, match=None):
    s1, s2 = bytes(s1), bytes(s2)
    S = _fn(S, None)
    match = _fn(match, lambda a, b: a == b)
    cs, cm = {}, {}

    def sub(a, b):   # S and match evaluated once per symbol pair
        if (a, b) not in cs:
            cs[a, b] = int(S(a, b))
        return cs[a, b]

    def lab(a, b):
        if (a, b) not in cm:
            cm[a, b] = bool(match(a, b))
        return cm[a, b]

    if algo in (SW, NW):
        return _linear(algo == SW, int(gaps), sub, lab, s1, s2, int(w))
    if algo in (LOCAL_GOTOH, GLOBAL_GOTOH):
        go, ge = gaps
        return _affine(algo == LOCAL_GOTOH, int(go), int(ge), sub, lab, s1, s2, int(w))
    raise ValueError(f"no model for algorithm {algo}")
