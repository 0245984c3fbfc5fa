"""Plain-Python model of the four aligners with a score function S(a, b) on the diagonal move.

oracle/sa_oracle.c has no table scoring, so this file restates its four recurrences and walks
(align_sw, align_nw, align_gotoh local / global, including the 'u' / 'l' ops of LocalGotoh) with the
term `match(a, b) ? match : mismatch` replaced by S(a, b); allow_mismatch is always on, so 'X' never
appears.  tests/test_submat_model.py pins it against the oracle with S = match / mismatch: the model
is only as good as that pin.

model_align(algo, gaps, S, s1, s2, match=None) -> dict(score, end_i, end_j, start_i, start_j, ops,
diverged).  gaps: the gap penalty (SW / NW) or (gap_open, gap_extend) (Gotoh).  S: a callable on two
byte values or a 256 x 256 table.  match: the op label ('M' when match(a, b), else 'S'), a callable,
a 256 x 256 table, or None for byte equality.  diverged: the LocalGotoh / GlobalGotoh walk found no
move (the reference loops forever there; the engine reports SA_FLAG_DIVERGED for LocalGotoh).
"""
INT_MIN = -(2 ** 31)
SW, NW, LOCAL_GOTOH, GLOBAL_GOTOH = 0, 1, 2, 3


def _fn(t, default):
    if t is None:
        return default
    if callable(t):
        return t
    rows = [list(map(int, r)) for r in t]
    return lambda a, b: rows[a][b]


def _terms(S, match, s1, s2):
    """sub[i][j] = S(s1[i], s2[j]) and lab[i][j] = match(s1[i], s2[j]), evaluated once per symbol pair."""
    S = _fn(S, None)
    match = _fn(match, lambda a, b: a == b)
    cs, cm = {}, {}
    sub, lab = [], []
    for a in s1:
        rs, rm = [], []
        for b in s2:
            k = (a, b)
            if k not in cs:
                cs[k] = int(S(a, b))
                cm[k] = bool(match(a, b))
            rs.append(cs[k])
            rm.append(cm[k])
        sub.append(rs)
        lab.append(rm)
    return sub, lab


def _sw(G, sub, lab, m, n):
    H = [[0] * (n + 1) for _ in range(m + 1)]
    best, maxr, maxc = INT_MIN, 0, 0
    for i in range(1, m + 1):
        Hi, Hu, si = H[i], H[i - 1], sub[i - 1]
        for j in range(1, n + 1):
            h = max(Hu[j - 1] + si[j - 1], Hu[j] + G, Hi[j - 1] + G, 0)
            Hi[j] = h
            if h >= best:
                best, maxr, maxc = h, i, j
    ops = bytearray()
    i, j = (maxr, maxc) if m and n else (0, 0)
    while i > 0 and j > 0:
        s = max(H[i - 1][j - 1] + sub[i - 1][j - 1], 0)
        if H[i][j] == s:
            if s == 0:
                break
            ops.append(ord("M" if lab[i - 1][j - 1] else "S"))
            i, j = i - 1, j - 1
            continue
        if H[i][j] == H[i - 1][j] + G:
            if H[i - 1][j] + G <= 0:
                break
            ops.append(ord("U"))
            i -= 1
        else:
            if H[i][j - 1] + G <= 0:
                break
            ops.append(ord("L"))
            j -= 1
    return dict(score=best if m and n else INT_MIN, end_i=maxr, end_j=maxc, start_i=i, start_j=j, ops=bytes(ops),
                diverged=False)


def _nw(G, sub, lab, m, n):
    H = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        H[i][0] = i * G
    for j in range(n + 1):
        H[0][j] = j * G
    for i in range(1, m + 1):
        Hi, Hu, si = H[i], H[i - 1], sub[i - 1]
        for j in range(1, n + 1):
            Hi[j] = max(Hu[j - 1] + si[j - 1], Hu[j] + G, Hi[j - 1] + G)
    ops = bytearray()
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and H[i][j] == H[i - 1][j - 1] + sub[i - 1][j - 1]:
            ops.append(ord("M" if lab[i - 1][j - 1] else "S"))
            i, j = i - 1, j - 1
            continue
        if i > 0 and H[i][j] == H[i - 1][j] + G:
            ops.append(ord("U"))
            i -= 1
        else:
            ops.append(ord("L"))
            j -= 1
    return dict(score=H[m][n], end_i=m, end_j=n, start_i=0, start_j=0, ops=bytes(ops), diverged=False)


def _gotoh(local, GO, GE, sub, lab, m, n):
    GOE = GO + GE
    M = [[0] * (n + 1) for _ in range(m + 1)]
    X = [[-10000] * (n + 1) for _ in range(m + 1)]
    Y = [[-10000] * (n + 1) for _ in range(m + 1)]
    if not local:
        for i in range(1, m + 1):
            M[i][0] = GO + i * GE
        for j in range(1, n + 1):
            M[0][j] = GO + j * GE
    best, maxr, maxc = INT_MIN, 0, 0
    for i in range(1, m + 1):
        Mi, Mu, Xi, Xu, Yi, si = M[i], M[i - 1], X[i], X[i - 1], Y[i], sub[i - 1]
        for j in range(1, n + 1):
            x = max(Mu[j] + GOE, Xu[j] + GE)
            y = max(Mi[j - 1] + GOE, Yi[j - 1] + GE)
            d = Mu[j - 1] + si[j - 1]
            h = max(d, x, y, 0) if local else max(d, x, y)
            Xi[j], Yi[j], Mi[j] = x, y, h
            if local and h >= best:
                best, maxr, maxc = h, i, j
    ops = bytearray()
    typ = 0
    diverged = False
    if local:
        i, j = maxr, maxc
        while i > 0 and j > 0:
            if typ == 0:
                s = max(M[i - 1][j - 1] + sub[i - 1][j - 1], 0)
                if M[i][j] == s:
                    if s <= 0:
                        break
                    ops.append(ord("M" if lab[i - 1][j - 1] else "S"))
                    i, j = i - 1, j - 1
                    continue
            mup = max(M[i - 1][j] + GOE, 0)
            xup = X[i - 1][j] + GE
            if X[i][j] == xup and typ == 1:
                ops.append(ord("U"))
                i -= 1
                continue
            if X[i][j] == mup and typ == 1:
                if mup <= 0:
                    ops.append(ord("u"))
                    break
                ops.append(ord("U"))
                typ = 0
                i -= 1
                continue
            if M[i][j] == X[i][j] and typ == 0:
                typ = 1
                continue
            mleft = max(M[i][j - 1] + GOE, 0)
            yleft = Y[i][j - 1] + GE
            if Y[i][j] == yleft and typ == 2:
                ops.append(ord("L"))
                j -= 1
                continue
            if Y[i][j] == mleft and typ == 2:
                if mleft <= 0:
                    ops.append(ord("l"))
                    break
                ops.append(ord("L"))
                typ = 0
                j -= 1
                continue
            if M[i][j] == Y[i][j] and typ == 0:
                typ = 2
                continue
            diverged = True
            break
        return dict(score=M[maxr][maxc], end_i=maxr, end_j=maxc, start_i=i, start_j=j, ops=bytes(ops),
                    diverged=diverged)
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and typ == 0 and M[i][j] == M[i - 1][j - 1] + sub[i - 1][j - 1]:
            ops.append(ord("M" if lab[i - 1][j - 1] else "S"))
            i, j = i - 1, j - 1
            continue
        if i > 0:
            if j == 0:
                ops.append(ord("U"))
                i -= 1
                continue
            if X[i][j] == X[i - 1][j] + GE and typ == 1:
                ops.append(ord("U"))
                i -= 1
                continue
            if X[i][j] == M[i - 1][j] + GOE and typ == 1:
                ops.append(ord("U"))
                typ = 0
                i -= 1
                continue
            if M[i][j] == X[i][j] and typ == 0:
                typ = 1
                continue
        if j > 0:
            if i == 0:
                ops.append(ord("L"))
                j -= 1
                continue
            if Y[i][j] == Y[i][j - 1] + GE and typ == 2:
                ops.append(ord("L"))
                j -= 1
                continue
            if Y[i][j] == M[i][j - 1] + GOE and typ == 2:
                ops.append(ord("L"))
                typ = 0
                j -= 1
                continue
            if M[i][j] == Y[i][j] and typ == 0:
                typ = 2
                continue
        diverged = True
        break
    return dict(score=M[m][n], end_i=m, end_j=n, start_i=i, start_j=j, ops=bytes(ops), diverged=diverged)


def model_align(algo, gaps, S, s1, s2, match=None):
    s1, s2 = bytes(s1), bytes(s2)
    m, n = len(s1), len(s2)
    sub, lab = _terms(S, match, s1, s2)
    if algo == SW:
        return _sw(int(gaps), sub, lab, m, n)
    if algo == NW:
        return _nw(int(gaps), sub, lab, m, n)
    go, ge = gaps
    if algo == LOCAL_GOTOH:
        return _gotoh(True, int(go), int(ge), sub, lab, m, n)
    if algo == GLOBAL_GOTOH:
        return _gotoh(False, int(go), int(ge), sub, lab, m, n)
    raise ValueError(f"no model for algorithm {algo}")
