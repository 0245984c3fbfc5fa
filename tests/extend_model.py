"""A plain-dict restatement of the banded X-drop extension semantics of include/seqalib_hip.h
(sa_align_batch_banded_extend) for both algorithms, and a numpy anti-diagonal version of its fill for bands
of thousands of diagonals.  The band is the seeded band round diagonal 0; the recurrence, borders and walk
are those of tests/seeded_model.py with free_ends = 0; new are the end cell (the last row-major maximum
over (0, 0) and the interior cells the sweep computed) and the drop rule, which the sweep applies step by
step.  Written from the header text, not from the kernels."""
import numpy as np

from util import scoring_fields

NW, GLOBAL_GOTOH, HIRSCHBERG = 1, 3, 4
BORDER_XY = -10000
XDROP_OFF, XDROP_PERIOD = -1, 16
FLAG_DROPPED = 32


def extend_band(m, n, w):
    """(lo', hi', tend): the band clipped to the matrix and its last step t = i + j - lo'."""
    lo, hi = max(-w, -m), min(w, n)
    return lo, hi, min(m + n, 2 * m + hi, 2 * n - lo) - lo


def step_cells(m, n, lo, hi, t):
    """The in-band cells (i, j) of step t, in row order."""
    out = []
    for c in range(t & 1, hi - lo + 1, 2):
        if (t - c) % 2 == 0:
            i = (t - c) // 2
            j = i + lo + c
            if 0 <= i <= m and 0 <= j <= n:
                out.append((i, j))
    return sorted(out)


def extend_model(algo, args, s1, s2, w, xdrop, lut=None, trace=None):
    """(score, end_i, end_j, start_i, start_j, ops, dropped, stop_step) of the extension's sweep and walk.
    stop_step: the step whose checkpoint stopped the pair, or None.  trace: a list that receives
    (t, best, recent) of every checkpoint whose window held an interior cell."""
    assert xdrop >= XDROP_OFF
    g, ma, mi, go, ge, allow = scoring_fields(args)
    affine = algo == GLOBAL_GOTOH
    assert affine or algo in (NW, HIRSCHBERG)
    m, n = len(s1), len(s2)
    lo, hi, tend = extend_band(m, n, w)

    def match(i, j):
        return bool(lut[s1[i - 1], s2[j - 1]]) if lut is not None else s1[i - 1] == s2[j - 1]

    def diag(i, j):   # the diagonal neighbour is on the same diagonal: always in band
        v = match(i, j)
        return v, (M[i - 1, j - 1] + (ma if v else mi)) if (v or allow) else None

    M, X, Y = {}, {}, {}   # linear: M is H, X / Y stay empty
    best, end = 0, (0, 0)   # the candidate (0, 0) holds 0
    recent, stop_step = None, None
    for t in range(tend + 1):
        for i, j in step_cells(m, n, lo, hi, t):
            if i == 0 or j == 0:
                M[i, j] = 0 if i + j == 0 else (go + (i + j) * ge if affine else (i + j) * g)
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
            v = M[i, j] = max(cands)
            if (v, (i, j)) > (best, end):   # the last row-major maximum
                best, end = v, (i, j)
            recent = v if recent is None else max(recent, v)
        if t % XDROP_PERIOD == XDROP_PERIOD - 1 and t < tend:   # a checkpoint
            if recent is not None:
                if trace is not None:
                    trace.append((t, best, recent))
                if xdrop >= 0 and best - recent > xdrop:
                    stop_step = t
                    break
            recent = None

    end_i, end_j = end
    ops = bytearray()
    i, j, typ = end_i, end_j, 0
    while i > 0 or j > 0:
        if j == 0:
            ops.append(ord("U"))
            i -= 1
            continue
        if i == 0:
            ops.append(ord("L"))
            j -= 1
            continue
        assert (i, j) in M, ("the walk left the computed cells", i, j)
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
    return best, end_i, end_j, i, j, bytes(ops), stop_step is not None, stop_step


NONE = -(10 ** 15)   # "no such cell" in the numpy fill: below every sum of real scores


def extend_fill_np(algo, args, s1, s2, w, xdrop, lut=None, trace=None):
    """(score, end_i, end_j, dropped, stop_step) of the same sweep, one numpy operation per step: V[c] holds
    the latest cell of diagonal c = j - i - lo', so at step t the diagonals of t's parity hold step t - 2
    (the diagonal neighbour) and the others step t - 1 (c + 1: the upper neighbour, c - 1: the left one).
    trace: as extend_model's."""
    assert xdrop >= XDROP_OFF
    g, ma, mi, go, ge, allow = scoring_fields(args)
    affine = algo == GLOBAL_GOTOH
    assert affine or algo in (NW, HIRSCHBERG)
    a = np.frombuffer(bytes(s1) + b"\0", dtype=np.uint8)   # (the pad: what a border cell's unused term indexes)
    b = np.frombuffer(bytes(s2) + b"\0", dtype=np.uint8)
    m, n = len(s1), len(s2)
    lo, hi, tend = extend_band(m, n, w)
    B = hi - lo + 1
    M = np.full(B + 2, NONE, dtype=np.int64)   # slot c + 1; slots 0 and B + 1 stay NONE
    X, Y = M.copy(), M.copy()
    cs = np.arange(B)
    best, end = 0, (0, 0)
    recent, stop_step = None, None
    for t in range(tend + 1):
        c = cs[(cs & 1) == (t & 1)]
        i = (t - c) // 2
        j = i + lo + c
        ok = (i >= 0) & (i <= m) & (j >= 0) & (j <= n)
        c, i, j = c[ok], i[ok], j[ok]
        if c.size:
            inner = (i >= 1) & (j >= 1)
            ii, jj = np.maximum(i, 1), np.maximum(j, 1)
            mt = lut[a[ii - 1], b[jj - 1]].astype(bool) if lut is not None else a[ii - 1] == b[jj - 1]
            dg, up, left = M[c + 1], M[c + 2], M[c]
            d = np.where(mt, dg + ma, dg + mi if allow else NONE)
            if affine:
                x = np.maximum(up + go + ge, X[c + 2] + ge)
                y = np.maximum(left + go + ge, Y[c] + ge)
            else:
                x, y = up + g, left + g
            x = np.where(up > NONE // 2, x, NONE)
            y = np.where(left > NONE // 2, y, NONE)
            v = np.maximum(np.maximum(d, x), y)
            k = i + j
            bord = np.where(k == 0, 0, go + k * ge if affine else k * g)
            M[c + 1] = np.where(inner, v, bord)
            if affine:
                X[c + 1] = np.where(inner, x, BORDER_XY)
                Y[c + 1] = np.where(inner, y, BORDER_XY)
            if inner.any():
                vi = v[inner]
                top = int(vi.max())
                r = int(i[inner][vi == top].max())   # within a step the largest row is the last in row-major order
                cell = (r, t + lo - r)
                if (top, cell) > (best, end):
                    best, end = top, cell
                recent = top if recent is None else max(recent, top)
        if t % XDROP_PERIOD == XDROP_PERIOD - 1 and t < tend:
            if recent is not None and trace is not None:
                trace.append((t, best, recent))
            if recent is not None and xdrop >= 0 and best - recent > xdrop:
                stop_step = t
                break
            recent = None
    return best, end[0], end[1], stop_step is not None, stop_step
