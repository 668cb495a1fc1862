"""The rules of the affine X-drop extension in Python, twice.

extend() is the banded extender itself: section 3o's DP under the derived costs, anti-diagonal by anti-diagonal in
the doubled score D = a (i + j) - H', with the stop rule, the end cell, the bits per cell and the traceback that
follows the bits alone. It is what the device must reproduce byte for byte: states, score, ends and flag.

plain_best() shares nothing with it: the three max-recurrences of the score definition over the full matrix, without
costs, band or bits; score_of() re-prices a state string. replay() is oracle_affine's."""
import numpy as np

from oracle_affine import INF, _ACTG, _bytes, cigar, matches, replay  # noqa: F401

NO_TOP = -(1 << 30)
MAX_BAND = 511
MAX_XDROP = 1 << 20
DEFAULT = (2, 4, 4, 2)


def in_range(a, x, o, e, B, X):
    return (a >= 1 and x >= 0 and o >= 0 and e >= 1 and a + x <= 127 and o <= 127 and a + 2 * e <= 255
            and 0 <= B <= MAX_BAND and -1 <= X <= MAX_XDROP)


def a_max(n, m, B):
    return min(n + m, 2 * min(n, m) + B)


def stride(B):
    return (((2 * B + 3) >> 1) + 3) & ~3


def bits_bytes(n, m, B):
    return ((a_max(n, m, B) + 1) * stride(B) + 255) & ~255 if n + m < 1 << 21 else 0


NO_RESULT = dict(states=None, score=-1, query_end=-1, target_end=-1, dropped=0)


def extend(Q, T, a=2, x=4, o=4, e=2, B=64, X=200):
    """dict(states (forward order; None: no result), score, query_end, target_end, dropped)"""
    assert in_range(a, x, o, e, B, X)
    q, t = _bytes(Q), _bytes(T)
    n, m = len(q), len(t)
    if n + m >= 1 << 21:
        return dict(NO_RESULT)
    xx, oo, ee = 2 * (a + x), 2 * o, a + 2 * e
    lo, hi, W = -B, B, 2 * B + 1
    tt = _ACTG[(t >> 1) & 3]
    H1, E1, F1 = (np.full(W + 2, INF, np.int64) for _ in range(3))
    H2 = np.full(W + 2, INF, np.int64)
    H1[1 - lo] = 0
    rows = {}
    best, end, top_before, dropped = 0, (0, 0), 0, 0  # end = (anti-diagonal, diagonal)
    for A in range(1, a_max(n, m, B) + 1):
        dmin, dmax = max(lo, A - 2 * n, -A), min(hi, A, 2 * m - A)
        dmin += (dmin - A) & 1
        dmax -= (dmax - A) & 1
        Hn, En, Fn = (np.full(W + 2, INF, np.int64) for _ in range(3))
        top = NO_TOP
        if dmin <= dmax:
            d = np.arange(dmin, dmax + 1, 2)
            k = d - lo + 1
            i, j = (A - d) >> 1, (A + d) >> 1
            hl, el, hu, fu, hd = H1[k - 1], E1[k - 1], H1[k + 1], F1[k + 1], H2[k]
            eext = (el < INF) & (el + ee <= hl + oo + ee)
            ev = np.where(eext, el + ee, np.where(hl < INF, hl + oo + ee, INF))
            fext = (fu < INF) & (fu + ee <= hu + oo + ee)
            fv = np.where(fext, fu + ee, np.where(hu < INF, hu + oo + ee, INF))
            inner = (i > 0) & (j > 0)
            same = inner & (q[np.maximum(i, 1) - 1] == tt[np.maximum(j, 1) - 1]) if n and m else inner
            h = np.where(hd < INF, hd + np.where(same, 0, xx), INF)
            src = np.zeros(len(d), np.int64)
            from_e = ev < h
            h = np.where(from_e, ev, h)
            src[from_e] = 1
            from_f = fv < h
            h = np.where(from_f, fv, h)
            src[from_f] = 2
            Hn[k], En[k], Fn[k] = h, ev, fv
            rows[A] = (dmin, src | (eext.astype(np.int64) << 2) | (fext.astype(np.int64) << 3))
            D = np.where(h < INF, a * A - h, NO_TOP)
            first = int(np.argmax(D))  # the smallest diagonal among the largest
            top = int(D[first])
            if top > best:  # a later anti-diagonal takes the end only when strictly better
                best, end = top, (A, int(d[first]))
        H2, H1, E1, F1 = H1, Hn, En, Fn
        if X >= 0 and max(top, top_before) < best - 2 * X:
            dropped = 1
            break
        top_before = top
    assert best % 2 == 0
    i, j = (end[0] - end[1]) >> 1, (end[0] + end[1]) >> 1
    result = dict(score=best // 2, query_end=i, target_end=j, dropped=dropped)
    matrix, out = 0, []
    while (i, j) != (0, 0) or matrix:
        first, row = rows[i + j]
        b = int(row[(j - i - first) >> 1])
        if matrix == 0:
            if b & 3:
                matrix = b & 3
            else:
                out.append(0 if tt[j - 1] == q[i - 1] else 1)
                i, j = i - 1, j - 1
        elif matrix == 1:
            out.append(2)
            j -= 1
            if not b & 4:
                matrix = 0
        else:
            out.append(3)
            i -= 1
            if not b & 8:
                matrix = 0
    result["states"] = out[::-1]
    return result


def plain_best(Q, T, a, x, o, e):
    """(the largest score of an alignment of a prefix of Q with a prefix of T, the set of (i, j) where it is reached):
    the score definition as three max-recurrences over the full matrix"""
    n, m = len(Q), len(T)
    low = float("-inf")
    S = [[low] * (m + 1) for _ in range(n + 1)]   # the best alignment of Q[:i], T[:j]
    GT = [[low] * (m + 1) for _ in range(n + 1)]  # ... that ends in a target-only column
    GQ = [[low] * (m + 1) for _ in range(n + 1)]  # ... that ends in a query-only column
    S[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            if j > 0:
                GT[i][j] = max(GT[i][j - 1] - e, S[i][j - 1] - o - e)
            if i > 0:
                GQ[i][j] = max(GQ[i - 1][j] - e, S[i - 1][j] - o - e)
            diagonal = S[i - 1][j - 1] + (a if matches(Q[i - 1], T[j - 1]) else -x) if i > 0 and j > 0 else low
            S[i][j] = max(diagonal, GT[i][j], GQ[i][j])
    best = max(max(row) for row in S)
    return best, {(i, j) for i in range(n + 1) for j in range(m + 1) if S[i][j] == best}


def score_of(states, a, x, o, e):
    """the score of a state string: +a per match, -x per mismatch, -(o + L e) per maximal run of one gap state"""
    score, before = 0, None
    for s in states:
        if s == 0:
            score += a
        elif s == 1:
            score -= x
        else:
            score -= e + (0 if s == before else o)
        before = s
    return score


def consumed(states):
    """(query bases, target bases) that a state string uses up"""
    return sum(s != 2 for s in states), sum(s != 3 for s in states)
