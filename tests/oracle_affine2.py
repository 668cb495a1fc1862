"""The rules of the two-piece affine-gap global aligner in Python, three times.

align() is the banded aligner itself: in-band cells only, one numpy step per anti-diagonal over the cells of the last
two anti-diagonals, one byte of choices per cell (src, the four ext bits, the mismatch bit) and the traceback that
follows the bytes alone through five matrices. It is what the device must reproduce byte for byte: states, cost, flag.

five_matrix_cost() is the plain recurrence over the full matrix, row by row, without a band and without bits.

general_gap_cost() knows nothing of E and F: H[i][j] = min(diagonal, min_L H[i][j-L] + g(L), min_L H[i-L][j] + g(L)),
written from the definition of g alone, so that the recurrences are checked against what they claim to compute.

cost_of() re-prices every maximal gap run of a state string with g; replay() is oracle_affine's."""
import numpy as np

from oracle_affine import INF, _ACTG, _bytes, band, cigar, matches, replay  # noqa: F401 (re-exported)

MAX_DIAGONALS = 1024
DEFAULT = (6, 4, 3, 24, 2)


def g(L, o1, e1, o2, e2):
    """the cost of a gap run of L >= 1 columns"""
    return min(o1 + L * e1, o2 + L * e2)


def bound(n, m, o1, e1, o2, e2, B):
    """the cheapest conceivable path that leaves the band: B + 1 gap columns of one kind, B + 1 + |m - n| of the other"""
    return g(B + 1, o1, e1, o2, e2) + g(B + 1 + abs(m - n), o1, e1, o2, e2)


def _gap(prev, h, o, e):
    """(value, ext bit) of one gap matrix from its own value and H at the cell the gap comes from"""
    ext = (prev < INF) & (prev + e <= h + o + e)
    return np.where(ext, prev + e, np.where(h < INF, h + o + e, INF)), ext.astype(np.int64)


def align(Q, T, x=6, o1=4, e1=3, o2=24, e2=2, B=128):
    """dict(states (forward order; None: no result), cost (-1: no result), optimal)"""
    q, t = _bytes(Q), _bytes(T)
    n, m = len(q), len(t)
    lo, hi, W = band(n, m, B)
    if W > MAX_DIAGONALS or n + m >= 1 << 21:
        return dict(states=None, cost=-1, optimal=False)
    tt = _ACTG[(t >> 1) & 3]
    # the values of anti-diagonals a - 1 and a - 2 by diagonal, index d - lo + 1, INF where there is no cell
    H1, E1, F1, E2, F2 = (np.full(W + 2, INF, np.int64) for _ in range(5))
    H2 = np.full(W + 2, INF, np.int64)
    H1[1 - lo] = 0  # (0, 0), as anti-diagonal 0
    rows = {}       # a -> (first diagonal, bytes of its cells, every second diagonal)
    for a in range(1, n + m + 1):
        dmin, dmax = max(lo, a - 2 * n, -a), min(hi, a, 2 * m - a)
        dmin += (dmin - a) & 1
        dmax -= (dmax - a) & 1
        Hn, E1n, F1n, E2n, F2n = (np.full(W + 2, INF, np.int64) for _ in range(5))
        if dmin <= dmax:
            d = np.arange(dmin, dmax + 1, 2)
            k = d - lo + 1
            i, j = (a - d) >> 1, (a + d) >> 1
            hl, hu, hd = H1[k - 1], H1[k + 1], H2[k]
            e1v, e1x = _gap(E1[k - 1], hl, o1, e1)
            f1v, f1x = _gap(F1[k + 1], hu, o1, e1)
            e2v, e2x = _gap(E2[k - 1], hl, o2, e2)
            f2v, f2x = _gap(F2[k + 1], hu, o2, e2)
            inner = (i > 0) & (j > 0)
            same = inner & (q[np.maximum(i, 1) - 1] == tt[np.maximum(j, 1) - 1]) if n and m else inner
            h = np.where(hd < INF, hd + np.where(same, 0, x), INF)
            src = np.zeros(len(d), np.int64)
            for code, v in ((1, e1v), (2, f1v), (3, e2v), (4, f2v)):
                better = v < h
                h = np.where(better, v, h)
                src[better] = code
            Hn[k], E1n[k], F1n[k], E2n[k], F2n[k] = h, e1v, f1v, e2v, f2v
            rows[a] = (dmin, src | (e1x << 3) | (f1x << 4) | (e2x << 5) | (f2x << 6) | ((~same).astype(np.int64) << 7))
        H2, H1, E1, F1, E2, F2 = H1, Hn, E1n, F1n, E2n, F2n
    cost = int(H1[m - n - lo + 1])
    # the traceback: the bytes only
    i, j, matrix, out = n, m, 0, []
    ext_bit = {1: 8, 2: 16, 3: 32, 4: 64}
    while (i, j) != (0, 0) or matrix:
        first, row = rows[i + j]
        b = int(row[(j - i - first) >> 1])
        if matrix == 0:
            if b & 7:
                matrix = b & 7
            else:
                out.append(1 if b & 128 else 0)
                i, j = i - 1, j - 1
            continue
        if matrix in (1, 3):
            out.append(2)
            j -= 1
        else:
            out.append(3)
            i -= 1
        if not b & ext_bit[matrix]:
            matrix = 0
    return dict(states=out[::-1], cost=cost, optimal=cost <= bound(n, m, o1, e1, o2, e2, B))


def five_matrix_cost(Q, T, x, o1, e1, o2, e2):
    """the optimal cost over the full matrix: rows of the five-matrix recurrence, no band, no bits"""
    n, m = len(Q), len(T)
    big = float("inf")
    h = [0] + [g(j, o1, e1, o2, e2) for j in range(1, m + 1)]
    f1, f2 = [big] * (m + 1), [big] * (m + 1)  # end in a query-only column, by piece
    for i in range(1, n + 1):
        up_h, up_f1, up_f2 = h, f1, f2
        h, f1, f2 = [big] * (m + 1), [big] * (m + 1), [big] * (m + 1)
        f1[0] = min(up_f1[0] + e1, up_h[0] + o1 + e1)
        f2[0] = min(up_f2[0] + e2, up_h[0] + o2 + e2)
        h[0] = min(f1[0], f2[0])
        row_e1 = row_e2 = big  # end in a target-only column
        for j in range(1, m + 1):
            row_e1 = min(row_e1 + e1, h[j - 1] + o1 + e1)
            row_e2 = min(row_e2 + e2, h[j - 1] + o2 + e2)
            f1[j] = min(up_f1[j] + e1, up_h[j] + o1 + e1)
            f2[j] = min(up_f2[j] + e2, up_h[j] + o2 + e2)
            h[j] = min(up_h[j - 1] + (0 if matches(Q[i - 1], T[j - 1]) else x), row_e1, f1[j], row_e2, f2[j])
    return h[m]


def general_gap_cost(Q, T, x, o1, e1, o2, e2):
    """the optimal cost when a gap run of L columns costs g(L), whatever g is: cubic, from the definition alone"""
    n, m = len(Q), len(T)
    H = [[None] * (m + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            best = []
            if i and j:
                best.append(H[i - 1][j - 1] + (0 if matches(Q[i - 1], T[j - 1]) else x))
            best += [H[i][j - L] + g(L, o1, e1, o2, e2) for L in range(1, j + 1)]
            best += [H[i - L][j] + g(L, o1, e1, o2, e2) for L in range(1, i + 1)]
            H[i][j] = min(best)
    return H[n][m]


def runs(states):
    """the maximal gap runs of a state string: (state, length)"""
    out = []
    for s in states:
        if s in (2, 3):
            if out and out[-1][0] == s and out[-1][2]:
                out[-1][1] += 1
            else:
                out.append([s, 1, True])
        elif out:
            out[-1][2] = False
    return [(s, L) for s, L, _ in out]


def cost_of(states, x, o1, e1, o2, e2):
    """the price of a state string: x per mismatch, g(L) per maximal run of one gap state"""
    return x * sum(1 for s in states if s == 1) + sum(g(L, o1, e1, o2, e2) for _, L in runs(states))
