"""The rules of the affine-gap global aligner in Python, twice.

align() is the banded aligner itself: in-band cells only, one numpy step per anti-diagonal over the cells of the
last two anti-diagonals, the four choice bits per cell, and the traceback that follows the bits alone. It is what the
device must reproduce byte for byte: states, cost and flag.

gotoh_cost() is a second formulation that shares nothing with it: the plain three-matrix recurrence over the full
matrix, row by row, without a band and without bits; cost_of() re-prices a state string. replay() checks with
tests/cigar_replay.py that a state string walks exactly the two sequences."""
import numpy as np

import cigar_replay

INF = 1 << 29
MAX_DIAGONALS = 2048
_ACTG = np.frombuffer(b"ACTG", np.uint8)


def _bytes(s):
    return np.frombuffer(s.encode("latin-1") if isinstance(s, str) else bytes(s), np.uint8)


def matches(q, t):
    """the default aligner's predicate on two characters"""
    return q == "ACTG"[(ord(t) >> 1) & 3]


def band(n, m, B):
    """(lo, hi, W) of a pair"""
    lo, hi = min(0, m - n) - B, max(0, m - n) + B
    return lo, hi, hi - lo + 1


def bound(n, m, x, o, e, B):
    """the cheapest conceivable path that leaves the band"""
    return 2 * o + e * (abs(m - n) + 2 * B + 2)


def align(Q, T, x=4, o=6, e=2, B=128):
    """dict(states (forward order; None: no result), cost (-1: no result), optimal)"""
    q, t = _bytes(Q), _bytes(T)
    n, m = len(q), len(t)
    lo, hi, W = band(n, m, B)
    if W > MAX_DIAGONALS or n + m >= 1 << 21:
        return dict(states=None, cost=-1, optimal=False)
    tt = _ACTG[(t >> 1) & 3]
    # the values of anti-diagonals a - 1 and a - 2 by diagonal, index d - lo + 1, INF where there is no cell
    H1, E1, F1 = (np.full(W + 2, INF, np.int64) for _ in range(3))
    H2 = np.full(W + 2, INF, np.int64)
    H1[1 - lo] = 0  # (0, 0), as anti-diagonal 0
    rows = {}       # a -> (first diagonal, bits of its cells, every second diagonal)
    for a in range(1, n + m + 1):
        dmin, dmax = max(lo, a - 2 * n, -a), min(hi, a, 2 * m - a)
        dmin += (dmin - a) & 1
        dmax -= (dmax - a) & 1
        Hn, En, Fn = (np.full(W + 2, INF, np.int64) for _ in range(3))
        if dmin <= dmax:
            d = np.arange(dmin, dmax + 1, 2)
            k = d - lo + 1
            i, j = (a - d) >> 1, (a + d) >> 1
            hl, el, hu, fu, hd = H1[k - 1], E1[k - 1], H1[k + 1], F1[k + 1], H2[k]
            eext = (el < INF) & (el + e <= hl + o + e)
            ev = np.where(eext, el + e, np.where(hl < INF, hl + o + e, INF))
            fext = (fu < INF) & (fu + e <= hu + o + e)
            fv = np.where(fext, fu + e, np.where(hu < INF, hu + o + e, INF))
            inner = (i > 0) & (j > 0)
            same = inner & (q[np.maximum(i, 1) - 1] == tt[np.maximum(j, 1) - 1]) if n and m else inner
            h = np.where(hd < INF, hd + np.where(same, 0, x), INF)
            src = np.zeros(len(d), np.int64)
            from_e = ev < h
            h = np.where(from_e, ev, h)
            src[from_e] = 1
            from_f = fv < h
            h = np.where(from_f, fv, h)
            src[from_f] = 2
            Hn[k], En[k], Fn[k] = h, ev, fv
            rows[a] = (dmin, src | (eext.astype(np.int64) << 2) | (fext.astype(np.int64) << 3))
        H2, H1, E1, F1 = H1, Hn, En, Fn
    cost = int(H1[m - n - lo + 1])
    # the traceback: the bits only
    i, j, matrix, out = n, m, 0, []
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
    return dict(states=out[::-1], cost=cost, optimal=cost <= bound(n, m, x, o, e, B))


def gotoh_cost(Q, T, x, o, e):
    """the optimal cost over the full matrix: three rows of the textbook recurrence, no band, no bits"""
    n, m = len(Q), len(T)
    big = float("inf")
    h = [0] + [o + e * j for j in range(1, m + 1)]
    f = [big] * (m + 1)  # ends in a query-only column
    for i in range(1, n + 1):
        up_h, up_f = h, f
        h, f = [big] * (m + 1), [big] * (m + 1)
        f[0] = min(up_f[0] + e, up_h[0] + o + e)
        h[0] = f[0]
        row_e = big  # ends in a target-only column
        for j in range(1, m + 1):
            row_e = min(row_e + e, h[j - 1] + o + e)
            f[j] = min(up_f[j] + e, up_h[j] + o + e)
            h[j] = min(up_h[j - 1] + (0 if matches(Q[i - 1], T[j - 1]) else x), row_e, f[j])
    return h[m]


def cost_of(states, x, o, e):
    """the price of a state string: x per mismatch, o + L e per maximal run of one gap state"""
    cost, before = 0, None
    for s in states:
        if s == 1:
            cost += x
        elif s in (2, 3):
            cost += e + (0 if s == before else o)
        before = s
    return cost


def cigar(states, extended=False):
    """Alignment::convert_to_cigar of a state string"""
    sym = "=XID" if extended else "MMID"
    out, last, run = [], None, 0
    for s in states:
        c = sym[s]
        if c == last:
            run += 1
        else:
            if last is not None:
                out.append("%d%s" % (run, last))
            last, run = c, 1
    if last is not None:
        out.append("%d%s" % (run, last))
    return "".join(out)


def replay(states, Q, T):
    """cigar_replay's walk of the states over Q and T (sequences of A, C, G, T): raises cigar_replay.ReplayError unless
    they use up both exactly and every 0 / 1 names an equal / an unequal pair; two empty sequences replay to nothing"""
    if not states and not Q and not T:
        return None
    record = ["q", str(len(Q)), "0", str(len(Q)), "+", "t", str(len(T)), "0", str(len(T)), "0", "0", "255",
              "cg:Z:" + cigar(states, True)]
    return cigar_replay.replay_paf(record, {"q": Q}, {"t": T})
