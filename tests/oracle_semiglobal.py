"""CPU oracle of cudaaligner's infix / prefix alignment types: a plain numpy dynamic program. TEST INFRASTRUCTURE ONLY.

Query Q (n bases), target T (m bases), unit costs, D[i][0] = i, D[0][j] = j (prefix) or 0 (infix), otherwise
D[i][j] = min(D[i-1][j-1] + (Q[i-1] does not match T[j-1]), D[i-1][j] + 1, D[i][j-1] + 1). A query base q matches a
target base t when q == "ACTG"[(t >> 1) & 3], the predicate of the default global aligner (equality on A, C, G, T).

    d  = min_j D[n][j]
    te = the smallest j with D[n][j] == d (column 0 counts)
    tb = 0 for prefix; for infix the largest b <= te with global_distance(Q, T[b:te]) == d

One row at a time, vectorised over the columns: the diagonal and vertical moves need the previous row only, and the
horizontal move, D[i][j] = min_k<=j (c[k] + j - k), is a running minimum of c[k] - k."""
import numpy as np

_ACTG = np.frombuffer(b"ACTG", np.uint8)


def _bytes(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)


def last_row(query, target, free_top_row):
    """D[n][0 .. m] as an int64 array."""
    q, t = _bytes(query), _bytes(target)
    m = len(t)
    wanted = _ACTG[(t >> 1) & 3] if m else t      # the query base that matches each target base
    columns = np.arange(m + 1, dtype=np.int64)
    row = np.zeros(m + 1, np.int64) if free_top_row else columns.copy()
    for i in range(1, len(q) + 1):
        cur = np.empty(m + 1, np.int64)
        cur[0] = i
        np.minimum(row[:-1] + (wanted != q[i - 1]), row[1:] + 1, out=cur[1:])
        row = np.minimum.accumulate(cur - columns) + columns
    return row


def semiglobal(query, target, mode):
    """(d, te, tb) of `mode` "infix" or "prefix"."""
    if mode not in ("infix", "prefix"):
        raise ValueError(mode)
    row = last_row(query, target, mode == "infix")
    d = int(row.min())
    te = int(np.argmax(row == d))                  # the first column at the minimum
    if mode == "prefix":
        return d, te, 0
    # the shortest suffix of T[0:te] at global distance d from Q: a prefix scan of both reversed, column 0 included
    back = last_row(query[::-1], target[:te][::-1], False)
    return d, te, te - int(np.argmax(back == d))


def global_distance(query, target):
    return int(last_row(query, target, False)[-1])
