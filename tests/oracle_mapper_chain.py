"""CPU oracle of cudamapper's chaining overlapper -- TEST INFRASTRUCTURE ONLY. Plain Python over numpy ANCHOR arrays
(tests/oracle_mapper.py), rules C1-C8 of include/gwhip_mapper.h taken literally, one anchor at a time:

  C1  a group is a maximal run of anchors of one (query read, target read); all against all a group of a read with
      itself yields nothing; a group of 2^24 anchors or more is an error;
  C2  every group is chained for '+' and for '-' on its own; dq = q_i - q_j, dt = t_i - t_j ('+') or t_j - t_i ('-'),
      exact (positions are uint32, the differences are taken in unbounded integers);
  C3  j may precede i iff i - 64 <= j < i, 0 < dq <= G, 0 < dt <= G and |dq - dt| <= B;
  C4  gain = min(dq, dt, k) - cost(|dq - dt|), cost(0) = 0, cost(d) = d k / 100 + (floor(log2 d) >> 1);
  C5  f(i) = max_j f(j) + gain if that exceeds k, with the largest such j as p(i); k and no predecessor otherwise;
  C6  up to M rounds per group and orientation: the unused anchor of largest f (smallest index on ties), stop below S;
      walk the predecessors until there is none or it is used; score f(e) - f(u) when cut in front of a used u;
      a round whose chain scores below S still uses its anchors;
  C7  one OVERLAP record per candidate, through the filter of the triggered overlapper (float32 fractions);
  C8  groups in anchor order, '+' rounds then '-' rounds.
`lookback=None` lifts the limit of 64 (tests only)."""
import numpy as np

from oracle_mapper import ANCHOR, OVERLAP

LOOKBACK = 64
DEFAULTS = dict(max_gap=5000, bandwidth=500, min_chain_score=40, max_chains=4)
FILTER_DEFAULTS = dict(min_residues=3, min_overlap_len=250, min_bases_per_residue=1000, min_overlap_fraction=0.8)


def cost(d, k):
    return 0 if d == 0 else (d * k) // 100 + ((d.bit_length() - 1) >> 1)


def gain(dq, dt, k):
    return min(dq, dt, k) - cost(abs(dq - dt), k)


def may_precede(dq, dt, max_gap, bandwidth):
    return 0 < dq <= max_gap and 0 < dt <= max_gap and abs(dq - dt) <= bandwidth


def check_parameters(kmer_size, max_gap, bandwidth, min_chain_score, max_chains, min_residues=0, min_overlap_len=0,
                     min_bases_per_residue=0):
    if not 1 <= kmer_size <= 32 or max_gap < 1 or bandwidth < 0 or min_chain_score < 0 or not 1 <= max_chains <= 64:
        raise ValueError("chaining parameter out of range")
    if min_residues < 0 or min_overlap_len < 0 or min_bases_per_residue < 0:
        raise ValueError("negative filter value")


def scores(q, t, sign, kmer_size, max_gap, bandwidth, lookback=LOOKBACK):
    """(f, p) of one group and one orientation (sign +1 / -1); p is -1 where an anchor has no predecessor"""
    m = len(q)
    f, p = [kmer_size] * m, [-1] * m
    for i in range(m):
        best, at = None, -1
        for j in range(0 if lookback is None else max(0, i - lookback), i):
            dq, dt = q[i] - q[j], sign * (t[i] - t[j])
            if may_precede(dq, dt, max_gap, bandwidth):
                v = f[j] + gain(dq, dt, kmer_size)
                if best is None or v >= best:  # the largest j among equals
                    best, at = v, j
        if best is not None and best > kmer_size:
            f[i], p[i] = best, at
    return f, p


def extract(f, p, min_chain_score, max_chains):
    """C6: [(anchor indices first to last, score, is candidate)] of the rounds that ran"""
    m, used, rounds = len(f), [False] * len(f), []
    for _ in range(max_chains):
        e = -1
        for i in range(m):
            if not used[i] and (e < 0 or f[i] > f[e]):
                e = i
        if e < 0 or f[e] < min_chain_score:
            break
        chain, cur, cut = [], e, -1
        while True:
            chain.append(cur)
            used[cur] = True
            if p[cur] < 0:
                break
            if used[p[cur]]:
                cut = p[cur]
                break
            cur = p[cur]
        score = f[e] - (f[cut] if cut >= 0 else 0)
        rounds.append((chain[::-1], score, score >= min_chain_score))
    return rounds


def passes_filter(o, all_to_all, min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction):
    """the predicate of the triggered overlapper's filter: unsigned lengths, integer bases per residue, strict > on the
    float32 fractions"""
    u32 = 0xFFFFFFFF
    tl = (int(o["target_end_position_in_read"]) - int(o["target_start_position_in_read"])) & u32
    ql = (int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"])) & u32
    length, residues = max(tl, ql), int(o["num_residues"])
    if residues < min_residues or residues == 0:
        return False
    if not length // residues < min_bases_per_residue or ql < min_overlap_len or tl < min_overlap_len:
        return False
    if all_to_all and o["query_read_id"] == o["target_read_id"]:
        return False
    fraction = np.float32(min_overlap_fraction)
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.float32(tl) / np.float32(length) > fraction and np.float32(ql) / np.float32(length) > fraction)


def groups_of(anchors):
    """[(first, one past last)] of the groups of C1"""
    a = np.ascontiguousarray(anchors, ANCHOR)
    if len(a) == 0:
        return []
    new = np.flatnonzero((a["query_read_id"][1:] != a["query_read_id"][:-1]) |
                         (a["target_read_id"][1:] != a["target_read_id"][:-1])) + 1
    edges = [0] + new.tolist() + [len(a)]
    return list(zip(edges[:-1], edges[1:]))


def chain_overlaps(anchors, kmer_size=15, max_gap=5000, bandwidth=500, min_chain_score=40, max_chains=4,
                   all_to_all=True, min_residues=3, min_overlap_len=250, min_bases_per_residue=1000,
                   min_overlap_fraction=0.8, lookback=LOOKBACK, with_chains=False):
    """(OVERLAP array, int32 scores) of rules C1-C8; with_chains adds the anchor indices of every kept record"""
    check_parameters(kmer_size, max_gap, bandwidth, min_chain_score, max_chains, min_residues, min_overlap_len,
                     min_bases_per_residue)
    a = np.ascontiguousarray(anchors, ANCHOR)
    if len(a) >= 1 << 32:
        raise ValueError("2^32 anchors or more")
    records, kept_scores, kept_chains = [], [], []
    for lo, hi in groups_of(a):
        if hi - lo >= 1 << 24:
            raise ValueError("a group of 2^24 anchors or more")
        qid, tid = int(a["query_read_id"][lo]), int(a["target_read_id"][lo])
        if all_to_all and qid == tid:
            continue
        q = [int(x) for x in a["query_position_in_read"][lo:hi]]
        t = [int(x) for x in a["target_position_in_read"][lo:hi]]
        for sign, strand in ((1, "+"), (-1, "-")):
            f, p = scores(q, t, sign, kmer_size, max_gap, bandwidth, lookback)
            for chain, score, candidate in extract(f, p, min_chain_score, max_chains):
                if not candidate:
                    continue
                first, last = chain[0], chain[-1]
                o = np.zeros((), OVERLAP)
                o["query_read_id"], o["target_read_id"] = qid, tid
                o["query_start_position_in_read"], o["query_end_position_in_read"] = q[first], q[last]
                ts, te = (t[first], t[last]) if sign > 0 else (t[last], t[first])
                o["target_start_position_in_read"], o["target_end_position_in_read"] = ts, te
                o["relative_strand"], o["num_residues"], o["overlap_complete"] = ord(strand), len(chain), 1
                if passes_filter(o, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                                 min_overlap_fraction):
                    records.append(o)
                    kept_scores.append(score)
                    kept_chains.append([lo + i for i in chain])
    out = np.array(records, OVERLAP) if records else np.zeros(0, OVERLAP)
    result = (out, np.array(kept_scores, np.int32))
    return result + (kept_chains,) if with_chains else result
