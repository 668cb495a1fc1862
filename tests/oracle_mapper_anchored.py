"""CPU oracle of anchored overlap alignment (rules G1-G6 next to gwm_align_overlaps_anchored
in include/gwhip_mapper.h): every overlap cut at anchors of its chain, the pieces aligned one by one by the oracle of
the call's aligner -- oracle_mapper_align's Hirschberg + Myers restatement, oracle_affine or oracle_affine2 -- and their
states concatenated. Plain Python, one anchor at a time. TEST INFRASTRUCTURE ONLY."""
import oracle_affine as OA
import oracle_affine2 as OA2
import oracle_aligner as A
import oracle_mapper_align as OM

DEFAULT_SPACING = 256


class NotMonotone(ValueError):
    """the valid anchors of a record are not strictly increasing (G3); .record names it"""

    def __init__(self, record):
        ValueError.__init__(self, "the anchors of overlap %d are not strictly increasing in query and target" % record)
        self.record = record


def check_parameters(k, S):
    if not (1 <= k <= 32 and S >= 1):
        raise ValueError("anchor_kmer_size %d, anchor_spacing %d outside 1..32, >= 1" % (k, S))


def check_offsets(offsets, n, n_anchors):
    offsets = [int(x) for x in offsets]
    if len(offsets) != n + 1 or offsets[0] != 0 or any(b < a for a, b in zip(offsets, offsets[1:])) or offsets[-1] != n_anchors:
        raise ValueError("anchor offsets must start at 0, never decrease and end at the number of anchors")


def lengths(o):
    return (int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"]),
            int(o["target_end_position_in_read"]) - int(o["target_start_position_in_read"]))


def coordinates(o, q, t, k):
    """G1: (u, v) of anchor (q, t) in the slices of record o"""
    u = int(q) - int(o["query_start_position_in_read"])
    if int(o["relative_strand"]) == ord("-"):
        return u, int(o["target_end_position_in_read"]) - int(t) - k
    return u, int(t) - int(o["target_start_position_in_read"])


def cuts(o, anchors, k, S):
    """G2-G4: the cuts [(u, v)] of one record from its anchors [(q, t)]; None when G3 fails"""
    n, m = lengths(o)
    out, before = [], None
    for q, t in anchors:
        u, v = coordinates(o, q, t, k)
        if not (0 < u < n and 0 < v < m):
            continue
        if before is not None and not (u > before[0] and v > before[1]):
            return None
        if before is None or u // S != before[0] // S:
            out.append((u, v))
        before = (u, v)
    return out


def pieces(o, anchors, k=15, S=DEFAULT_SPACING):
    """G5: [(u, v, query length, target length)] of one record, or None when G3 fails"""
    c = cuts(o, anchors, k, S)
    if c is None:
        return None
    n, m = lengths(o)
    edges = [(0, 0)] + c + [(n, m)]
    return [(u, v, u2 - u, v2 - v) for (u, v), (u2, v2) in zip(edges[:-1], edges[1:])]


def plan(overlaps, anchor_offsets, anchor_positions, k=15, S=DEFAULT_SPACING):
    """the pieces of every record of a call; raises ValueError, and NotMonotone for the first record that fails G3"""
    check_parameters(k, S)
    check_offsets(anchor_offsets, len(overlaps), len(anchor_positions))
    out = []
    for i, o in enumerate(overlaps):
        own = [(int(q), int(t)) for q, t in anchor_positions[int(anchor_offsets[i]):int(anchor_offsets[i + 1])]]
        p = pieces(o, own, k, S)
        if p is None:
            raise NotMonotone(i)
        out.append(p)
    return out


def _aligner(scoring, capacity):
    """(query, target) -> forward states or None, for scoring None, (x, o, e, B) or (x, o1, e1, o2, e2, B)"""
    if scoring is None:
        def default(q, t):
            r = A.hirschberg(q, t, capacity)
            return list(r["states"]) if (r["states"] or not (q or t)) else None
        return default
    scoring = tuple(int(v) for v in scoring)
    one = OA.align if len(scoring) == 4 else OA2.align

    def affine(q, t):
        return one(q, t, *scoring)["states"]
    return affine


def alignments(overlaps, queries, targets, anchor_offsets, anchor_positions, k=15, S=DEFAULT_SPACING, scoring=None,
               first_query_read_id=0, first_target_read_id=0):
    """G6 for every record: dict(states (forward order; None: a piece had no result), pieces, piece_states)"""
    targets = queries if targets is None else targets
    plans = plan(overlaps, anchor_offsets, anchor_positions, k, S)
    capacity = max([p[2] for record in plans for p in record] + [0])
    align = _aligner(scoring, capacity)
    out = []
    for o, record in zip(overlaps, plans):
        q, t = OM.slices(o, queries, targets, first_query_read_id, first_target_read_id)
        q, t = q.decode(), t.decode()
        parts = [align(q[u:u + dn], t[v:v + dm]) for u, v, dn, dm in record]
        whole = None if any(p is None for p in parts) else [s for p in parts for s in p]
        out.append(dict(states=whole, pieces=record, piece_states=parts))
    return out


def cigars(results):
    """(CIGARs, edit distances) of alignments() as align_overlaps returns them"""
    texts = [OA.cigar(r["states"]) if r["states"] is not None else "" for r in results]
    edits = [sum(1 for s in r["states"] if s != 0) if r["states"] is not None else -1 for r in results]
    return texts, edits


def lists_of(chains, anchors):
    """(anchor_offsets, anchor_positions) from the chains of oracle_mapper_chain.chain_overlaps(with_chains=True)"""
    import numpy as np
    offsets, rows = [0], []
    for chain in chains:
        rows += [(int(anchors["query_position_in_read"][i]), int(anchors["target_position_in_read"][i])) for i in chain]
        offsets.append(len(rows))
    return np.array(offsets, np.int64), np.array(rows, np.uint32).reshape(-1, 2)
