"""CPU oracle of pileups, on top of the pinned aligner oracle (tests/oracle_mapper_align.py):
the per-base counts of both roles from the per-column alignment states, column by column with the counts a(j) and b(j),
and, as a second, independent formulation, from the CIGAR string, run by run with positions from run lengths and whole
runs added at once. The CIGAR formulation takes any CIGAR, so the GPU tests apply it to what align_overlaps() returns.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import cigar_replay as CR
import oracle_correct as OC
import oracle_mapper_align as OA
import oracle_polish as OPo

CHANNELS = ("A", "C", "G", "T", "deletion", "insertion")
DELETION, INSERTION = 4, 5
# byte -> channel: the aligner's folding (c >> 1) & 3 gives A, C, T, G = 0, 1, 2, 3
CHANNEL_OF = np.array([(0, 1, 3, 2)[(c >> 1) & 3] for c in range(256)], np.int64)


def _data(r):
    return np.frombuffer(OPo._bytes(r), np.uint8)


def empty(reads):
    return [np.zeros((6, len(r)), np.uint32) for r in reads]


def add_from_states(pile, o, states, supplier, query_role):
    """Adds overlap o with per-column `states` (forward column order) to `pile`, the (6, length) array of the read that
    owns the positions: the target read, or in the query role the query read. `supplier` is the other read."""
    qs, qe, ts, te, reverse = OPo._fields(o)
    supplier = _data(supplier)
    A, B = sum(s != 2 for s in states), sum(s != 3 for s in states)
    a = b = 0
    before = None
    for s in states:
        q = qs + a
        t = te - 1 - b if reverse else ts + b
        own, other = (q, t) if query_role else (t, q)
        skips = 2 if query_role else 3  # the state that consumes no base of the owner
        if s < 2:
            c = int(CHANNEL_OF[supplier[other]])
            pile[3 - c if reverse else c, own] += 1
        elif s != skips:
            pile[DELETION, own] += 1
        elif before != skips:  # the head of a maximal run
            if query_role and 1 <= a <= A - 1:
                pile[INSERTION, qs + a - 1] += 1
            if not query_role and 1 <= b <= B - 1:
                pile[INSERTION, te - 1 - b if reverse else ts + b - 1] += 1
        before = s
        a += s != 2
        b += s != 3


def add_from_cigar(pile, o, cigar, supplier, query_role):
    """The same from the CIGAR text (M: match and mismatch, I: target only, D: query only), whole runs at a time."""
    qs, qe, ts, te, reverse = OPo._fields(o)
    supplier = _data(supplier)
    runs = CR.parse_cigar(cigar, "MID") if cigar else []
    in_query = sum(n for n, op in runs if op != "I")   # A
    in_target = sum(n for n, op in runs if op != "D")  # B
    q_used = t_used = 0
    for n, op in runs:
        # the run's positions in column order
        q_at = np.arange(qs + q_used, qs + q_used + n)
        t_at = np.arange(te - 1 - t_used, te - 1 - t_used - n, -1) if reverse else np.arange(ts + t_used, ts + t_used + n)
        own, other = (q_at, t_at) if query_role else (t_at, q_at)
        if op == "M":
            c = CHANNEL_OF[supplier[other]]
            np.add.at(pile, (3 - c if reverse else c, own), 1)
            q_used += n
            t_used += n
        elif (op == "D") == query_role:  # the owner's base alone
            pile[DELETION, own] += 1     # positions of one run are distinct
            if query_role:
                q_used += n
            else:
                t_used += n
        elif query_role:  # I: target bases between two query bases
            if 1 <= q_used <= in_query - 1:
                pile[INSERTION, qs + q_used - 1] += 1
            t_used += n
        else:             # D: query bases between two target bases
            if 1 <= t_used <= in_target - 1:
                pile[INSERTION, te - 1 - t_used if reverse else ts + t_used - 1] += 1
            q_used += n


def _add(pile, o, alignment, supplier, query_role, formulation):
    if formulation == "states":
        add_from_states(pile, o, alignment["states"], supplier, query_role)
    else:
        add_from_cigar(pile, o, alignment["cigar"], supplier, query_role)


def of_cigars(cigars):
    """alignments that hold nothing but their CIGAR strings, for the "cigar" formulation"""
    return [dict(cigar=c) for c in cigars]


def overlap_pileup(overlaps, queries, targets=None, alignments=None, formulation="states", first_query_read_id=0,
                   first_target_read_id=0):
    """[(6, len(target)) uint32 per target] as cudamapper.overlap_pileup; `alignments` = OA.alignments(...) or
    of_cigars(...) if the caller has them already"""
    targets = queries if targets is None else targets
    if alignments is None:
        alignments = OA.alignments(overlaps, queries, targets, None, first_query_read_id, first_target_read_id)
    piles = empty(targets)
    for o, a in zip(overlaps, alignments):
        qi, ti = int(o["query_read_id"]) - first_query_read_id, int(o["target_read_id"]) - first_target_read_id
        _add(piles[ti], o, a, queries[qi], False, formulation)
    return piles


def pair_pileup(pairs, reads, alignments=None, formulation="states", first_read_id=0, roles=(False, True)):
    """[(6, len(read)) uint32 per read] as cudamapper.pair_pileup: both roles of every pair into one array; `roles`
    picks one of them: (False,) the target role alone, (True,) the query role alone"""
    if alignments is None:
        alignments = OA.alignments(pairs, reads, None, None, first_read_id, first_read_id)
    piles = empty(reads)
    for o, a in zip(pairs, alignments):
        qi, ti = int(o["query_read_id"]) - first_read_id, int(o["target_read_id"]) - first_read_id
        for query_role in roles:
            owner, other = (qi, ti) if query_role else (ti, qi)
            _add(piles[owner], o, a, reads[other], query_role, formulation)
    return piles


def one_overlap_per_read(overlaps):
    """rule 1 of section 3j: the positions of the overlaps polish() aligns, ascending"""
    kept = {}
    for i, o in enumerate(overlaps):
        q = int(o["query_read_id"])
        span = int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"])
        if q not in kept or span > kept[q][0]:
            kept[q] = (span, i)
    return sorted(i for _, i in kept.values())


def pileup(reads, targets, overlaps, formulation="states"):
    """polisher.pileup with overlaps given"""
    return overlap_pileup(overlaps[one_overlap_per_read(overlaps)], reads, targets, None, formulation)


def read_pileup(reads, overlaps, formulation="states"):
    """polisher.read_pileup with overlaps given"""
    return pair_pileup(overlaps[OC.select_pairs(overlaps)], reads, None, formulation)


def covering(overlaps, reads, query_role, alignments, first_read_id=0):
    """per read of `reads`, the number of records with an alignment whose slice of it covers each position: the slice
    of the target read, or in the query role that of the query read"""
    out = [np.zeros(len(r), np.int64) for r in reads]
    for o, a in zip(overlaps, alignments):
        if not (a.get("states") or a.get("cigar")):
            continue
        qs, qe, ts, te, _ = OPo._fields(o)
        if query_role:
            out[int(o["query_read_id"]) - first_read_id][qs:qe] += 1
        else:
            out[int(o["target_read_id"]) - first_read_id][ts:te] += 1
    return out


def depth(pile):
    return pile[:5].sum(0)
