"""CPU oracle of cudamapper's on-device overlap alignment: slices and strand as the gather kernel takes them, the
aligner's own complement table, and the project's pinned Hirschberg + Myers restatement (tests/oracle_aligner.py) with
max_query_length = the longest query slice of one call. TEST INFRASTRUCTURE ONLY."""
import oracle_aligner as A

# genomeutils::reverse_complement: "TGAC"[(c >> 1) & 3] for every byte, N and lower case included
COMPLEMENT = bytes(b"TGAC"[(c >> 1) & 3] for c in range(256))


def _bytes(r):
    return r.encode() if isinstance(r, str) else bytes(r)


def slices(o, queries, targets, first_query_read_id=0, first_target_read_id=0):
    """(query slice, target slice as the aligner sees it) of one overlap record"""
    q = _bytes(queries[int(o["query_read_id"]) - first_query_read_id])
    t = _bytes(targets[int(o["target_read_id"]) - first_target_read_id])
    qs = q[int(o["query_start_position_in_read"]):int(o["query_end_position_in_read"])]
    ts = t[int(o["target_start_position_in_read"]):int(o["target_end_position_in_read"])]
    return qs, (ts.translate(COMPLEMENT)[::-1] if int(o["relative_strand"]) == ord("-") else ts)


def alignments(overlaps, queries, targets=None, groups=None, first_query_read_id=0, first_target_read_id=0):
    """oracle_aligner.hirschberg() of every overlap. One call aligns with M = its longest query slice: all overlaps
    are one call, or, with groups = (query descriptors, target descriptors) of group_reads_into_indices, the overlaps
    of one index pair are, the way the batched driver calls the aligner."""
    targets = queries if targets is None else targets
    pairs = [slices(o, queries, targets, first_query_read_id, first_target_read_id) for o in overlaps]

    def group_of(read, descriptors):
        return next(i for i, (first, n) in enumerate(descriptors) if first <= read < first + n)
    calls = [0 if groups is None else (group_of(int(o["query_read_id"]), groups[0]),
                                       group_of(int(o["target_read_id"]), groups[1])) for o in overlaps]
    capacity = {}
    for call, (q, _) in zip(calls, pairs):
        capacity[call] = max(capacity.get(call, 0), len(q))
    return [A.hirschberg(q, t, capacity[call]) for call, (q, t) in zip(calls, pairs)]


def cigars(overlaps, queries, targets=None, groups=None, first_query_read_id=0, first_target_read_id=0):
    return [a["cigar"] for a in alignments(overlaps, queries, targets, groups, first_query_read_id,
                                           first_target_read_id)]
