"""CPU oracle of cudamapper's overlap post-processing -- TEST INFRASTRUCTURE ONLY. Plain Python, one overlap at a time,
restated from the behaviour of GenomeWorks' cudamapper (overlapper.cpp, cudamapper_utils.cpp, utils.cpp), not from its
text. Overlaps are numpy OVERLAP arrays (tests/oracle_mapper.py), reads are bytes / str.

The rules a quick reading misses are kept literally:
  * gaps are abs() of a uint32 difference reinterpreted as int32 (abs of -2^31 stays -2^31, as two's complement gives);
  * float32 ratios are compared with the doubles 0.8 and 0.2;
  * a fused record takes its other fields from the run's last member, or from the second to last when the run reaches
    the end of the array;
  * a window shorter than 15 bases is one k-mer (the empty window too); k-mers form multisets;
  * the three rescue rounds and their early exit (which compares query_end with the previous query *start*);
  * reverse complement: A<->T, C<->G in upper case, every other byte stays as it is (the reference indexes a 26-entry
    table with c - 'A', which leaves the other upper-case letters alone and is undefined for anything else); the middle
    base of an odd-length target is not complemented (the reference swaps len / 2 pairs in place and skips it).
Where the reference is undefined or throws -- an overlap position beyond its read, a read id outside the read set --
rescue_overlap_ends raises ValueError."""
from collections import Counter

import numpy as np

from oracle_mapper import OVERLAP

U32 = 0xFFFFFFFF
KMER = 15
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _abs_i32(x):
    """abs(int(uint32 difference))"""
    x &= U32
    if x >= 1 << 31:
        x -= 1 << 32
    return x if x == -(1 << 31) else abs(x)


def _f32_div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float32(a) / np.float32(b))


def merge_conditions(o1, o2):
    """None when strand or read pair differ, else which of (short_gap, gap_ratio_ok, short_gap_relative_to_length)
    hold, each evaluated on its own (the reference stops at the first that holds, so it never forms 0 / 0)."""
    if o1["relative_strand"] != o2["relative_strand"] or int(o1["relative_strand"]) not in (ord("+"), ord("-")):
        return None
    if o1["query_read_id"] != o2["query_read_id"] or o1["target_read_id"] != o2["target_read_id"]:
        return None
    g = lambda r, f: int(r[f + "_position_in_read"])
    query_gap = _abs_i32(g(o2, "query_start") - g(o1, "query_end"))
    if int(o1["relative_strand"]) == ord("-"):
        target_gap = _abs_i32(g(o1, "target_start") - g(o2, "target_end"))
    else:
        target_gap = _abs_i32(g(o2, "target_start") - g(o1, "target_end"))
    short = query_gap < 500 and target_gap < 500
    ratio = _f32_div(min(query_gap, target_gap), max(query_gap, target_gap)) > 0.8  # nan > 0.8 is False
    total_q = ((g(o1, "query_end") - g(o1, "query_start")) + (g(o2, "query_end") - g(o2, "query_start"))) & U32
    total_t = ((g(o1, "target_end") - g(o1, "target_start")) + (g(o2, "target_end") - g(o2, "target_start"))) & U32
    relative = _f32_div(query_gap, total_q) < 0.2 and _f32_div(target_gap, total_t) < 0.2
    return short, ratio, relative


def overlaps_mergable(o1, o2):
    c = merge_conditions(o1, o2)
    return c is not None and (c[0] or c[1] or c[2])


def mergable_flags(overlaps):
    """flags[i]: overlaps[i] and overlaps[i + 1] fuse"""
    return np.array([overlaps_mergable(overlaps[i], overlaps[i + 1]) for i in range(len(overlaps) - 1)], bool)


def post_process_overlaps(overlaps, drop_fused_overlaps=False):
    overlaps = np.ascontiguousarray(overlaps, OVERLAP)
    n = len(overlaps)
    fused, drop = [], np.zeros(n, bool)
    in_fuse, prev = False, None
    qs = ts = qe = te = res = 0

    def emit():
        f = prev.copy()
        f["query_start_position_in_read"], f["target_start_position_in_read"] = qs, ts
        f["query_end_position_in_read"], f["target_end_position_in_read"] = qe, te
        f["num_residues"] = res & U32
        fused.append(f)

    for i in range(1, n):
        prev, cur = overlaps[i - 1], overlaps[i]
        forward = int(cur["relative_strand"]) == ord("+")
        if overlaps_mergable(prev, cur):
            drop[i] = drop[i - 1] = True
            if not in_fuse:
                in_fuse = True
                res = int(prev["num_residues"]) + int(cur["num_residues"])
                qs, qe = int(prev["query_start_position_in_read"]), int(cur["query_end_position_in_read"])
                if forward:
                    ts, te = int(prev["target_start_position_in_read"]), int(cur["target_end_position_in_read"])
                else:
                    ts, te = int(cur["target_start_position_in_read"]), int(prev["target_end_position_in_read"])
            else:
                res += int(cur["num_residues"])
                qe = int(cur["query_end_position_in_read"])
                if forward:
                    te = int(cur["target_end_position_in_read"])
                else:
                    ts = int(cur["target_start_position_in_read"])
        elif in_fuse:
            in_fuse = False
            emit()
    if in_fuse:
        emit()  # prev is still overlaps[n - 2]
    kept = overlaps[~drop] if drop_fused_overlaps else overlaps
    out = np.zeros(len(kept) + len(fused), OVERLAP)
    out[:len(kept)] = kept
    for j, f in enumerate(fused):
        out[len(kept) + j] = f
    return out


def drop_overlaps_by_mask(overlaps, mask):
    mask = np.asarray(mask, bool)
    keep = np.ones(len(overlaps), bool)
    m = min(len(mask), len(overlaps))
    keep[:m] = ~mask[:m]
    return overlaps[keep]


def split_into_kmers(s, kmer_size, stride=1):
    if len(s) < kmer_size:
        return [s]
    return [s[i:i + kmer_size] for i in range(0, len(s) - kmer_size + 1, stride)]


def count_shared_elements(a, b):
    """elements of two sorted lists matched one to one"""
    ca, cb = Counter(a), Counter(b)
    return sum(min(c, cb[k]) for k, c in ca.items())


def sequence_jaccard_similarity(a, b, kmer_size, stride=1):
    ka, kb = split_into_kmers(a, kmer_size, stride), split_into_kmers(b, kmer_size, stride)
    shared = count_shared_elements(ka, kb)
    return _f32_div(shared, len(ka) + len(kb) - shared)


def reverse_complement(s):
    """The reference swaps and complements len / 2 pairs in place, so the middle base of an odd-length read is left as
    it is, uncomplemented."""
    r = bytearray(s.translate(_COMP)[::-1])
    if len(s) % 2:
        r[len(s) // 2] = s[len(s) // 2]
    return bytes(r)


def extend_overlap_by_sequence_similarity(o, query, target, extension, required_similarity, moved=None):
    """o: dict with qs, qe, ts, te (forward coordinates), updated in place. `moved`, if given, collects (head moved,
    tail moved, head window, tail window) per call."""
    req = float(np.float32(required_similarity))
    ext = extension & U32
    head = min(o["qs"], o["ts"], ext)
    sim = sequence_jaccard_similarity(query[o["qs"] - head:o["qs"]], target[o["ts"] - head:o["ts"]], KMER, 1)
    head_moved = sim >= req
    if head_moved:
        o["qs"] -= head
        o["ts"] -= head
    tail = min(ext, (len(query) - o["qe"]) & U32, (len(target) - o["te"]) & U32)
    sim = sequence_jaccard_similarity(query[o["qe"]:o["qe"] + tail], target[o["te"]:o["te"] + tail], KMER, 1)
    tail_moved = sim >= req
    if tail_moved:
        o["qe"] += tail
        o["te"] += tail
    if moved is not None:
        moved.append((head_moved, tail_moved, head, tail))


def _as_bytes(reads):
    return [r.encode() if isinstance(r, str) else bytes(r) for r in reads]


def rescue_overlap_ends(overlaps, query_reads, target_reads, extension=50, required_similarity=0.5,
                        first_query_read_id=0, first_target_read_id=0, trace=None):
    """Returns the rescued copy. `trace`, if a list, receives per overlap the list of (head moved, tail moved, head
    window, tail window) of its rounds."""
    out = np.ascontiguousarray(overlaps, OVERLAP).copy()
    queries, targets = _as_bytes(query_reads), _as_bytes(target_reads)
    for o in out:
        qi, ti = int(o["query_read_id"]) - first_query_read_id, int(o["target_read_id"]) - first_target_read_id
        if not (0 <= qi < len(queries) and 0 <= ti < len(targets)):
            raise ValueError("read id outside the read set")
        q, t = queries[qi], targets[ti]
        if max(int(o["query_start_position_in_read"]), int(o["query_end_position_in_read"])) > len(q) or \
                max(int(o["target_start_position_in_read"]), int(o["target_end_position_in_read"])) > len(t):
            raise ValueError("overlap beyond its read")
    for o in out:
        q = queries[int(o["query_read_id"]) - first_query_read_id]
        t = targets[int(o["target_read_id"]) - first_target_read_id]
        s = dict(qs=int(o["query_start_position_in_read"]), qe=int(o["query_end_position_in_read"]),
                 ts=int(o["target_start_position_in_read"]), te=int(o["target_end_position_in_read"]))
        reverse = int(o["relative_strand"]) == ord("-")
        if reverse:
            s["ts"], s["te"] = len(t) - s["te"], len(t) - s["ts"]
            t = reverse_complement(t)
        prev = (s["qs"], s["qe"], s["ts"], s["te"])
        rounds = []
        for _ in range(3):
            extend_overlap_by_sequence_similarity(s, q, t, extension, required_similarity, rounds)
            if s["qe"] == prev[0] and s["qe"] == prev[1] and s["ts"] == prev[2] and s["te"] == prev[3]:
                break
            prev = (s["qs"], s["qe"], s["ts"], s["te"])
        if reverse:
            s["ts"], s["te"] = len(t) - s["te"], len(t) - s["ts"]
        o["query_start_position_in_read"], o["query_end_position_in_read"] = s["qs"], s["qe"]
        o["target_start_position_in_read"], o["target_end_position_in_read"] = s["ts"], s["te"]
        if trace is not None:
            trace.append(rounds)
    return out


def group_reads_into_indices(read_lengths, max_basepairs_per_index):
    """[(first_read, number_of_reads)], the loop as the reference runs it (a first read longer than the limit leaves a
    descriptor of zero reads in front; no reads give [(0, 0)])"""
    out, first, count, bases = [], 0, 0, 0
    for i, n in enumerate(read_lengths):
        if int(n) + bases > max_basepairs_per_index:
            out.append((first, count))
            first, count, bases = i, 1, int(n)
        else:
            bases += int(n)
            count += 1
    out.append((first, count))
    return out


def format_paf(overlaps, query_names, query_lengths, target_names, target_lengths, kmer_size,
               first_query_read_id=0, first_target_read_id=0):
    lines = []
    for o in overlaps:
        qi, ti = int(o["query_read_id"]) - first_query_read_id, int(o["target_read_id"]) - first_target_read_id
        qs, qe = int(o["query_start_position_in_read"]), int(o["query_end_position_in_read"])
        ts, te = int(o["target_start_position_in_read"]), int(o["target_end_position_in_read"])
        res = (int(o["num_residues"]) * kmer_size) & U32
        res = res - (1 << 32) if res >= 1 << 31 else res  # printed with %i
        lines.append("%s\t%d\t%d\t%d\t%c\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (
            query_names[qi], query_lengths[qi], _as_i32(qs), _as_i32(qe), int(o["relative_strand"]), target_names[ti],
            target_lengths[ti], _as_i32(ts), _as_i32(te), res, max(abs(ts - te), abs(qs - qe))))
    return "".join(lines)


def _as_i32(x):
    return x - (1 << 32) if x >= 1 << 31 else x


def map_batched(queries, targets, k, w, filtering_parameter, overlap_params, max_basepairs_per_index,
                max_basepairs_per_target_index=None, post_process=True, drop_fused_overlaps=False,
                rescue=False):
    """The walk of the reference's main.cu for one device, with tests/oracle_mapper.py for the per-pair stages."""
    import oracle_mapper as O
    all_to_all = targets is None
    if all_to_all:
        targets = queries
    t_limit = max_basepairs_per_index if max_basepairs_per_target_index is None else max_basepairs_per_target_index
    qd = group_reads_into_indices([len(r) for r in queries], max_basepairs_per_index)
    td = group_reads_into_indices([len(r) for r in targets], t_limit)
    parts = []
    for qf, qn in qd:
        for tf, tn in td:
            if qn == 0 or tn == 0 or (all_to_all and tf < qf):
                continue
            qi = O.index(queries[qf:qf + qn], k, w, True, filtering_parameter, first_read_id=qf)
            ti = O.index(targets[tf:tf + tn], k, w, True, filtering_parameter, first_read_id=tf)
            o = O.overlaps(O.anchors(qi, ti), all_to_all, **overlap_params)
            if post_process:
                o = post_process_overlaps(o, drop_fused_overlaps)
            if rescue:
                o = rescue_overlap_ends(o, queries, targets, 50, 0.5)
            parts.append(o)
    return np.concatenate(parts) if parts else np.zeros(0, OVERLAP)
