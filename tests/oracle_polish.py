"""CPU oracle of polishing: segments from the alignment states of the pinned Hirschberg +
Myers restatement (tests/oracle_mapper_align.py), the layer selection, the windows, and consensus by the POA oracle
(tests/oracle_poa.py), stitched. A second, independent formulation of the segments walks the CIGAR string with the
parser of tests/cigar_replay.py and takes positions from run lengths instead of per-column counts.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import cigar_replay as CR
import mapper_cases as MC
import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_poa as OP

SEGMENT = np.dtype([("overlap", "<u4"), ("window", "<u4"), ("target_first", "<u4"), ("target_last", "<u4"),
                    ("query_begin", "<u4"), ("query_end", "<u4")])

# the small case of the GPU tests: 22 reads of a 1500-base genome on both strands, 3 % errors
SMALL = dict(seed=11, genome_length=1500, coverage=12, mean_length=800, error_rate=0.03)
MAPPING = dict(k=15, w=10, filtering_parameter=1.0)


def genome_of(seed, genome_length):
    """the genome mapper_cases.synthetic_reads draws its reads from: the generator's first draw"""
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), genome_length).tobytes().decode()


def small_case(seed=SMALL["seed"]):
    """(reads, genome) of the small case"""
    c = dict(SMALL, seed=seed)
    return (MC.synthetic_reads(c["seed"], c["genome_length"], c["coverage"], c["mean_length"], c["error_rate"]),
            genome_of(c["seed"], c["genome_length"]))


def draft_of(genome, error_rate, seed):
    """`genome` with every base mutated with probability error_rate: equal thirds substitution, insertion, deletion"""
    rng = np.random.default_rng([seed, 77])
    out = []
    for c in genome:
        if rng.random() >= error_rate:
            out.append(c)
            continue
        kind = int(rng.integers(0, 3))
        other = "ACGT"[int(rng.integers(0, 4))]
        if kind == 0:
            out.append(other)
        elif kind == 1:
            out.append(c + other)
    return "".join(out)


def _fields(o):
    return (int(o["query_start_position_in_read"]), int(o["query_end_position_in_read"]),
            int(o["target_start_position_in_read"]), int(o["target_end_position_in_read"]),
            int(o["relative_strand"]) == ord("-"))


def segments_from_states(i, o, states, W):
    """The records of overlap i from its per-column states in forward column order, by the counts a(j) and b(j)."""
    qs, _, ts, te, reverse = _fields(o)
    found = {}
    a = b = 0
    for s in states:
        if s < 2:
            q = qs + a
            t = te - 1 - b if reverse else ts + b
            k = t // W
            if k in found:
                r = found[k]
                found[k] = (min(r[0], t), max(r[1], t), min(r[2], q), max(r[3], q + 1))
            else:
                found[k] = (t, t, q, q + 1)
        a += s != 2
        b += s != 3
    return [(i, k) + found[k] for k in sorted(found)]


def segments_from_cigar(i, o, cigar, W):
    """The same records from the CIGAR text (M: match and mismatch, I: target only, D: query only): every M run is a
    stretch of consecutive target and query positions, cut at the window boundaries by arithmetic."""
    qs, _, ts, te, reverse = _fields(o)
    found = {}
    q, used = qs, 0  # next query position, target bases of the slice used up
    for n, op in (CR.parse_cigar(cigar, "MID") if cigar else []):
        if op == "I":
            used += n
        elif op == "D":
            q += n
        else:
            lo, hi = (te - used - n, te - used - 1) if reverse else (ts + used, ts + used + n - 1)  # target positions
            for k in range(lo // W, hi // W + 1):
                first, last = max(lo, k * W), min(hi, (k + 1) * W - 1)
                # query positions of the stretch's ends
                qa, qb = (q + hi - last, q + hi - first) if reverse else (q + first - lo, q + last - lo)
                r = found.get(k)
                found[k] = (first, last, qa, qb + 1) if r is None else (min(r[0], first), max(r[1], last),
                                                                        min(r[2], qa), max(r[3], qb + 1))
            q += n
            used += n
    return [(i, k) + found[k] for k in sorted(found)]


def segments(overlaps, queries, targets, W, alignments=None, formulation="states", first_query_read_id=0,
             first_target_read_id=0):
    """(SEGMENT array, segment_offsets, edit_distances) of window_segments; `alignments` = OA.alignments(...) if the
    caller has them already"""
    if alignments is None:
        alignments = OA.alignments(overlaps, queries, targets, None, first_query_read_id, first_target_read_id)
    rows, offsets, edits = [], [0], []
    for i, (o, a) in enumerate(zip(overlaps, alignments)):
        ql = int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"])
        tl = int(o["target_end_position_in_read"]) - int(o["target_start_position_in_read"])
        if formulation == "states":
            rows += segments_from_states(i, o, a["states"], W)
        else:
            rows += segments_from_cigar(i, o, a["cigar"], W)
        offsets.append(len(rows))
        edits.append(a["edit_distance"] if a["states"] else (0 if ql == 0 and tl == 0 else -1))
    return np.array(rows, SEGMENT).reshape(-1), np.array(offsets, np.int64), np.array(edits, np.int32)


def select_layers(segs, overlaps, target_lengths, W, max_depth, first_query_read_id=0, first_target_read_id=0):
    """(plan, windows) as cudamapper.select_layers returns them"""
    kept = {}
    for i, o in enumerate(overlaps):
        q = int(o["query_read_id"])
        span = int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"])
        if q not in kept or span > kept[q][0]:
            kept[q] = (span, i)
    kept = {i for _, i in kept.values()}
    layers = {}
    for s in segs:
        i, k = int(s["overlap"]), int(s["window"])
        if i not in kept:
            continue
        o = overlaps[i]
        t = int(o["target_read_id"]) - first_target_read_id
        end_k = min((k + 1) * W, int(target_lengths[t]))
        n = int(s["query_end"]) - int(s["query_begin"])
        if int(s["target_first"]) - k * W <= W // 100 and end_k - 1 - int(s["target_last"]) <= W // 100 and 1 <= n <= 2 * W:
            layers.setdefault((t, k), []).append((int(s["target_first"]), i, int(s["query_begin"]), int(s["query_end"])))
    plan, windows = [], []
    for t, length in enumerate(target_lengths):
        for k in range((int(length) + W - 1) // W):
            first = len(plan)
            plan.append((1, t, k * W, min((k + 1) * W, int(length)), 0))
            for _, i, qb, qe in sorted(layers.get((t, k), []))[:max_depth]:
                o = overlaps[i]
                plan.append((0, int(o["query_read_id"]) - first_query_read_id, qb, qe,
                             int(int(o["relative_strand"]) == ord("-"))))
            windows.append((t, k, first, len(plan) - first))
    return plan, windows


def _bytes(r):
    return r.encode("latin-1") if isinstance(r, str) else bytes(r)


def windows(overlaps, queries, targets, W, max_depth, alignments=None):
    """[(target_read, window, [backbone, layer, ...])] with the sequences as bytes, as cudamapper.overlap_windows"""
    targets = queries if targets is None else targets
    segs, _, _ = segments(overlaps, queries, targets, W, alignments)
    plan, table = select_layers(segs, overlaps, [len(t) for t in targets], W, max_depth)
    sets = ([_bytes(r) for r in queries], [_bytes(r) for r in targets])
    seqs = []
    for which, read, begin, end, reverse in plan:
        s = sets[which][read][begin:end]
        seqs.append(s.translate(OA.COMPLEMENT)[::-1] if reverse else s)
    return [(t, k, seqs[first:first + n]) for t, k, first, n in table]


def poa_shape(W, max_depth, band_width):
    """(max_sequence_size, max_sequences_per_poa, band width) of the batch polish() runs: the band as cudapoa aligns
    it, to a multiple of 128, and reads of 2 W bases, or of the band's width where that is more"""
    band = (band_width + 127) // 128 * 128
    return max(2 * W, band), max_depth + 1, band


def polish(reads, targets, overlaps, W, max_depth, band_width=256, band_mode=1, alignments=None):
    """(polished targets, report) of polisher.polish with overlaps given: windows of fewer than 2 layers and windows
    whose POA fails keep their backbone; report rows are (target_read, window, layers, status, backbone_kept)."""
    wins = windows(overlaps, reads, targets, W, max_depth, alignments)
    polished = ["" for _ in targets]
    report = []
    with OP.Workspace(OP.make_cfg(*poa_shape(W, max_depth, band_width), band_mode)) as ws:
        for t, k, seqs in wins:
            status, text = None, seqs[0].decode("latin-1")
            if len(seqs) - 1 >= 2:
                r = ws.process(seqs)
                status = int(r["status"])
                if status == 0:
                    text = r["consensus"]
            report.append((t, k, len(seqs) - 1, status, status != 0))
            polished[t] += text
    return polished, report


def mapped_overlaps(reads, targets):
    """the oracle's mapping of the reads against the targets with post-processing and end rescue, as polish() maps"""
    import oracle_mapper_postprocess as P
    return P.map_batched(reads, targets, MAPPING["k"], MAPPING["w"], MAPPING["filtering_parameter"], MC.OVERLAP_PARAMS,
                         30_000_000, rescue=True)


def edit_distance(a, b):
    import oracle_aligner as A
    return A.hirschberg(a, b)["edit_distance"]
