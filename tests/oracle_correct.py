"""CPU oracle of read correction, on top of the polishing oracle (tests/oracle_polish.py):
the pair selection (C1), the query-role records from the per-column alignment states and, as a second, independent
formulation, from the CIGAR string (C2), the layer selection over both roles (C3, C4), the windows, and the pipeline
with the POA oracle. TEST INFRASTRUCTURE ONLY."""
import numpy as np

import cigar_replay as CR
import mapper_cases as MC
import oracle_mapper_align as OA
import oracle_poa as OP
import oracle_polish as OPo

SEGMENT = OPo.SEGMENT


def reads_with_truth(seed, genome_length, n_reads, mean_length, error_rate):
    """(reads, true_reads): n_reads stretches of ~mean_length (uniform in [3 mean/4, 5 mean/4]) of a random genome, half
    of them reverse-complemented -- the true reads --, and the same with every base mutated with probability
    error_rate in equal thirds substitution, insertion and deletion."""
    rng = np.random.default_rng([seed, 3011])
    genome = "".join(rng.choice(list("ACGT"), genome_length))
    reads, truth = [], []
    for _ in range(n_reads):
        length = min(int(rng.integers(mean_length * 3 // 4, mean_length * 5 // 4 + 1)), genome_length)
        start = int(rng.integers(0, genome_length - length + 1))
        true = genome[start:start + length]
        if rng.random() < 0.5:
            true = true.translate(str.maketrans("ACGT", "TGCA"))[::-1]
        out = []
        for c in true:
            if rng.random() >= error_rate:
                out.append(c)
                continue
            kind = int(rng.integers(0, 3))
            other = "ACGT"[int(rng.integers(0, 4))]
            if kind == 0:
                out.append(other)
            elif kind == 1:
                out.append(c + other)
        truth.append(true)
        reads.append("".join(out))
    return reads, truth


def select_pairs(overlaps):
    """C1: the input positions of the records that are aligned, ascending"""
    best = {}
    for i, o in enumerate(overlaps):
        a, b = int(o["query_read_id"]), int(o["target_read_id"])
        if a == b:
            continue
        span = int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"])
        key = (min(a, b), max(a, b))
        if key not in best or span > best[key][0]:
            best[key] = (span, i)
    return sorted(i for _, i in best.values())


def query_role_from_states(i, o, states, W):
    """The query-role records of pair i from its per-column states in forward column order, by the counts a(j), b(j)."""
    qs, _, ts, te, reverse = OPo._fields(o)
    found = {}
    a = b = 0
    for s in states:
        if s < 2:
            q = qs + a
            t = te - 1 - b if reverse else ts + b
            k = q // W
            r = found.get(k)
            found[k] = (q, q, t, t + 1) if r is None else (min(r[0], q), max(r[1], q), min(r[2], t), max(r[3], t + 1))
        a += s != 2
        b += s != 3
    return [(i, k) + found[k] for k in sorted(found)]


def query_role_from_cigar(i, o, cigar, W):
    """The same records from the CIGAR text: an M run is a stretch of consecutive query positions, cut at the query's
    window boundaries by arithmetic; the target positions of a piece follow from its distance to the run's start."""
    qs, _, ts, te, reverse = OPo._fields(o)
    found = {}
    q, used = qs, 0
    for n, op in (CR.parse_cigar(cigar, "MID") if cigar else []):
        if op == "I":
            used += n
        elif op == "D":
            q += n
        else:
            for k in range(q // W, (q + n - 1) // W + 1):
                first, last = max(q, k * W), min(q + n - 1, (k + 1) * W - 1)
                if reverse:  # the run's first column has the largest target position
                    top = te - 1 - used
                    lo, hi = top - (last - q), top - (first - q)
                else:
                    lo, hi = ts + used + (first - q), ts + used + (last - q)
                r = found.get(k)
                found[k] = (first, last, lo, hi + 1) if r is None else (min(r[0], first), max(r[1], last),
                                                                        min(r[2], lo), max(r[3], hi + 1))
            q += n
            used += n
    return [(i, k) + found[k] for k in sorted(found)]


def pair_segments(pairs, reads, W, alignments=None, formulation="states", first_read_id=0):
    """((target-role SEGMENT array, offsets, edit_distances), (query-role SEGMENT array, offsets)) of
    cudamapper.pair_segments; `alignments` = OA.alignments(pairs, reads) if the caller has them already"""
    if alignments is None:
        alignments = OA.alignments(pairs, reads, None, None, first_read_id, first_read_id)
    target_role = OPo.segments(pairs, reads, reads, W, alignments, formulation, first_read_id, first_read_id)
    rows, offsets = [], [0]
    for i, (o, a) in enumerate(zip(pairs, alignments)):
        if formulation == "states":
            rows += query_role_from_states(i, o, a["states"], W)
        else:
            rows += query_role_from_cigar(i, o, a["cigar"], W)
        offsets.append(len(rows))
    return target_role, (np.array(rows, SEGMENT).reshape(-1), np.array(offsets, np.int64))


def select_correction_layers(target_role, query_role, pairs, read_lengths, W, max_depth, first_read_id=0):
    """C3 and C4: (plan, windows) as cudamapper.select_correction_layers returns them"""
    layers = {}
    for role, segs in enumerate((target_role, query_role)):
        for s in segs:
            i, k = int(s["overlap"]), int(s["window"])
            o = pairs[i]
            owner = int(o["query_read_id" if role else "target_read_id"]) - first_read_id
            other = int(o["target_read_id" if role else "query_read_id"]) - first_read_id
            end_k = min((k + 1) * W, int(read_lengths[owner]))
            n = int(s["query_end"]) - int(s["query_begin"])
            if (int(s["target_first"]) - k * W <= W // 100 and end_k - 1 - int(s["target_last"]) <= W // 100
                    and 1 <= n <= 2 * W):
                layers.setdefault((owner, k), []).append(
                    (int(s["target_first"]), i, role, other, int(s["query_begin"]), int(s["query_end"]),
                     int(int(o["relative_strand"]) == ord("-"))))
    plan, windows = [], []
    for r, length in enumerate(read_lengths):
        for k in range((int(length) + W - 1) // W):
            first = len(plan)
            plan.append((0, r, k * W, min((k + 1) * W, int(length)), 0))
            plan += [(0,) + layer[3:] for layer in sorted(layers.get((r, k), []))[:max_depth]]
            windows.append((r, k, first, len(plan) - first))
    return plan, windows


def windows(overlaps, reads, W, max_depth, alignments=None):
    """[(read, window, [backbone, layer, ...])] with the sequences as bytes, as cudamapper.correction_windows;
    `alignments` are those of the pairs"""
    pairs = overlaps[select_pairs(overlaps)]
    (target_role, _, _), (query_role, _) = pair_segments(pairs, reads, W, alignments)
    plan, table = select_correction_layers(target_role, query_role, pairs, [len(r) for r in reads], W, max_depth)
    seqs = cut(plan, reads)
    return [(r, k, seqs[first:first + n]) for r, k, first, n in table]


def cut(plan, reads):
    """the sequences of a plan of set 0 as bytes, reversed ones through the aligner's table"""
    data = [OPo._bytes(r) for r in reads]
    seqs = []
    for _, read, begin, end, reverse in plan:
        s = data[read][begin:end]
        seqs.append(s.translate(OA.COMPLEMENT)[::-1] if reverse else s)
    return seqs


def pair_alignments(overlaps, reads):
    """the oracle's alignments of the pairs of `overlaps`, for windows() and correct()"""
    return OA.alignments(overlaps[select_pairs(overlaps)], reads)


def correct(reads, overlaps, W, max_depth, band_width=256, band_mode=1, alignments=None):
    """(corrected reads, report) of polisher.correct_reads with overlaps given; report rows are (read, window, layers,
    status, backbone_kept)"""
    wins = windows(overlaps, reads, W, max_depth, alignments)
    corrected = ["" for _ in reads]
    report = []
    with OP.Workspace(OP.make_cfg(*OPo.poa_shape(W, max_depth, band_width), band_mode)) as ws:
        for r, k, seqs in wins:
            status, text = None, seqs[0].decode("latin-1")
            if len(seqs) - 1 >= 2:
                out = ws.process(seqs)
                status = int(out["status"])
                if status == 0:
                    text = out["consensus"]
            report.append((r, k, len(seqs) - 1, status, status != 0))
            corrected[r] += text
    return corrected, report


def mapped_all_against_all(reads):
    """the oracle's mapping of the reads against themselves as two sets: self overlaps and both directions of a pair
    are among the records, which is what C1 has to cope with"""
    import oracle_mapper_postprocess as P
    return P.map_batched(reads, reads, OPo.MAPPING["k"], OPo.MAPPING["w"], OPo.MAPPING["filtering_parameter"],
                         MC.OVERLAP_PARAMS, 30_000_000, rescue=True)


def summed_edit_distance(reads, truth):
    return sum(OPo.edit_distance(a, b) for a, b in zip(reads, truth))
