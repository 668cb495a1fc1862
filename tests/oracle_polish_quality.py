"""CPU oracle of the base-quality weights of polishing and read correction, on top of the
polishing and the read-correction oracles (tests/oracle_polish.py, tests/oracle_correct.py), which are imported and
not edited: the quality sums of the segment records (Q1), the selection with the quality filter (Q2), the weights of
the window sequences (Q3), and the two pipelines with weighted consensus by the POA oracle (Q4). It also holds the
deterministic quality generator of the tests. TEST INFRASTRUCTURE ONLY."""
import numpy as np

import mapper_cases as MC
import oracle_correct as OC
import oracle_mapper_align as OA
import oracle_poa as OP
import oracle_polish as OPo

SATURATED = 2 ** 32 - 1


def qualities_for(reads, seed=5, zero_read=3):
    """Phred+33 strings for `reads`: per read, bytes drawn from Phred 2..40 with a seeded default_rng; every fifth read
    (0, 5, 10, ...) from Phred 2..8, so that its mean lies below 10; read `zero_read` nothing but '!' (Phred 0)."""
    rng = np.random.default_rng([seed, 4099])
    out = []
    for i, r in enumerate(reads):
        low, high = (2, 8) if i % 5 == 0 else (2, 40)
        q = rng.integers(low, high + 1, len(r)).astype(np.uint8) + 33
        if i == zero_read:
            q[:] = 33
        out.append(q.tobytes().decode("latin-1"))
    return out


def informative_qualities(seed, genome_length, coverage, mean_length, error_rate, min_length=1):
    """Phred+33 strings for mapper_cases.synthetic_reads(the same arguments) that know where the errors are: the
    generator's draws are replayed to mark every substituted and every inserted base and the base in front of a
    deletion; marked bases get Phred 3..8, the others Phred 15..40 (a second, independent stream). For the
    benchmarks' --qualities: low Phred at the mutated bases."""
    rng = np.random.default_rng(seed)
    draw = np.random.default_rng([seed, 8191])
    rng.choice(np.frombuffer(b"ACGT", np.uint8), genome_length)  # the genome
    out = []
    for _ in range(max(1, int(genome_length * coverage / mean_length))):
        length = int(rng.integers(max(min_length, mean_length // 2), mean_length * 3 // 2 + 1))
        length = min(length, genome_length)
        rng.integers(0, genome_length - length + 1)
        u = rng.random(length)
        kind = rng.integers(0, 3, length)
        rng.choice(np.frombuffer(b"ACGT", np.uint8), length)
        hit = u < error_rate
        ins, deleted = hit & (kind == 1), hit & (kind == 2)
        marked = hit & (kind == 0)
        marked[:-1] |= deleted[1:]  # the base in front of a deleted one
        copies = np.where(ins, 2, 1)
        flags = np.repeat(marked, copies)
        flags[np.cumsum(copies) - 1] |= ins  # the inserted base stands behind the original
        flags = flags[np.repeat(~deleted, copies)]
        if rng.random() < 0.5:
            flags = flags[::-1]
        phred = np.where(flags, draw.integers(3, 9, len(flags)), draw.integers(15, 41, len(flags)))
        out.append((phred.astype(np.uint8) + 33).tobytes().decode("latin-1"))
    return out


def _q(quality):
    return np.frombuffer(quality.encode("latin-1") if isinstance(quality, str) else bytes(quality), np.uint8)


def check(qualities, reads):
    """what the public functions refuse: wrong lengths, bytes outside 33..126"""
    if len(qualities) != len(reads) or any(len(q) != len(r) for q, r in zip(qualities, reads)):
        raise ValueError("qualities do not match the reads")
    if any(len(q) and (_q(q).min() < 33 or _q(q).max() > 126) for q in qualities):
        raise ValueError("a quality byte outside 33..126")


def quality_sums(segs, overlaps, qualities, first_read_id=0, query_role=False):
    """Q1: per record the sum of c - 33 over the supplier's bytes [query_begin, query_end), forward coordinates,
    saturating at 2^32 - 1; the supplier is the overlap's query read, in the query role its target read"""
    field = "target_read_id" if query_role else "query_read_id"
    out = []
    for s in segs:
        q = _q(qualities[int(overlaps[int(s["overlap"])][field]) - first_read_id])
        total = int(q[int(s["query_begin"]):int(s["query_end"])].astype(np.int64).sum()) - 33 * (
            int(s["query_end"]) - int(s["query_begin"]))
        out.append(min(total, SATURATED))
    return np.array(out, np.uint32).reshape(-1)


def passes(total, bases, min_mean_quality):
    """Q2, in Python's unbounded integers"""
    return int(total) > 0 and int(total) >= int(min_mean_quality) * int(bases)


def _filtered(segs, sums, min_mean_quality):
    if sums is None:
        return segs
    if min_mean_quality < 0:
        raise ValueError("negative min_mean_quality")
    keep = [passes(t, int(s["query_end"]) - int(s["query_begin"]), min_mean_quality) for s, t in zip(segs, sums)]
    return segs[np.array(keep, bool)] if len(segs) else segs


def select_layers(segs, overlaps, target_lengths, W, max_depth, sums=None, min_mean_quality=0, first_query_read_id=0,
                  first_target_read_id=0):
    """(plan, windows) of cudamapper.select_layers with quality sums: the records that fail Q2 are gone before rule 2,
    the ordering and the max_depth cut see them; sums None is the unweighted selection"""
    return OPo.select_layers(_filtered(segs, sums, min_mean_quality), overlaps, target_lengths, W, max_depth,
                             first_query_read_id, first_target_read_id)


def select_correction_layers(target_role, query_role, pairs, read_lengths, W, max_depth, target_sums=None,
                             query_sums=None, min_mean_quality=0, first_read_id=0):
    return OC.select_correction_layers(_filtered(target_role, target_sums, min_mean_quality),
                                       _filtered(query_role, query_sums, min_mean_quality), pairs, read_lengths, W,
                                       max_depth, first_read_id)


def weights_of(plan, qualities_of_sets):
    """Q3: the weights of every sequence of a plan as np.int8 arrays; qualities_of_sets[set] is the list of quality
    strings of that set or None, which gives 1 throughout. Reversed entries back to front, nothing complemented."""
    out = []
    for which, read, begin, end, reverse in plan:
        if qualities_of_sets[which] is None:
            out.append(np.ones(end - begin, np.int8))
            continue
        w = (_q(qualities_of_sets[which][read])[begin:end].astype(np.int16) - 33).astype(np.int8)
        out.append(w[::-1].copy() if reverse else w)
    return out


def polish_windows(overlaps, queries, targets, W, max_depth, query_qualities=None, target_qualities=None,
                   min_mean_quality=10, alignments=None, segs=None):
    """[(target_read, window, [sequences], [weights])] as cudamapper.overlap_windows_weighted; `segs`: the records of
    window_segments where the caller has them already"""
    if segs is None:
        segs, _, _ = OPo.segments(overlaps, queries, targets, W, alignments)
    sums = None if query_qualities is None else quality_sums(segs, overlaps, query_qualities)
    plan, table = select_layers(segs, overlaps, [len(t) for t in targets], W, max_depth, sums, min_mean_quality)
    sets = ([OPo._bytes(r) for r in queries], [OPo._bytes(r) for r in targets])
    seqs = []
    for which, read, begin, end, reverse in plan:
        s = sets[which][read][begin:end]
        seqs.append(s.translate(OA.COMPLEMENT)[::-1] if reverse else s)
    weights = weights_of(plan, (query_qualities, target_qualities))
    return [(t, k, seqs[first:first + n], weights[first:first + n]) for t, k, first, n in table]


def correction_windows(overlaps, reads, qualities, W, max_depth, min_mean_quality=10, alignments=None, records=None):
    """[(read, window, [sequences], [weights])] as cudamapper.correction_windows_weighted; `alignments` of the pairs,
    or `records` = (target-role, query-role) records of pair_segments where the caller has them already"""
    pairs = overlaps[OC.select_pairs(overlaps)]
    if records is None:
        (target_role, _, _), (query_role, _) = OC.pair_segments(pairs, reads, W, alignments)
    else:
        target_role, query_role = records
    sums = (None, None) if qualities is None else (quality_sums(target_role, pairs, qualities),
                                                   quality_sums(query_role, pairs, qualities, query_role=True))
    plan, table = select_correction_layers(target_role, query_role, pairs, [len(r) for r in reads], W, max_depth,
                                           sums[0], sums[1], min_mean_quality)
    seqs = OC.cut(plan, reads)
    weights = weights_of(plan, (qualities, qualities))
    return [(r, k, seqs[first:first + n], weights[first:first + n]) for r, k, first, n in table]


def consensus_of(windows, n_reads, W, max_depth, band_width=256, band_mode=1):
    """Q4: (sequences, report rows) of weighted windows -- the POA oracle with the weights where at least 2 layers span
    the window and the backbone's weights do not sum to 0, the backbone otherwise"""
    out = ["" for _ in range(n_reads)]
    report = []
    with OP.Workspace(OP.make_cfg(*OPo.poa_shape(W, max_depth, band_width), band_mode)) as ws:
        for t, k, seqs, weights in windows:
            status, text = None, seqs[0].decode("latin-1")
            if len(seqs) - 1 >= 2 and int(weights[0].astype(np.int64).sum()) > 0:
                r = ws.process(seqs, weights)
                status = int(r["status"])
                if status == 0:
                    text = r["consensus"]
            report.append((t, k, len(seqs) - 1, status, status != 0))
            out[t] += text
    return out, report


def polish(reads, targets, overlaps, W, max_depth, band_width=256, band_mode=1, read_qualities=None,
           target_qualities=None, min_mean_quality=10, alignments=None, segs=None):
    """(polished targets, report rows) of polisher.polish with overlaps and qualities given"""
    wins = polish_windows(overlaps, reads, targets, W, max_depth, read_qualities, target_qualities, min_mean_quality,
                          alignments, segs)
    return consensus_of(wins, len(targets), W, max_depth, band_width, band_mode)


def correct(reads, overlaps, qualities, W, max_depth, band_width=256, band_mode=1, min_mean_quality=10,
            alignments=None, records=None):
    """(corrected reads, report rows) of polisher.correct_reads with overlaps and qualities given"""
    wins = correction_windows(overlaps, reads, qualities, W, max_depth, min_mean_quality, alignments, records)
    return consensus_of(wins, len(reads), W, max_depth, band_width, band_mode)


def paper_case():
    """The window of the issue: 333 bases, the backbone and two layers carry the same substitution at position 100,
    the third layer is the truth. Returns (truth, reads, weights) with the weights [unit, 2.., 2.., 40..]."""
    rng = np.random.default_rng(333)
    truth = "".join(rng.choice(list("ACGT"), 333))
    wrong = truth[:100] + "ACGT"[("ACGT".index(truth[100]) + 1) % 4] + truth[101:]
    reads = [wrong, wrong, wrong, truth]
    weights = [None, np.full(333, 2, np.int8), np.full(333, 2, np.int8), np.full(333, 40, np.int8)]
    return truth, reads, weights
