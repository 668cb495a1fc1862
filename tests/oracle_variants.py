"""CPU oracle of variant calling, on top of the pileup oracle (tests/oracle_pileup.py): the
counts are those of OPi.overlap_pileup, the insertion runs come from the CIGAR's D runs -- query bases between two
target bases, with positions and the both-neighbours condition as OPi.add_from_cigar has them -- or, as a second
formulation, from the per-column states, column by column; the allele comes from the query; then the vote, the
thresholds and the order. Also the host side of polisher.call_variants (joined deletions) and a reader of the VCF text
of polisher.format_vcf. The CIGAR formulation takes any CIGAR, so the GPU tests apply it to what align_overlaps()
returns. TEST INFRASTRUCTURE ONLY."""
from collections import Counter

import numpy as np

import cigar_replay as CR
import oracle_mapper_align as OA
import oracle_pileup as OPi
import oracle_polish as OPo

KINDS = ("snv", "deletion", "insertion")
SNV, DELETION, INSERTION = 0, 1, 2
LONGEST_RUN = 32
# gwm_variant of include/gwhip_mapper.h
VARIANT = np.dtype({"names": ["target_read", "position", "count", "depth", "kind", "ref", "alt", "length", "key"],
                    "formats": ["<u4", "<u4", "<u4", "<u4", "u1", "u1", "u1", "u1", "<u8"],
                    "offsets": [0, 4, 8, 12, 16, 17, 18, 19, 24], "itemsize": 32})


def pack_key(allele):
    """the key of an allele given as text"""
    key = 0
    for c in allele:
        key = key << 2 | "ACGT".index(c)
    return key


def allele_text(length, key):
    return "".join("ACGT"[(int(key) >> 2 * (int(length) - 1 - i)) & 3] for i in range(int(length)))


def _allele(query, q, n, reverse):
    """the n query bases from q on in forward target coordinates, as text after the aligner's folding"""
    codes = OPi.CHANNEL_OF[OPi._data(query)[q:q + n]]
    assert len(codes) == n
    if reverse:
        codes = 3 - codes[::-1]
    return "".join("ACGT"[c] for c in codes)


def runs_from_cigar(o, cigar, query):
    """[(p, allele)] of overlap o: every D run of the CIGAR with a target base on both sides, whatever its length"""
    qs, qe, ts, te, reverse = OPo._fields(o)
    runs = CR.parse_cigar(cigar, "MID") if cigar else []
    in_target = sum(n for n, op in runs if op != "D")
    q_used = t_used = 0
    out = []
    for n, op in runs:
        if op == "D":
            if 1 <= t_used <= in_target - 1:
                out.append((te - 1 - t_used if reverse else ts + t_used - 1, _allele(query, qs + q_used, n, reverse)))
            q_used += n
        else:
            q_used += n if op == "M" else 0
            t_used += n
    return out


def runs_from_states(o, states, query):
    """the same from the per-column states (forward column order), a column at a time"""
    qs, qe, ts, te, reverse = OPo._fields(o)
    B = sum(s != 3 for s in states)
    a = b = 0
    out, open_run = [], None  # open_run: [p or None, first query position, columns]
    for s in list(states) + [None]:
        if s == 3:
            if open_run is None:
                counted = 1 <= b <= B - 1
                open_run = [(te - 1 - b if reverse else ts + b - 1) if counted else None, qs + a, 0]
            open_run[2] += 1
        elif open_run is not None:
            if open_run[0] is not None:
                out.append((open_run[0], _allele(query, open_run[1], open_run[2], reverse)))
            open_run = None
        if s is not None:
            a += s != 2
            b += s != 3
    return out


def insertion_runs(overlaps, queries, n_targets, alignments, formulation, first_query_read_id=0, first_target_read_id=0):
    """per target read {p: Counter of the alleles of the run records there}: runs of 1..32 bases"""
    out = [dict() for _ in range(n_targets)]
    for o, a in zip(overlaps, alignments):
        query = queries[int(o["query_read_id"]) - first_query_read_id]
        runs = runs_from_states(o, a["states"], query) if formulation == "states" else runs_from_cigar(o, a["cigar"], query)
        for p, allele in runs:
            if 1 <= len(allele) <= LONGEST_RUN:
                out[int(o["target_read_id"]) - first_target_read_id].setdefault(p, Counter())[allele] += 1
    return out


def passes(k, d, min_count, min_percent):
    return k >= min_count and 100 * int(k) >= min_percent * int(d)


def best_allele(alleles):
    """(allele, records): the most records, then the shorter, then the alphabetically smaller"""
    return min(alleles.items(), key=lambda item: (-item[1], len(item[0]), item[0]))


def call(piles, targets, runs, min_count=3, min_percent=30):
    """the VARIANT records of the targets from their pileups and run records, in the order of the device"""
    rows = []
    for ti, (pile, target) in enumerate(zip(piles, targets)):
        own = OPi.CHANNEL_OF[OPi._data(target)]
        pile = pile.astype(np.int64)
        depth = pile[:5].sum(0)
        candidates = set(np.nonzero(pile[:5].sum(0))[0].tolist()) | set(runs[ti])
        for p in sorted(candidates):
            r, d = int(own[p]), int(depth[p])
            alt = max((c for c in range(4) if c != r), key=lambda c: (pile[c, p], -c))
            if passes(pile[alt, p], d, min_count, min_percent):
                rows.append((ti, p, int(pile[alt, p]), d, SNV, r, alt, 0, 0))
            if passes(pile[OPi.DELETION, p], d, min_count, min_percent):
                rows.append((ti, p, int(pile[OPi.DELETION, p]), d, DELETION, r, 0, 0, 0))
            if p in runs[ti]:
                allele, k = best_allele(runs[ti][p])
                if passes(k, d, min_count, min_percent):
                    rows.append((ti, p, k, d, INSERTION, r, 0, len(allele), pack_key(allele)))
    return np.array(rows, VARIANT).reshape(-1)


def overlap_variants(overlaps, queries, targets=None, alignments=None, formulation="cigar", min_count=3, min_percent=30,
                     first_query_read_id=0, first_target_read_id=0, return_pileup=False):
    """cudamapper.overlap_variants; `alignments` = OA.alignments(...) or OPi.of_cigars(...) if the caller has them"""
    targets = queries if targets is None else targets
    if alignments is None:
        alignments = OA.alignments(overlaps, queries, targets, None, first_query_read_id, first_target_read_id)
    piles = OPi.overlap_pileup(overlaps, queries, targets, alignments, "cigar", first_query_read_id, first_target_read_id)
    runs = insertion_runs(overlaps, queries, len(targets), alignments, formulation, first_query_read_id,
                          first_target_read_id)
    records = call(piles, targets, runs, min_count, min_percent)
    return (records, piles) if return_pileup else records


def join_deletions(records, targets):
    """the dicts of polisher.call_variants from VARIANT records: deleted neighbours of one target become one variant"""
    out = []
    for v in records:
        ti, p, kind = int(v["target_read"]), int(v["position"]), KINDS[int(v["kind"])]
        base = OPo._bytes(targets[ti])[p:p + 1].decode("latin-1")
        before = next((x for x in reversed(out) if x["kind"] == "deletion"), None)
        if kind == "deletion" and before and before["target"] == ti and before["position"] + len(before["ref"]) == p:
            before["ref"] += base
            before["count"] = min(before["count"], int(v["count"]))
            continue
        ref, alt = base, ""
        if kind == "snv":
            alt = "ACGT"[int(v["alt"])]
        if kind == "insertion":
            ref, alt = "", allele_text(v["length"], v["key"])
        out.append(dict(target=ti, position=p, kind=kind, ref=ref, alt=alt, count=int(v["count"]), depth=int(v["depth"])))
    return out


def call_variants(reads, targets, overlaps, alignments_of, min_count=3, min_percent=30):
    """polisher.call_variants with overlaps given; alignments_of(kept records) gives their alignments"""
    kept = overlaps[OPi.one_overlap_per_read(overlaps)]
    return join_deletions(overlap_variants(kept, reads, targets, alignments_of(kept), "cigar", min_count, min_percent),
                          targets)


def parse_vcf(text, target_names):
    """the variants a VCF text of polisher.format_vcf speaks of, as the dicts of call_variants, in file order, and the
    header lines"""
    header = [line for line in text.split("\n") if line.startswith("#")]
    out = []
    for line in text.split("\n"):
        if not line or line.startswith("#"):
            continue
        chrom, pos, ident, ref, alt, qual, flt, info = line.split("\t")
        assert (ident, qual, flt) == (".", ".", "PASS")
        info = dict(item.split("=") for item in info.split(";"))
        kind, pos = info["TYPE"], int(pos)
        v = dict(target=target_names.index(chrom), kind=kind, count=int(info["AD"]), depth=int(info["DP"]))
        if kind == "snv":
            v.update(position=pos - 1, ref=ref, alt=alt)
        elif kind == "insertion":
            assert alt[0] == ref and len(ref) == 1
            v.update(position=pos - 1, ref="", alt=alt[1:])
        elif ref.startswith(alt):  # the base before the deleted ones
            v.update(position=pos, ref=ref[1:], alt="")
        else:                      # a deletion from position 0 on: the base behind them
            assert pos == 1 and ref.endswith(alt)
            v.update(position=0, ref=ref[:-1], alt="")
        out.append(v)
    return out, header
