"""The affine-gap global aligner on one GPU, on the polishing workload of tools/bench_polish.py, next to the unit-cost
path over the same records. Prints one JSON record and, with --out, writes it.

Workload: a seeded random contig (--contig-kbp, default 200) with reads of ~--read-length bases (default 5000) from
both strands at --coverage (default 30) with --read-error (default 3 %) errors, and a draft of the contig with
--draft-error (default 3 %) errors; the reads are mapped (k=15 w=10, fusion and end rescue, F=1) against the draft and
one overlap per read is kept, as polish() and call_variants() keep them. Costs (4, 6, 2). For every band B of --bands
(default 64 128 256), after one warm-up, --repeats times:

  aligner     the kept records' slices through CudaAlignerBatch(algorithm="affine"): the forward pass and the traceback
              by HIP events, the in-band cells per second of the forward pass, the share of alignments flagged optimal;
  mapper      align_overlaps(..., scoring=...) and overlap_variants(..., scoring=...): the align stage (offsets, forward
              pass, traceback), the number of gap runs in the CIGARs, the numbers of SNV, deleted-base and insertion
              records at the default thresholds.

And once, in the same process, the same two calls without a scoring: the align stage of the default aligner, its gap
runs and its records. Medians over the repeats. No threshold: the record says what was measured. Whether affine costs
improve the calls on real reads is not measured here; the counts say only how much the alignments change.

With --two-piece the arm that is measured is the two-piece aligner under (6, 4, 3, 24, 2),
and every band also holds the same measurements of the one-piece aligner under its first piece (6, 4, 3), from the same
process, with the two-piece forward pass over the one-piece forward pass; the gap runs of 20 columns or more are counted
under unit, one-piece and two-piece costs.

    python tools/bench_affine.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--out profiles/affine_bench.json]
    python tools/bench_affine.py --two-piece --out profiles/affine2_bench.json
"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapper_cases as MC  # noqa: E402
import oracle_polish as OPo  # noqa: E402
from genomeworks_amd import cudaaligner, cudamapper, polisher  # noqa: E402

COSTS = (4, 6, 2)
TWO_PIECE, ITS_FIRST_PIECE = (6, 4, 3, 24, 2), (6, 4, 3)


def med(values):
    return round(statistics.median(values), 4)


def gap_runs(cigars):
    return sum(c.count("I") + c.count("D") for c in cigars)


def long_gap_runs(cigars, least=20):
    return sum(1 for c in cigars for n in re.findall(r"(\d+)[ID]", c) if int(n) >= least)


def kinds(records):
    return {name: int((records["kind"] == k).sum()) for k, name in enumerate(("snv", "deleted_bases", "insertions"))}


def band_cells(lengths, B):
    """the cells (i, j) of every pair with lo <= j - i <= hi, 0 <= i <= n, 0 <= j <= m"""
    total = 0
    for n, m in lengths:
        d = np.arange(min(0, m - n) - B, max(0, m - n) + B + 1)
        total += int(np.maximum(np.minimum(n, m - d) - np.maximum(0, -d) + 1, 0).sum())
    return total


def mapper_side(kept, reads, draft, scoring, repeats):
    """the align stage, the gap runs and the records of align_overlaps / overlap_variants under `scoring` (None: unit costs)"""
    cudamapper.align_overlaps(kept[:64], reads, [draft], scoring=scoring)  # code objects
    align_ms, variants_align_ms = [], []
    for _ in range(repeats):
        t = {}
        cigars, edits = cudamapper.align_overlaps(kept, reads, [draft], scoring=scoring, timings=t)
        align_ms.append(t["align"])
        t = {}
        records = cudamapper.overlap_variants(kept, reads, [draft], scoring=scoring, timings=t)
        variants_align_ms.append(t["align"])
    return {"align_ms": med(align_ms), "overlap_variants_align_ms": med(variants_align_ms), "gap_runs": gap_runs(cigars),
            "gap_runs_of_20_or_more": long_gap_runs(cigars), "no_result": int((edits < 0).sum()), "non_match_columns": int(edits[edits >= 0].sum()),
            "variants": kinds(records)}


def aligner_side(pairs, B, repeats, costs=COSTS):
    """the forward pass and the traceback of the affine aligner over `pairs` at band B; five costs: the two-piece one"""
    longest = max(max(len(q), len(t)) for q, t in pairs)
    names = ("mismatch", "gap_open", "gap_extend", "gap_open2", "gap_extend2")
    batch = cudaaligner.CudaAlignerBatch(longest, longest, len(pairs), algorithm="affine", band_width=B,
                                         max_device_memory_allocator_caching_size=16 << 30, **dict(zip(names, costs)))
    forward, traceback = [], []
    for k in range(repeats + 1):  # the first is the warm-up
        batch.reset()
        for q, t in pairs:
            assert batch.add_alignment(q, t) == cudaaligner.success
        batch.align_all()
        runs = batch.get_runs()
        f, tb = batch.stage_ms()
        if k:
            forward.append(f)
            traceback.append(tb)
        print("B", B, "forward", round(f, 3), "traceback", round(tb, 3), file=sys.stderr, flush=True)
    cells = band_cells([(len(q), len(t)) for q, t in pairs], B)
    f, tb = med(forward), med(traceback)
    return {"forward_ms": f, "traceback_ms": tb, "traceback_over_forward": round(tb / f, 3), "band_cells": cells,
            "band_cells_per_second": round(cells / (f * 1e-3)), "optimal_share": round(float(runs["optimal"].mean()), 4),
            "with_result": int((runs["status"] == 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--draft-error", type=float, default=0.03)
    ap.add_argument("--bands", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--two-piece", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length = 2025, int(args.contig_kbp * 1000)
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    draft = OPo.draft_of(OPo.genome_of(seed, length), args.draft_error, seed)
    mapping = dict(k=15, w=10, filtering_parameter=1.0)
    o = cudamapper.map_reads_batched(reads, [draft], post_process=True, rescue_overlap_ends=True, **mapping)
    kept = o[polisher.one_overlap_per_read(o)]
    print("polishing:", len(o), "records,", len(kept), "kept", file=sys.stderr, flush=True)
    rc = lambda s: "".join("TGAC"[(ord(c) >> 1) & 3] for c in reversed(s))
    pairs = []
    for x in kept:
        q = reads[int(x["query_read_id"])][int(x["query_start_position_in_read"]):int(x["query_end_position_in_read"])]
        t = draft[int(x["target_start_position_in_read"]):int(x["target_end_position_in_read"])]
        pairs.append((q, rc(t) if chr(x["relative_strand"]) == "-" else t))
    costs = TWO_PIECE if args.two_piece else COSTS
    rec = {"metric": ("two-piece " if args.two_piece else "") + "affine-gap global alignment of the polishing records next to the unit-cost path", "device": "gpu0",
           "contig_bases": length, "draft_bases": len(draft), "coverage": args.coverage, "reads": len(reads),
           "read_bases": sum(len(r) for r in reads), "mean_read_length": args.read_length, "read_error": args.read_error,
           "draft_error": args.draft_error, "mapping": mapping, "repeats": args.repeats, "records": int(len(kept)),
           "slice_bases": sum(len(q) + len(t) for q, t in pairs), "costs": dict(zip(("mismatch", "gap_open", "gap_extend", "gap_open2", "gap_extend2"), costs)),
           "unit_costs": mapper_side(kept, reads, draft, None, args.repeats), "bands": {}}
    for B in args.bands:
        entry = aligner_side(pairs, B, args.repeats, costs)
        entry["mapper"] = mapper_side(kept, reads, draft, costs + (B,), args.repeats)
        entry["align_ms_over_unit_costs"] = round(entry["mapper"]["align_ms"] / rec["unit_costs"]["align_ms"], 3)
        if args.two_piece:
            one = aligner_side(pairs, B, args.repeats, ITS_FIRST_PIECE)
            one["costs"] = list(ITS_FIRST_PIECE)
            one["mapper"] = mapper_side(kept, reads, draft, ITS_FIRST_PIECE + (B,), args.repeats)
            entry["one_piece"] = one
            entry["forward_ms_over_one_piece"] = round(entry["forward_ms"] / one["forward_ms"], 3)
            entry["traceback_ms_over_one_piece"] = round(entry["traceback_ms"] / one["traceback_ms"], 3)
        rec["bands"][str(B)] = entry
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
