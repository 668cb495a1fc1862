"""Anchored overlap alignment on one GPU next to the whole-slice path, in one process, on
the polishing workload of tools/bench_affine.py. Prints one JSON record and, with --out, writes it.

Workload: bench_affine.py's contig, reads and draft (the same seed and defaults). The reads are mapped against the
draft with overlapper="chained" (k=15 w=10, F=1, one index a set) with the chains handed out, and one overlap per read
is kept, as polish() keeps them; the records are not extended. Costs (4, 6, 2). After one warm-up, --repeats times each:

  whole       align_overlaps(..., scoring=(4, 6, 2, B)) for B of --bands (default 64 128);
  anchored    align_overlaps(..., scoring=(4, 6, 2, B), anchors=..., anchor_spacing=S) for B of --anchored-bands
              (default 16 32) at S = --spacing (default 256).

Per arm the medians of the gather, align and cigar_text stages (HIP events; the stitch is part of align), the in-band
cells and the aligner's workspace bytes (host arithmetic over the slices or the pieces), the records without a result,
and the alignments' costs re-priced from the CIGARs and edit distances; per anchored arm besides the number of pieces,
the distribution of their band widths W = |dm - dn| + 2 B + 1, the register variant K = the power of two at or above
ceil(W / 64) each piece would get alone against the K of the call (the aligner picks one K per call from the widest
band), and how many records cost less, the same or more than under the widest whole-slice band. No threshold: the
record says what was measured.

    python tools/bench_anchored.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--out profiles/anchored_align_bench.json]
"""
import argparse
import ctypes as C
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
import oracle_mapper_anchored as OG  # noqa: E402
import oracle_polish as OPo  # noqa: E402
from genomeworks_amd import cudamapper, polisher  # noqa: E402

COSTS = (4, 6, 2)


def med(values):
    return round(statistics.median(values), 4)


def band_cells(lengths, B):
    """the cells (i, j) of every pair with lo <= j - i <= hi, 0 <= i <= n, 0 <= j <= m"""
    total = 0
    for n, m in lengths:
        d = np.arange(min(0, m - n) - B, max(0, m - n) + B + 1)
        total += int(np.maximum(np.minimum(n, m - d) - np.maximum(0, -d) + 1, 0).sum())
    return total


def workspace_bytes(lengths, B):
    """gwhip_affine_workspace_bytes over these pairs"""
    L = C.CDLL(os.path.join(ROOT, "genomeworks_amd", "lib", "libgwaffine.so"))
    L.gwhip_affine_workspace_bytes.restype = C.c_size_t
    L.gwhip_affine_workspace_bytes.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_int32]
    starts = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64).reshape(-1))]).astype(np.int64)
    return int(L.gwhip_affine_workspace_bytes(len(lengths), starts.ctypes.data_as(C.POINTER(C.c_int64)), B))


def costs_of(cigars, edits):
    """the affine cost of every alignment from its CIGAR and its non-match columns; None where there is no result"""
    x, o, e = COSTS
    out = []
    for c, d in zip(cigars, edits.tolist()):
        if d < 0:
            out.append(None)
            continue
        runs = [int(n) for n in re.findall(r"(\d+)[ID]", c)]
        out.append(x * (d - sum(runs)) + sum(o + e * n for n in runs))
    return out


def arm(kept, reads, draft, scoring, repeats, **anchored):
    cudamapper.align_overlaps(kept[:64], reads, [draft], scoring=scoring)  # code objects
    stages = {"gather": [], "align": [], "cigar_text": []}
    for k in range(repeats + 1):  # the first is the warm-up
        t = {}
        cigars, edits = cudamapper.align_overlaps(kept, reads, [draft], scoring=scoring, timings=t, **anchored)
        if k:
            for name in stages:
                stages[name].append(t[name])
    costs = costs_of(cigars, edits)
    return {"gather_ms": med(stages["gather"]), "align_ms": med(stages["align"]), "cigar_text_ms": med(stages["cigar_text"]),
            "no_result": sum(c is None for c in costs), "cost_sum": sum(c for c in costs if c is not None)}, costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--draft-error", type=float, default=0.03)
    ap.add_argument("--bands", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--anchored-bands", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--spacing", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length = 2025, int(args.contig_kbp * 1000)
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    draft = OPo.draft_of(OPo.genome_of(seed, length), args.draft_error, seed)
    o, offsets, positions = cudamapper.map_reads(reads, [draft], k=15, w=10, filtering_parameter=1.0, overlapper="chained",
                                                 return_anchors=True)
    keep = polisher.one_overlap_per_read(o)
    kept = o[keep]
    per_record = [positions[int(offsets[i]):int(offsets[i + 1])] for i in keep]
    kept_offsets = np.cumsum([0] + [len(a) for a in per_record]).astype(np.int64)
    kept_positions = np.concatenate(per_record) if per_record else np.zeros((0, 2), np.uint32)
    print("chained:", len(o), "records,", len(kept), "kept,", len(kept_positions), "anchors", file=sys.stderr, flush=True)
    slices = [OG.lengths(x) for x in kept]
    plans = OG.plan(kept, kept_offsets, kept_positions, 15, args.spacing)
    pieces = [(dn, dm) for record in plans for _, _, dn, dm in record]
    rec = {"metric": "anchored overlap alignment of the polishing records next to the whole-slice path", "device": "gpu0",
           "contig_bases": length, "coverage": args.coverage, "reads": len(reads), "read_error": args.read_error,
           "draft_error": args.draft_error, "repeats": args.repeats, "records": int(len(kept)),
           "chain_anchors": int(len(kept_positions)), "slice_bases": int(sum(n + m for n, m in slices)),
           "costs": list(COSTS), "spacing": args.spacing, "pieces": len(pieces),
           "pieces_per_record_max": max(len(p) for p in plans), "piece_query_bases_max": max(dn for dn, _ in pieces),
           "piece_drift_max": max(abs(dn - dm) for dn, dm in pieces), "whole": {}, "anchored": {}}
    yardstick = None
    for B in args.bands:
        entry, costs = arm(kept, reads, draft, COSTS + (B,), args.repeats)
        entry.update(band_cells=band_cells(slices, B), workspace_bytes=workspace_bytes(slices, B))
        rec["whole"][str(B)] = entry
        yardstick = costs  # the widest whole-slice band comes last
        print("whole B", B, entry, file=sys.stderr, flush=True)
    variant = lambda W: min(32, 1 << max(0, (-(-W // 64) - 1).bit_length()))
    for B in args.anchored_bands:
        entry, costs = arm(kept, reads, draft, COSTS + (B,), args.repeats, anchors=(kept_offsets, kept_positions),
                           anchor_kmer_size=15, anchor_spacing=args.spacing)
        W = np.array([abs(dm - dn) + 2 * B + 1 for dn, dm in pieces])
        own = np.array([variant(int(w)) for w in W])
        both = [(a, b) for a, b in zip(costs, yardstick) if a is not None and b is not None]
        entry.update(band_cells=band_cells(pieces, B), workspace_bytes=workspace_bytes(pieces, B),
                     W={"min": int(W.min()), "median": int(np.median(W)), "p99": int(np.percentile(W, 99)), "max": int(W.max())},
                     K_of_the_call=variant(int(W.max())),
                     pieces_by_own_K={str(k): int((own == k).sum()) for k in sorted(set(own.tolist()))},
                     records_cheaper=sum(a < b for a, b in both), records_equal=sum(a == b for a, b in both),
                     records_dearer=sum(a > b for a, b in both), compared_with_whole_band=args.bands[-1])
        rec["anchored"][str(B)] = entry
        print("anchored B", B, entry, file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
