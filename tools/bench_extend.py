"""The affine X-drop extension on one GPU, on the ends of the polishing workload of tools/bench_polish.py, next to the
global affine aligner over the same slice pairs. Prints one JSON record and, with --out, writes it.

Workload: tools/bench_affine.py's (a seeded contig, reads of both strands, a draft with errors, one kept overlap per
read). Every kept overlap's ends are pulled in by --pull (default 200) bases, in the query and, in the target's strand
coordinates, in the target; then the 2 N slice pairs behind the tails and, read back to front, in front of the heads,
at most --max-extension (default 1024) bases each, are extended from the pulled ends through
CudaAlignerBatch(algorithm="extend") under (2, 4, 4, 2) and X = --xdrop (default 200). For every band B of --bands
(default 32 64 128), after one warm-up, the medians of --repeats runs:

  forward_ms, traceback_ms     by HIP events; cells per second of the forward pass over the cells of the anti-diagonals
                               that were computed are not known to the host, so the cells counted are those of the
                               whole band up to a_max: a lower bound of the rate for pairs that dropped;
  dropped_share                the share of extensions that the stop rule ended;
  mean_bases_recovered         the mean query_end per end (--pull bases lead back to the record's end; an overlap that
                               goes on behind it gives more);
  global_affine_forward_ms     the forward pass of the global affine aligner (CudaAlignerBatch(algorithm="affine"),
                               costs (4, 6, 2)) over the same 2 N pairs at the same B, in the same process, and
  forward_over_global_affine   the ratio of the two forward passes. The global band of a pair is |m - n| wider than
                               the extension's and the global pass runs to n + m, so this compares two jobs;
  prefixes_*                   both forward passes again over the aligned prefixes Q[:query_end], T[:target_end], the
                               extension at X = -1: nearly the same cells in both, so this ratio is what the stop
                               tracking costs per step.

No threshold: the record says what was measured.

    python tools/bench_extend.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--out profiles/extend_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapper_cases as MC  # noqa: E402
import oracle_polish as OPo  # noqa: E402
from genomeworks_amd import cudaaligner, cudamapper, polisher  # noqa: E402

SCORES = dict(match=2, mismatch=4, gap_open=4, gap_extend=2)


def med(values):
    return round(statistics.median(values), 4)


def reverse_complement(s):
    return "".join("TGAC"[(ord(c) >> 1) & 3] for c in reversed(s))


def end_pairs(kept, reads, draft, pull, most):
    """(head pair, tail pair) of every kept overlap whose ends can be pulled in by `pull`, in the target's strand coordinates"""
    complement = reverse_complement(draft)
    pairs = []
    for x in kept:
        q = reads[int(x["query_read_id"])]
        qs, qe = int(x["query_start_position_in_read"]) + pull, int(x["query_end_position_in_read"]) - pull
        ts, te = int(x["target_start_position_in_read"]), int(x["target_end_position_in_read"])
        t = draft
        if chr(x["relative_strand"]) == "-":
            t, ts, te = complement, len(draft) - te, len(draft) - ts
        ts, te = ts + pull, te - pull
        if qs >= qe or ts >= te:
            continue
        pairs.append((q[max(0, qs - most):qs][::-1], t[max(0, ts - most):ts][::-1]))
        pairs.append((q[qe:qe + most], t[te:te + most]))
    return pairs


def band_cells(lengths, B):
    """the cells of the extension's band up to a_max: |j - i| <= B, i <= n, j <= m"""
    total = 0
    for n, m in lengths:
        for d in range(-B, B + 1):
            total += max(min(n, m - d) - max(0, -d) + 1, 0)
    return total


def run(batch, pairs, repeats):
    forward, traceback = [], []
    for k in range(repeats + 1):  # the first is the warm-up
        batch.reset()
        for q, t in pairs:
            assert batch.add_alignment(q, t) == cudaaligner.success
        batch.align_all()
        batch.sync()
        f, tb = batch.stage_ms()
        if k:
            forward.append(f)
            traceback.append(tb)
    return med(forward), med(traceback)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--draft-error", type=float, default=0.03)
    ap.add_argument("--bands", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--pull", type=int, default=200)
    ap.add_argument("--max-extension", type=int, default=1024)
    ap.add_argument("--xdrop", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length = 2025, int(args.contig_kbp * 1000)
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    draft = OPo.draft_of(OPo.genome_of(seed, length), args.draft_error, seed)
    mapping = dict(k=15, w=10, filtering_parameter=1.0)
    o = cudamapper.map_reads_batched(reads, [draft], post_process=True, rescue_overlap_ends=True, **mapping)
    kept = o[polisher.one_overlap_per_read(o)]
    pairs = end_pairs(kept, reads, draft, args.pull, args.max_extension)
    print("polishing:", len(kept), "kept,", len(pairs), "end pairs", file=sys.stderr, flush=True)
    longest = max(max(len(q), len(t)) for q, t in pairs)
    rec = {"metric": "affine X-drop extension of the pulled-in ends of the polishing records next to the global affine aligner",
           "device": "gpu0", "contig_bases": length, "coverage": args.coverage, "reads": len(reads), "read_error": args.read_error,
           "draft_error": args.draft_error, "mapping": mapping, "repeats": args.repeats, "records": int(len(kept)),
           "end_pairs": len(pairs), "pulled_in": args.pull, "max_extension": args.max_extension, "scores": SCORES,
           "xdrop": args.xdrop, "slice_bases": sum(len(q) + len(t) for q, t in pairs), "bands": {}}
    memory = dict(max_device_memory_allocator_caching_size=16 << 30)
    for B in args.bands:
        batch = cudaaligner.CudaAlignerBatch(longest, longest, len(pairs), algorithm="extend", band_width=B, xdrop=args.xdrop,
                                             **SCORES, **memory)
        forward, traceback = run(batch, pairs, args.repeats)
        got = batch.get_alignments()
        del batch
        affine = cudaaligner.CudaAlignerBatch(longest, longest, len(pairs), algorithm="affine", band_width=B, **memory)
        global_forward, _ = run(affine, pairs, args.repeats)
        del affine
        # the cost of the stop tracking per step: both forward passes over the aligned prefixes, where the two bands hold
        # nearly the same cells (the global band is |m - n| wider), the extension never stopping
        prefixes = [(q[:a.query_end], t[:a.target_end]) for a, (q, t) in zip(got, pairs)]
        batch = cudaaligner.CudaAlignerBatch(longest, longest, len(pairs), algorithm="extend", band_width=B, xdrop=-1, **SCORES, **memory)
        prefix_forward, _ = run(batch, prefixes, args.repeats)
        del batch
        affine = cudaaligner.CudaAlignerBatch(longest, longest, len(pairs), algorithm="affine", band_width=B, **memory)
        prefix_global_forward, _ = run(affine, prefixes, args.repeats)
        del affine
        cells = band_cells([(len(q), len(t)) for q, t in pairs], B)
        rec["bands"][str(B)] = {
            "forward_ms": forward, "traceback_ms": traceback, "band_cells": cells,
            "band_cells_per_second": round(cells / (forward * 1e-3)),
            "dropped_share": round(sum(a.dropped for a in got) / len(got), 4),
            "mean_bases_recovered": round(sum(a.query_end for a in got) / len(got), 2),
            "global_affine_forward_ms": global_forward, "forward_over_global_affine": round(forward / global_forward, 3),
            "prefixes_forward_ms": prefix_forward, "prefixes_global_affine_forward_ms": prefix_global_forward,
            "prefixes_forward_over_global_affine": round(prefix_forward / prefix_global_forward, 3),
            "prefixes_widest_global_band": max(abs(len(q) - len(t)) for q, t in prefixes) + 2 * B + 1}
        print("B", B, rec["bands"][str(B)], file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
