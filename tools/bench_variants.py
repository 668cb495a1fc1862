"""Variant calling on one GPU next to the pileup over the same records, in one process. Prints one JSON record and,
with --out, writes it.

Workload: the polishing one of tools/bench_pileup.py -- a seeded random contig (--contig-kbp, default 200) with reads of
~--read-length bases (default 5000) from both strands at --coverage (default 30) with --read-error (default 3 %)
errors, and a draft of the contig with --draft-error (default 3 %) errors. The reads are mapped (k=15 w=10, fusion and
end rescue, F=1) against the draft. After one warm-up, --repeats times over the records that polish() aligns (rule 1 of
INTEGRATION.md section 3j), alternating:

  overlap_variants      gather, align, pileup + insertion-run records, vote + call on the device; the records copied out;
  overlap_pileup        the same alignments with the pileup alone as their consumer, the counters copied out.

Device stage times are HIP events (the first three summed over the chunks); medians over the repeats. The cost of
calling is reported as shares of the same run's align stage: `call` itself, and what the insertion-run records add to
the chunk consumer (overlap_variants' pileup stage less overlap_pileup's). No threshold: the record says what was
measured.

    python tools/bench_variants.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--out profiles/variants_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapper_cases as MC  # noqa: E402
import oracle_polish as OPo  # noqa: E402
from genomeworks_amd import cudamapper, polisher  # noqa: E402


def med(rows, key):
    return round(statistics.median(r[key] for r in rows), 4)


def timed(call, *args, **kw):
    """(timings of one call with its wall time among them, its result)"""
    t = {}
    t0 = time.perf_counter()
    out = call(*args, timings=t, **kw)
    t["seconds"] = time.perf_counter() - t0
    return t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--draft-error", type=float, default=0.03)
    ap.add_argument("--min-count", type=int, default=3)
    ap.add_argument("--min-percent", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length = 2025, int(args.contig_kbp * 1000)
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    draft = OPo.draft_of(OPo.genome_of(seed, length), args.draft_error, seed)
    mapping = dict(k=15, w=10, filtering_parameter=1.0)
    rec = {"metric": "variant calling next to the pileup over the same aligned records, stage times", "device": "gpu0",
           "contig_bases": length, "draft_bases": len(draft), "coverage": args.coverage, "reads": len(reads),
           "read_bases": sum(len(r) for r in reads), "mean_read_length": args.read_length,
           "read_error": args.read_error, "draft_error": args.draft_error, "mapping": mapping,
           "min_count": args.min_count, "min_percent": args.min_percent, "repeats": args.repeats}
    o = cudamapper.map_reads_batched(reads, [draft], post_process=True, rescue_overlap_ends=True, **mapping)
    kept = o[polisher.one_overlap_per_read(o)]
    print("polishing:", len(o), "records,", len(kept), "kept", file=sys.stderr, flush=True)
    thresholds = dict(min_count=args.min_count, min_percent=args.min_percent)
    cudamapper.overlap_variants(kept[:64], reads, [draft], **thresholds)  # code objects
    cudamapper.overlap_pileup(kept[:64], reads, [draft])
    called, piled = [], []
    for _ in range(args.repeats):
        t, records = timed(cudamapper.overlap_variants, kept, reads, [draft], **thresholds)
        called.append(t)
        t, piles = timed(cudamapper.overlap_pileup, kept, reads, [draft])
        piled.append(t)
        print({k: round(v, 3) for k, v in called[-1].items()}, {k: round(v, 3) for k, v in piled[-1].items()},
              file=sys.stderr, flush=True)
    align_ms = med(called, "align")
    runs_ms = round(med(called, "pileup") - med(piled, "pileup"), 4)
    rec.update({
        "records": int(len(kept)), "owner_bases": len(draft),
        "mean_depth": round(float(polisher.depth(piles[0]).sum()) / max(len(draft), 1), 3),
        "insertion_runs_counted": int(piles[0][5].sum()),
        "variants": {kind: int((records["kind"] == i).sum()) for i, kind in enumerate(cudamapper.VARIANT_KINDS)},
        "overlap_variants": {"device_ms": {k: med(called, k) for k in ("gather", "align", "pileup", "call")},
                             "wall_s": med(called, "seconds"), "bytes_to_host": int(called[-1]["bytes_to_host"])},
        "overlap_pileup": {"device_ms": {k: med(piled, k) for k in ("gather", "align", "pileup")},
                           "wall_s": med(piled, "seconds"), "bytes_to_host": int(piled[-1]["bytes_to_host"])},
        "run_records_ms": runs_ms,
        "call_over_align": round(med(called, "call") / align_ms, 4) if align_ms else None,
        "run_records_over_align": round(runs_ms / align_ms, 4) if align_ms else None})
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
