"""Pileups on one GPU next to the segments pass over the same records. Prints one JSON record and, with --out, writes
it.

Workloads: those of tools/bench_polish.py and tools/bench_correct.py -- a seeded random contig (--contig-kbp, default
200) with reads of ~--read-length bases (default 5000) from both strands at --coverage (default 30) with --read-error
(default 3 %) errors, and a draft of the contig with --draft-error (default 3 %) errors. The reads are mapped (k=15
w=10, fusion and end rescue, F=1) against the draft and against themselves as one set. For each, after one warm-up,
--repeats times over the records that polish() / correct_reads() align (rule 1 of INTEGRATION.md section 3j, the pairs
of rule C1 of section 3k):

  overlap_pileup / pair_pileup         gather, align and the pileup stage on the device, the counters copied out once;
  window_segments / pair_segments      the same alignments with the segment writer as their consumer (window 500);
  align_overlaps                       the same alignments as CIGAR text: what a pileup on the host would have to
                                       bring over and walk.

Device stage times are HIP events summed over the chunks; the others are host wall times. Medians over the repeats.
No threshold: the record says what was measured.

    python tools/bench_pileup.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--out profiles/pileup_bench.json]
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


def timed(call, *args):
    """(timings of one call with its wall time among them, its result)"""
    t = {}
    t0 = time.perf_counter()
    out = call(*args, timings=t)
    t["seconds"] = time.perf_counter() - t0
    return t, out


def measure(records, pileup, segments, segment_keys, cigars, repeats):
    """the stage times of the three consumers over `records`; each of the calls takes (records, timings=)"""
    for call in (pileup, segments, cigars):
        call(records[:64], timings={})  # code objects
    piles, segs, texts = [], [], []
    for _ in range(repeats):
        t, counts = timed(pileup, records)
        piles.append(t)
        t, _ = timed(segments, records)
        t["segments_of_all_roles"] = sum(t[k] for k in segment_keys)
        segs.append(t)
        t, (text, _) = timed(cigars, records)
        texts.append(t)
        print({k: round(v, 3) for k, v in piles[-1].items()}, {k: round(v, 3) for k, v in segs[-1].items()},
              file=sys.stderr, flush=True)
    columns = sum(sum(int(n) for n in "".join(c if c.isdigit() else " " for c in s).split()) for s in text)
    cigar_bytes = sum(len(s) for s in text)
    depth = [polisher.depth(p) for p in counts]
    pileup_ms, segments_ms = med(piles, "pileup"), med(segs, "segments_of_all_roles")
    return {"records": int(len(records)), "alignment_columns": columns, "owner_bases": int(sum(len(d) for d in depth)),
            "mean_depth": round(float(sum(int(d.sum()) for d in depth)) / max(sum(len(d) for d in depth), 1), 3),
            "pileup": {"device_ms": {k: med(piles, k) for k in ("gather", "align", "pileup")},
                       "wall_s": med(piles, "seconds"), "bytes_to_host": int(piles[-1]["bytes_to_host"])},
            "segments": {"device_ms": {k: med(segs, k) for k in ("gather", "align") + tuple(segment_keys)},
                         "wall_s": med(segs, "seconds"), "bytes_to_host": int(segs[-1]["bytes_to_host"])},
            "align_overlaps": {"device_ms": {k: med(texts, k) for k in ("gather", "align", "cigar_text")},
                               "wall_s": med(texts, "seconds"), "cigar_bytes": cigar_bytes},
            "pileup_stage_over_segments_stage": round(pileup_ms / segments_ms, 3) if segments_ms else None,
            "counter_bytes_over_cigar_bytes": round(24 * sum(len(d) for d in depth) / max(cigar_bytes, 1), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--draft-error", type=float, default=0.03)
    ap.add_argument("--window-length", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length, W = 2025, int(args.contig_kbp * 1000), args.window_length
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    draft = OPo.draft_of(OPo.genome_of(seed, length), args.draft_error, seed)
    mapping = dict(k=15, w=10, filtering_parameter=1.0)
    rec = {"metric": "pileups next to the segments pass over the same aligned records, stage times", "device": "gpu0",
           "contig_bases": length, "draft_bases": len(draft), "coverage": args.coverage, "reads": len(reads),
           "read_bases": sum(len(r) for r in reads), "mean_read_length": args.read_length,
           "read_error": args.read_error, "draft_error": args.draft_error, "mapping": mapping, "window_length": W,
           "repeats": args.repeats}
    o = cudamapper.map_reads_batched(reads, [draft], post_process=True, rescue_overlap_ends=True, **mapping)
    kept = o[polisher.one_overlap_per_read(o)]
    print("polishing:", len(o), "records,", len(kept), "kept", file=sys.stderr, flush=True)
    rec["polishing"] = measure(
        kept, lambda r, timings: cudamapper.overlap_pileup(r, reads, [draft], timings=timings),
        lambda r, timings: cudamapper.window_segments(r, reads, [draft], W, timings=timings), ("segments",),
        lambda r, timings: cudamapper.align_overlaps(r, reads, [draft], timings=timings), args.repeats)
    o = cudamapper.map_reads_batched(reads, None, post_process=True, rescue_overlap_ends=True, **mapping)
    pairs = o[cudamapper.select_pairs(o)]
    print("correction:", len(o), "records,", len(pairs), "pairs", file=sys.stderr, flush=True)
    rec["correction"] = measure(
        pairs, lambda r, timings: cudamapper.pair_pileup(r, reads, timings=timings),
        lambda r, timings: cudamapper.pair_segments(r, reads, W, timings=timings), ("segments", "query_role_segments"),
        lambda r, timings: cudamapper.align_overlaps(r, reads, timings=timings), args.repeats)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
