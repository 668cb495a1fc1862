"""Read correction on one GPU, stage by stage. Prints one JSON record and, with --out, writes it.

Workload: the read set of tools/bench_polish.py -- a seeded random contig (--contig-kbp, default 200) with reads of
~--read-length bases (default 5000) from both strands at --coverage (default 30) with --read-error (default 3 %)
errors -- mapped against itself (k=15 w=10, fusion and end rescue, F=1), twice: as one set, which is what
correct_reads() does when it maps, and as two sets (the reads as queries and as targets), which returns self overlaps
and both directions of every pair. For each of the two mappings, after one warm-up, --repeats times:

  correct_reads(reads, overlaps=...)   pairs selected on the host, each aligned once, the records of both roles written
                                       on the device, the layers selected on the host, the windows gathered on the
                                       device, cudapoa over the windows with >= 2 layers, stitched;
  align_overlaps(non-self records)     every record of the mapping that is not a read with itself, aligned: what has to
                                       be aligned when both directions are kept. Same machine, same run.

Device stage times are HIP events summed over the chunks; the others are host wall times. Medians over the repeats.
No threshold: the record says what was measured.

--qualities gives the reads synthetic Phred strings (low Phred at the mutated bases,
tests/oracle_polish_quality.informative_qualities) and runs correct_reads(..., qualities=...) in the same repeats, next
to the run without; each mapping's record gains "with_qualities".

    python tools/bench_correct.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--qualities] [--min-mean-quality 10]
                                  [--out profiles/correct_bench.json]
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
import oracle_polish_quality as OQ  # noqa: E402
from genomeworks_amd import cudamapper, polisher  # noqa: E402


def med(rows, key):
    return round(statistics.median(r[key] for r in rows), 4)


def wall(r):
    return r["windows_seconds"] + r["poa_seconds"] + r["stitch_seconds"]


def measure(reads, overlaps, kw, repeats, qualities=None, min_mean_quality=10):
    """the stage times of correct_reads() over `overlaps` and the align time of all their non-self records; with
    qualities, those of correct_reads(..., qualities=...) as well"""
    others = overlaps[overlaps["query_read_id"] != overlaps["target_read_id"]]
    few = overlaps[(overlaps["query_read_id"] < 64) & (overlaps["target_read_id"] < 64)]
    polisher.correct_reads(reads[:64], overlaps=few, **kw)  # code objects, pools
    cudamapper.align_overlaps(others[:64], reads)
    if qualities:
        polisher.correct_reads(reads[:64], overlaps=few, qualities=qualities[:64], **kw)
    runs, both, weighted_runs = [], [], []
    for _ in range(repeats):
        t = {}
        _, report = polisher.correct_reads(reads, overlaps=overlaps, timings=t, **kw)
        runs.append(t)
        if qualities:
            t = {}
            _, weighted_report = polisher.correct_reads(reads, overlaps=overlaps, timings=t, qualities=qualities,
                                                        min_mean_quality=min_mean_quality, **kw)
            weighted_runs.append(t)
            print("with qualities", {k: round(v, 3) for k, v in t.items()}, file=sys.stderr, flush=True)
        c = {}
        t0 = time.perf_counter()
        cudamapper.align_overlaps(others, reads, timings=c)
        c["seconds"] = time.perf_counter() - t0
        both.append(c)
        print({k: round(v, 3) for k, v in t.items()}, {k: round(v, 3) for k, v in c.items()}, file=sys.stderr, flush=True)
    pairs_ms, others_ms = med(runs, "align"), med(both, "align")
    more = {}
    if qualities:
        more["with_qualities"] = {
            "min_mean_quality": min_mean_quality,
            "windows_through_poa": sum(1 for r in weighted_report if r["status"] is not None),
            "windows_corrected": sum(1 for r in weighted_report if not r["backbone_kept"]),
            "layers": sum(r["layers"] for r in weighted_report),
            "windows_step": {"device_ms": {k: med(weighted_runs, k) for k in ("gather", "align", "segments", "query_role_segments",
                                                                               "quality_sums", "window_gather", "weight_gather")},
                             "wall_s": med(weighted_runs, "windows_seconds"),
                             "bytes_to_host": int(weighted_runs[-1]["bytes_to_host"])},
            "poa": {"wall_s": med(weighted_runs, "poa_seconds")},
            "end_to_end_s": {"with": round(statistics.median(wall(r) for r in weighted_runs), 4),
                             "without": round(statistics.median(wall(r) for r in runs), 4)}}
    return dict(more, **{"records": int(len(overlaps)), "self_records": int(len(overlaps) - len(others)),
            "non_self_records": int(len(others)), "pairs": int(runs[-1]["pairs"]),
            "windows": len(report), "windows_through_poa": sum(1 for r in report if r["status"] is not None),
            "windows_corrected": sum(1 for r in report if not r["backbone_kept"]),
            "layers": sum(r["layers"] for r in report),
            "windows_step": {"device_ms": {k: med(runs, k) for k in ("gather", "align", "segments", "query_role_segments",
                                                                     "window_gather")},
                             "wall_s": med(runs, "windows_seconds"), "bytes_to_host": int(runs[-1]["bytes_to_host"]),
                             "segment_bytes": int(runs[-1]["segment_bytes"]),
                             "window_bases": int(runs[-1]["window_bases"])},
            "poa": {"wall_s": med(runs, "poa_seconds")}, "host_stitch": {"wall_s": med(runs, "stitch_seconds")},
            "align_ms_of_the_pairs": pairs_ms,
            "align_ms_of_every_non_self_record": others_ms,
            "align_overlaps_non_self_records": {"device_ms": {k: med(both, k) for k in ("gather", "align", "cigar_text")},
                                                "wall_s": med(both, "seconds")},
            "pairs_over_non_self_records": {"records": round(runs[-1]["pairs"] / max(len(others), 1), 4),
                                            "align_ms": round(pairs_ms / others_ms, 4) if others_ms else None}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--window-length", type=int, default=500)
    ap.add_argument("--max-depth", type=int, default=30)
    ap.add_argument("--band-width", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--qualities", action="store_true", help="also correct with synthetic base qualities")
    ap.add_argument("--min-mean-quality", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length = 2025, int(args.contig_kbp * 1000)
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    qualities = None
    if args.qualities:
        qualities = OQ.informative_qualities(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
        assert [len(q) for q in qualities] == [len(r) for r in reads]
    mapping = dict(k=15, w=10, filtering_parameter=1.0)
    kw = dict(window_length=args.window_length, max_depth=args.max_depth, band_width=args.band_width)
    rec = {"metric": "correction of a read set by itself, stage times", "device": "gpu0", "contig_bases": length,
           "coverage": args.coverage, "reads": len(reads), "read_bases": sum(len(r) for r in reads),
           "mean_read_length": args.read_length, "read_error": args.read_error, "mapping": mapping,
           "window_length": args.window_length, "max_depth": args.max_depth, "band_width": args.band_width,
           "band_mode": "static_band", "repeats": args.repeats}
    for name, targets in (("mapped_as_one_set", None), ("mapped_as_two_sets", reads)):
        map_timings = {}
        t0 = time.perf_counter()
        overlaps = cudamapper.map_reads_batched(reads, targets, post_process=True, rescue_overlap_ends=True,
                                                timings=map_timings, **mapping)
        map_s = time.perf_counter() - t0
        print(name, len(reads), "reads,", len(overlaps), "records", file=sys.stderr, flush=True)
        rec[name] = dict({"map": {"wall_s": round(map_s, 4),
                                  "device_ms": {k: round(float(map_timings[k]), 3)
                                                for k in ("chain_fuse_filter", "fuse", "rescue")}}},
                         **measure(reads, overlaps, kw, args.repeats, qualities, args.min_mean_quality))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
