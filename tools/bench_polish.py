"""Polishing on one GPU, stage by stage. Prints one JSON record and, with --out, writes it.

Workload: a seeded random contig (--contig-kbp, default 200) with reads of ~--read-length bases (default 5000) drawn
from both strands at --coverage (default 30) with --read-error (default 3 %) errors, and a draft of the contig with
--draft-error (default 3 %) errors: tests/mapper_cases.synthetic_reads and tests/oracle_polish.draft_of. The reads are
mapped against the draft (k=15 w=10, fusion and end rescue; the frequency filter is off, F=1, because at F=1e-5 an
index of this size keeps no representation at all) once; then, after one warm-up, --repeats times:

  polish(reads, [draft], overlaps=...)   the windows step (gather, align, segments on the device; selection on the host;
                                         window gather on the device) and cudapoa over the windows with >= 2 layers,
                                         stitched;
  align_overlaps(overlaps, ...)          the same overlaps to CIGAR text: its cigar_text stage is what the segments
                                         stage replaces, the gather and align stages are the same work.

Device stage times are HIP events summed over the chunks; the others are host wall times. Medians over the repeats.
Bytes to the host are counted from the shapes. No threshold: the record says what was measured.

--qualities gives the reads synthetic Phred strings that know where the errors are (low Phred at the mutated bases,
tests/oracle_polish_quality.informative_qualities) and runs, in the same repeats, polish(..., read_qualities=...) next
to the run without: the record gains "with_qualities" -- the quality_sums and weight_gather stages, the same stage and
wall times, bytes_to_host, the layers left by the filter -- and the edit distance of both results to the contig
(on the CPU, minutes at 200 kbp; --no-distance leaves it out).

    python tools/bench_polish.py [--contig-kbp 200] [--coverage 30] [--repeats 3] [--qualities] [--min-mean-quality 10]
                                 [--out profiles/polish_bench.json]
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
import oracle_polish_quality as OQ  # noqa: E402
from genomeworks_amd import cudamapper, polisher  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-kbp", type=float, default=200.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=5000)
    ap.add_argument("--read-error", type=float, default=0.03)
    ap.add_argument("--draft-error", type=float, default=0.03)
    ap.add_argument("--window-length", type=int, default=500)
    ap.add_argument("--max-depth", type=int, default=30)
    ap.add_argument("--band-width", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distance", action="store_true", help="edit distance of draft and result to the contig (CPU, slow)")
    ap.add_argument("--qualities", action="store_true", help="also polish with synthetic base qualities")
    ap.add_argument("--min-mean-quality", type=int, default=10)
    ap.add_argument("--no-distance", action="store_true", help="with --qualities: leave the edit distances out")
    ap.add_argument("--out")
    args = ap.parse_args()
    seed, length = 2025, int(args.contig_kbp * 1000)
    reads = MC.synthetic_reads(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
    qualities = None
    if args.qualities:
        qualities = OQ.informative_qualities(seed, length, args.coverage, args.read_length, args.read_error, min_length=200)
        assert [len(q) for q in qualities] == [len(r) for r in reads]
    contig = OPo.genome_of(seed, length)
    draft = OPo.draft_of(contig, args.draft_error, seed)
    mapping = dict(k=15, w=10, filtering_parameter=1.0)
    map_timings = {}
    t0 = time.perf_counter()
    overlaps = cudamapper.map_reads_batched(reads, [draft], post_process=True, rescue_overlap_ends=True,
                                            timings=map_timings, **mapping)
    map_s = time.perf_counter() - t0
    print(len(reads), "reads,", len(overlaps), "overlaps", file=sys.stderr, flush=True)
    kw = dict(window_length=args.window_length, max_depth=args.max_depth, band_width=args.band_width)
    polisher.polish(reads[:64], [draft], overlaps=overlaps[overlaps["query_read_id"] < 64], **kw)  # code objects, pools
    cudamapper.align_overlaps(overlaps[:64], reads, [draft])
    weighted_kw = dict(kw, read_qualities=qualities, min_mean_quality=args.min_mean_quality)
    if qualities:
        polisher.polish(reads[:64], [draft], overlaps=overlaps[overlaps["query_read_id"] < 64],
                        **dict(weighted_kw, read_qualities=qualities[:64]))
    runs, cigar_runs, weighted_runs = [], [], []
    for _ in range(args.repeats):
        t = {}
        polished, report = polisher.polish(reads, [draft], overlaps=overlaps, timings=t, **kw)
        runs.append(t)
        if qualities:
            t = {}
            weighted, weighted_report = polisher.polish(reads, [draft], overlaps=overlaps, timings=t, **weighted_kw)
            weighted_runs.append(t)
            print("with qualities", {k: round(v, 3) for k, v in t.items()}, file=sys.stderr, flush=True)
        c = {}
        t0 = time.perf_counter()
        cigars, _ = cudamapper.align_overlaps(overlaps, reads, [draft], timings=c)
        c["seconds"] = time.perf_counter() - t0
        cigar_runs.append(c)
        print({k: round(v, 3) for k, v in t.items()}, {k: round(v, 3) for k, v in c.items()}, file=sys.stderr, flush=True)

    def med(rows, key):
        return round(statistics.median(r[key] for r in rows), 4)
    stages_ms = {k: med(runs, k) for k in ("gather", "align", "segments", "window_gather")}
    rec = {"metric": "polishing of a draft contig by its reads, stage times", "device": "gpu0",
           "contig_bases": length, "draft_bases": len(draft), "coverage": args.coverage, "reads": len(reads),
           "read_bases": sum(len(r) for r in reads), "mean_read_length": args.read_length,
           "read_error": args.read_error, "draft_error": args.draft_error, "mapping": mapping,
           "overlaps": int(len(overlaps)), "window_length": args.window_length, "max_depth": args.max_depth,
           "band_width": args.band_width, "band_mode": "static_band", "repeats": args.repeats,
           "windows": len(report), "windows_through_poa": sum(1 for r in report if r["status"] is not None),
           "windows_polished": sum(1 for r in report if not r["backbone_kept"]),
           "layers": sum(r["layers"] for r in report),
           "map": {"wall_s": round(map_s, 4),
                   "device_ms": {k: round(float(map_timings[k]), 3) for k in ("chain_fuse_filter", "fuse", "rescue")}},
           "windows_step": {"device_ms": stages_ms, "wall_s": med(runs, "windows_seconds"),
                            "bytes_to_host": int(runs[-1]["bytes_to_host"]),
                            "segment_bytes": int(runs[-1]["segment_bytes"]), "window_bases": int(runs[-1]["window_bases"]),
                            "overlap_record_bytes": int(len(overlaps)) * 36},
           "poa": {"wall_s": med(runs, "poa_seconds")},
           "host_stitch": {"wall_s": med(runs, "stitch_seconds")},
           "polish_wall_s_per_repeat": [round(r["windows_seconds"] + r["poa_seconds"] + r["stitch_seconds"], 4) for r in runs],
           # what the segments stage replaces: the CIGAR writer of align_overlaps on the same overlaps
           "align_overlaps_same_overlaps": {"device_ms": {k: med(cigar_runs, k) for k in ("gather", "align", "cigar_text")},
                                            "wall_s": med(cigar_runs, "seconds"),
                                            "cigar_text_bytes": sum(len(c) for c in cigars)}}
    distances = args.distance or (qualities and not args.no_distance)
    if distances:
        rec["edit_distance_to_contig"] = {"draft": OPo.edit_distance(draft, contig),
                                          "polished": OPo.edit_distance(polished[0], contig)}
    if qualities:
        rec["with_qualities"] = {
            "qualities": "Phred 3..8 at the mutated bases, 15..40 elsewhere", "min_mean_quality": args.min_mean_quality,
            "windows_through_poa": sum(1 for r in weighted_report if r["status"] is not None),
            "windows_polished": sum(1 for r in weighted_report if not r["backbone_kept"]),
            "layers": sum(r["layers"] for r in weighted_report),
            "windows_step": {"device_ms": {k: med(weighted_runs, k) for k in ("gather", "align", "segments", "quality_sums",
                                                                               "window_gather", "weight_gather")},
                             "wall_s": med(weighted_runs, "windows_seconds"),
                             "bytes_to_host": int(weighted_runs[-1]["bytes_to_host"]),
                             "window_bases": int(weighted_runs[-1]["window_bases"])},
            "poa": {"wall_s": med(weighted_runs, "poa_seconds")},
            "host_stitch": {"wall_s": med(weighted_runs, "stitch_seconds")},
            "end_to_end_s": {"with": round(statistics.median(sum(r[k] for k in ("windows_seconds", "poa_seconds", "stitch_seconds")) for r in weighted_runs), 4),
                             "without": round(statistics.median(sum(r[k] for k in ("windows_seconds", "poa_seconds", "stitch_seconds")) for r in runs), 4)},
            "edit_distance_to_contig": OPo.edit_distance(weighted[0], contig) if distances else None}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
