"""Device time of cudamapper's overlap post-processing (fusion, end rescue) on one GPU. Prints one JSON record.

Workload: the synthetic set of tools/bench_mapper.py (a seeded 5 Mbp genome at 30x coverage of ~10 kbp reads with 5 %
errors, both strands, k=15 w=10 F=1e-5, r=3 l=250 b=1000 z=0.8), reads grouped into indices of --index-mbp Mbp and
every index pair on or above the diagonal mapped, as the cudamapper tool does all-to-all. Per index pair the overlaps of
find_overlaps go through post_process_overlaps and rescue_overlap_ends(50, 0.5); the record holds the device time of
both (HIP events inside the library: kernels, rocPRIM calls, their allocations and host waits), summed and per pair,
overlaps/s over those sums, and the single-thread CPU oracle (tests/oracle_mapper_postprocess.py, plain Python) on the
first index pair as the baseline.

    python tools/bench_mapper_postprocess.py [--index-mbp 30] [--out profiles/mapper_postprocess.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mapper_cases as MC  # noqa: E402
import oracle_mapper_postprocess as P  # noqa: E402
from bench_mapper import group  # noqa: E402
from genomeworks_amd import cudamapper  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mbp", type=float, default=30.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    k, w, F = 15, 10, 1e-5
    genome_mbp, coverage = 5.0, 30.0
    reads = MC.synthetic_reads(2024, int(genome_mbp * 1e6), coverage, 10_000, 0.05)
    groups = group(reads, int(args.index_mbp * 1e6))
    print(len(reads), "reads in", len(groups), "indices", file=sys.stderr, flush=True)
    warm = reads[:40]
    o = cudamapper.map_reads(warm, filtering_parameter=1.0)  # warm-up: code objects, allocator
    cudamapper.rescue_overlap_ends(cudamapper.post_process_overlaps(o), warm)

    indices = [cudamapper.Index([reads[i] for i in g], k, w, True, F, first_read_id=g[0]) for g in groups]
    pairs, first_pair = [], None
    total = dict(overlaps_in=0, fused_records=0, overlaps_out=0, ends_moved=0, fuse_ms=0.0, rescue_ms=0.0,
                 chain_fuse_filter_ms=0.0)
    t0 = time.perf_counter()
    for qi in range(len(indices)):
        for ti in range(qi, len(indices)):
            m = cudamapper.Matcher(indices[qi], indices[ti])
            found = cudamapper.find_overlaps(m, True, **MC.OVERLAP_PARAMS)
            t = {}
            fused = cudamapper.post_process_overlaps(found, timings=t)
            rescued = cudamapper.rescue_overlap_ends(fused, reads, timings=t)
            moved = int(((rescued["query_start_position_in_read"] != fused["query_start_position_in_read"]) |
                         (rescued["query_end_position_in_read"] != fused["query_end_position_in_read"])).sum())
            pairs.append(dict(query_index=qi, target_index=ti, overlaps_in=len(found), overlaps_out=len(fused),
                              ends_moved=moved, fuse_ms=round(t["fuse"], 3), rescue_ms=round(t["rescue"], 3)))
            total["overlaps_in"] += len(found)
            total["fused_records"] += len(fused) - len(found)
            total["overlaps_out"] += len(fused)
            total["ends_moved"] += moved
            total["fuse_ms"] += t["fuse"]
            total["rescue_ms"] += t["rescue"]
            total["chain_fuse_filter_ms"] += m.stage_ms.get("chain_fuse_filter", 0.0)
            if first_pair is None:
                first_pair = found
            print("pair", qi, ti, pairs[-1], file=sys.stderr, flush=True)
            m.close()
    wall = time.perf_counter() - t0
    for idx in indices:
        idx.close()
    rec = {"metric": "cudamapper overlap post-processing, all-vs-all", "device": "gpu0", "k": k, "w": w, "F": F,
           "genome_mbp": genome_mbp, "coverage": coverage, "reads": len(reads),
           "bases": sum(len(r) for r in reads), "indices": len(groups), "index_pairs": len(pairs),
           "extension": 50, "required_similarity": 0.5,
           **{key: round(v, 3) if isinstance(v, float) else v for key, v in total.items()},
           "fuse_overlaps_per_s": round(total["overlaps_in"] / max(1e-9, total["fuse_ms"] / 1e3), 1),
           "rescue_overlaps_per_s": round(total["overlaps_out"] / max(1e-9, total["rescue_ms"] / 1e3), 1),
           "wall_s_with_mapping_and_copies": round(wall, 3), "pairs": pairs}
    t0 = time.perf_counter()
    fused = P.post_process_overlaps(first_pair)
    t1 = time.perf_counter()
    rescued = P.rescue_overlap_ends(fused, reads, reads, 50, 0.5)
    t2 = time.perf_counter()
    same = bool((cudamapper.rescue_overlap_ends(cudamapper.post_process_overlaps(first_pair), reads) == rescued).all())
    rec["cpu_baseline"] = dict(kind="single-thread Python oracle", scope="first index pair",
                               overlaps_in=len(first_pair), overlaps_out=len(fused),
                               fuse_s=round(t1 - t0, 3), rescue_s=round(t2 - t1, 3), equals_gpu=same)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
