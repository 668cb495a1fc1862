"""Device time of the chaining overlapper (cudamapper.chain_overlaps) next to the triggered one (find_overlaps) on the
same device anchors, on one GPU. Writes one JSON record (default profiles/mapper_chain_bench.json) and prints it.

The anchors are those of tools/bench_mapper.py's workloads (all-vs-all, hashed representations, F=1e-5): the covid
fixture at k=15 w=5 in one index, and the seeded 5 Mbp genome at 30x of ~10 kbp reads with 5 % errors at k=15 w=10 in
indices of --index-mbp Mbp, every index pair on or above the diagonal. Per index pair both overlappers run on the
Matcher's anchors, alternating, --repeats times after one warm-up run of each; the times are HIP-event device times
(stage_ms["chain_dp"] and stage_ms["chain_fuse_filter"]), the median per pair summed over the pairs. Both go through
the default filter (r=3 l=250 b=1000 z=0.8); the chaining runs with its defaults (max_gap 5000, bandwidth 500,
min_chain_score 40, max_chains 4).

    python tools/bench_mapper_chain.py [--index-mbp 30] [--repeats 3] [--skip-synthetic] [--out record.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mapper_cases as MC  # noqa: E402
from bench_mapper import group  # noqa: E402
from genomeworks_amd import cudamapper  # noqa: E402


def count_groups(anchors):
    """runs of one (query read, target read) in the sorted anchors"""
    if len(anchors) == 0:
        return 0
    q, t = anchors["query_read_id"], anchors["target_read_id"]
    return 1 + int(np.count_nonzero((q[1:] != q[:-1]) | (t[1:] != t[:-1])))


def run(reads, k, w, F, index_bases, repeats, label):
    groups = group(reads, index_bases)
    indices = [cudamapper.Index([reads[i] for i in g], k, w, True, F, first_read_id=g[0]) for g in groups]
    total = dict(anchors=0, groups=0, chained_records=0, triggered_records=0)
    dp_ms, triggered_ms, per_repeat = 0.0, 0.0, [[0.0, 0.0] for _ in range(repeats)]
    for qi in range(len(indices)):
        for ti in range(qi, len(indices)):
            with cudamapper.Matcher(indices[qi], indices[ti]) as m:
                chained = cudamapper.chain_overlaps(m, k, **MC.OVERLAP_PARAMS)  # warm-up of both
                triggered = cudamapper.find_overlaps(m, True, **MC.OVERLAP_PARAMS)
                dp, tr = [], []
                for r in range(repeats):
                    cudamapper.chain_overlaps(m, k, **MC.OVERLAP_PARAMS)
                    dp.append(m.stage_ms["chain_dp"])
                    cudamapper.find_overlaps(m, True, **MC.OVERLAP_PARAMS)
                    tr.append(m.stage_ms["chain_fuse_filter"])
                    per_repeat[r][0] += dp[-1]
                    per_repeat[r][1] += tr[-1]
                dp_ms += statistics.median(dp)
                triggered_ms += statistics.median(tr)
                total["anchors"] += m.n_anchors
                total["chained_records"] += len(chained)
                total["triggered_records"] += len(triggered)
                total["groups"] += count_groups(m.anchors())
            print("%s: pair (%d, %d) of %d indices done" % (label, qi, ti, len(indices)), file=sys.stderr, flush=True)
    for idx in indices:
        idx.close()
    return dict(total, k=k, w=w, F=F, indices=len(indices), index_pairs=len(indices) * (len(indices) + 1) // 2,
                bases=sum(len(r) for r in reads), repeats=repeats,
                chain_dp_ms=round(dp_ms, 3), chain_fuse_filter_ms=round(triggered_ms, 3),
                chain_dp_ms_per_repeat=[round(a, 3) for a, _ in per_repeat],
                chain_fuse_filter_ms_per_repeat=[round(b, 3) for _, b in per_repeat],
                chain_dp_over_chain_fuse_filter=round(dp_ms / max(triggered_ms, 1e-9), 2),
                chain_dp_anchors_per_s=round(total["anchors"] / max(dp_ms / 1e3, 1e-12), 1),
                chain_fuse_filter_anchors_per_s=round(total["anchors"] / max(triggered_ms / 1e3, 1e-12), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mbp", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-synthetic", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapper_chain_bench.json"))
    args = ap.parse_args()
    rec = {"metric": "cudamapper overlappers on the same anchors: chain_dp vs chain_fuse_filter (device ms, HIP events)",
           "device": "gpu0", "chaining": dict(cudamapper.CHAINING_DEFAULTS), "filter": MC.OVERLAP_PARAMS}
    covid = MC.covid_reads()[1]
    run(covid[:200], 15, 5, 1e-5, 1 << 40, 1, "warm-up")  # code objects, allocator
    rec["covid"] = run(covid, 15, 5, 1e-5, 1 << 40, args.repeats, "covid")
    if not args.skip_synthetic:
        t0 = time.perf_counter()
        reads = MC.synthetic_reads(2024, 5_000_000, 30, 10_000, 0.05)
        print("synthetic reads generated in %.1f s" % (time.perf_counter() - t0), file=sys.stderr, flush=True)
        rec["synthetic"] = dict(run(reads, 15, 10, 1e-5, int(args.index_mbp * 1e6), args.repeats, "synthetic"),
                                reads=len(reads), genome_mbp=5, coverage=30, error=0.05)
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
