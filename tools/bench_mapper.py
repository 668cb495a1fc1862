"""Throughput of cudamapper (libcudamapper.so) on one GPU. Prints one JSON record.

Workloads (all-vs-all, hashed representations, F=1e-5, r=3 l=250 b=1000 z=0.8):
  covid      the reference's covid read fixture (3 000 reads, 1.15 Mbp), k=15 w=5 (the reference sample), one index;
  synthetic  a seeded 5 Mbp genome at 30x coverage of ~10 kbp reads with 5 % errors (both strands), k=15 w=10, reads
             grouped into indices of --index-mbp Mbp (the CLI's -i, default 30) and every index pair on or above the
             diagonal mapped, as the CLI does when the query and target files are the same.

Per workload: device time per stage from HIP events (sketch, index sort, unique, filter, match, anchor sort,
chain/fuse/filter), summed over the indices and pairs; bases indexed/s, anchors/s and overlaps/s over the summed device
time; wall time; and the single-thread C oracle (tests/oracle_mapper.c) on the same work as the CPU baseline (on the
first index pair only for synthetic, reported with its share of the bases).

    python tools/bench_mapper.py [--index-mbp 30] [--skip-synthetic] [--out record.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapper_cases as MC  # noqa: E402
import oracle_mapper as O  # noqa: E402
from genomeworks_amd import cudamapper  # noqa: E402

STAGES = ("sketch", "sort", "unique", "filter", "match", "anchor_sort", "chain_fuse_filter")


def group(reads, index_bases):
    """group_reads_into_indices: consecutive reads until an index holds index_bases bases"""
    groups, cur, size = [], [], 0
    for i, r in enumerate(reads):
        if cur and size + len(r) > index_bases:
            groups.append(cur)
            cur, size = [], 0
        cur.append(i)
        size += len(r)
    if cur:
        groups.append(cur)
    return groups


def run_gpu(reads, k, w, F, index_bases):
    groups = group(reads, index_bases)
    ms = dict.fromkeys(STAGES, 0.0)
    t0 = time.perf_counter()
    indices = []
    for g in groups:
        idx = cudamapper.Index([reads[i] for i in g], k, w, True, F, first_read_id=g[0])
        for s in ("sketch", "sort", "unique", "filter"):
            ms[s] += idx.stage_ms[s]
        indices.append(idx)
    n_anchors = n_overlaps = 0
    for qi in range(len(indices)):
        for ti in range(qi, len(indices)):
            m = cudamapper.Matcher(indices[qi], indices[ti])
            o = cudamapper.find_overlaps(m, True, **MC.OVERLAP_PARAMS)
            ms["match"] += m.stage_ms.get("match", 0.0)
            ms["anchor_sort"] += m.stage_ms.get("anchor_sort", 0.0)
            ms["chain_fuse_filter"] += m.stage_ms.get("chain_fuse_filter", 0.0)
            n_anchors += m.n_anchors
            n_overlaps += len(o)
            m.close()
    wall = time.perf_counter() - t0
    for idx in indices:
        idx.close()
    bases = sum(len(r) for r in reads)
    dev = sum(ms.values()) / 1e3
    return {"indices": len(groups), "index_pairs": len(groups) * (len(groups) + 1) // 2, "bases": bases,
            "anchors": n_anchors, "overlaps": n_overlaps, "stage_ms": {s: round(v, 3) for s, v in ms.items()},
            "device_ms": round(dev * 1e3, 3), "wall_s": round(wall, 3),
            "bases_indexed_per_s": round(bases / max(1e-9, sum(ms[s] for s in STAGES[:4]) / 1e3), 1),
            "anchors_per_s": round(n_anchors / max(1e-9, (ms["match"] + ms["anchor_sort"]) / 1e3), 1),
            "overlaps_per_s": round(n_overlaps / max(1e-9, ms["chain_fuse_filter"] / 1e3), 1)}


def run_cpu(reads, k, w, F):
    t0 = time.perf_counter()
    idx = O.index(reads, k, w, True, F)
    a = O.anchors(idx, idx)
    o = O.overlaps(a, True, **MC.OVERLAP_PARAMS)
    dt = time.perf_counter() - t0
    return {"seconds": round(dt, 3), "bases": sum(len(r) for r in reads), "anchors": len(a), "overlaps": len(o),
            "bases_per_s": round(sum(len(r) for r in reads) / dt, 1), "kind": "single-thread C oracle (gcc -O2)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mbp", type=float, default=30.0)
    ap.add_argument("--skip-synthetic", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    rec = {"metric": "cudamapper all-vs-all", "device": "gpu0"}
    covid = MC.covid_reads()[1]
    run_gpu(covid[:200], 15, 5, 1e-5, 1 << 40)  # warm-up: code objects, allocator
    rec["covid"] = dict(run_gpu(covid, 15, 5, 1e-5, 1 << 40), k=15, w=5, F=1e-5)
    rec["covid"]["cpu_baseline"] = run_cpu(covid, 15, 5, 1e-5)
    if not args.skip_synthetic:
        t0 = time.perf_counter()
        reads = MC.synthetic_reads(2024, 5_000_000, 30, 10_000, 0.05)
        gen = time.perf_counter() - t0
        index_bases = int(args.index_mbp * 1e6)
        rec["synthetic"] = dict(run_gpu(reads, 15, 10, 1e-5, index_bases), k=15, w=10, F=1e-5, reads=len(reads),
                                genome_mbp=5, coverage=30, error=0.05, generation_s=round(gen, 1))
        first = [reads[i] for i in group(reads, index_bases)[0]]
        rec["synthetic"]["cpu_baseline"] = dict(run_cpu(first, 15, 10, 1e-5), scope="first index against itself")
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
