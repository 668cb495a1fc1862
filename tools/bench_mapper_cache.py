"""What cudamapper's index cache buys on one GPU: the batched driver of this tree at -Q 10 -q 5 -C 10 -c 5 and at
1, 1, 1, 1 against the driver of a baseline libcudamapper.so (the parent commit's, built apart and named with
--baseline-lib), on the seeded 5 Mbp x 30 read set of tools/bench_mapper.py, all against all, k=15 w=10 F=1e-5.

One process. After a warm-up of each, the three runs alternate `--repeats` times; the wall time of a run is taken around
the library call and a device synchronise behind it, with the reads already packed. Reported: the medians, the spread
(max - min) of each, the overlaps of the three runs compared as tests/test_gpu_mapper_cache.py compares them, the
builds / restores counted, and per index the packed restore time (copy and the two kernels, HIP events) beside the
four build stage times of the baseline library for the same index, and the packed size beside 17 n + 12 n_unique.

Acceptance (written into the record as booleans, and the exit status): the cached median is below the baseline median
by more than the larger of the two spreads; this tree at 1, 1, 1, 1 is not slower than the baseline beyond that spread;
the overlaps agree; every restore is faster than its build.

With --like-for-like the baseline library has the cached driver too and the question is whether this tree's driver
costs what the baseline's does: both are called through gw_mapper_map_batched_cached, at 1, 1, 1, 1 and at 10, 5, 10, 5,
the four runs alternating. Accepted when at each setting this tree's median is not above the baseline's by more than
the larger of the two spreads, the overlaps are equal and the builds / restores are equal. The per-index table is
left out of that record.

Not measured: other k / w settings, host memory pressure at large -Q, more than one device.

    python tools/bench_mapper_cache.py --baseline-lib path/to/parent/libcudamapper.so [--index-mbp 15] [--repeats 5]
                                       [--like-for-like] [--out profiles/mapper_cache.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapper_cases as MC  # noqa: E402
import oracle_mapper_batcher as B  # noqa: E402
import oracle_mapper_postprocess as P  # noqa: E402
from genomeworks_amd import _native, cudamapper  # noqa: E402

K, W, F = 15, 10, 1e-5
CACHED = (10, 5, 10, 5)
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
MAP_ARGS = [vp, vp, i32, vp, vp, i32, i32, i32, C.c_double, i64, i64, i64, f32, i64, i64, i32, i32, i32]


def load_baseline(path):
    """the baseline library beside this tree's in one process: its own symbols first (RTLD_DEEPBIND), because this
    tree's library is loaded globally and carries the same names"""
    L = C.CDLL(os.path.abspath(path), mode=os.RTLD_NOW | os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    L.gw_mapper_last_error.restype = C.c_char_p
    L.gw_mapper_map_batched.restype = vp
    L.gw_mapper_map_batched.argtypes = MAP_ARGS + [vp]
    if hasattr(L, "gw_mapper_map_batched_cached"):  # a baseline from before the index cache has neither
        L.gw_mapper_map_batched_cached.restype = vp
        L.gw_mapper_map_batched_cached.argtypes = MAP_ARGS + [i32, i64, i32, i32, i32, i32, vp]
        L.gw_mapper_overlaps_cache_counts.argtypes = [vp, vp, vp, vp]
    L.gw_mapper_overlaps_count.restype = i64
    L.gw_mapper_overlaps_count.argtypes = [vp]
    L.gw_mapper_overlaps_copy.argtypes = [vp, vp, i64, vp, vp]
    L.gw_mapper_overlaps_destroy.restype = None
    L.gw_mapper_overlaps_destroy.argtypes = [vp]
    L.gw_mapper_index_create.restype = vp
    L.gw_mapper_index_create.argtypes = [vp, vp, i32, C.c_uint32, i32, i32, i32, C.c_double, vp]
    L.gw_mapper_index_info.argtypes = [vp, vp, vp, vp]
    L.gw_mapper_index_destroy.restype = None
    L.gw_mapper_index_destroy.argtypes = [vp]
    return L


def p(a):
    return a.ctypes.data_as(vp)


class Runner:
    """one library call per run over reads that are packed once"""

    def __init__(self, hip, bases, offsets, n_reads, index_bases):
        self.hip, self.bases, self.offsets = hip, bases, offsets
        self.head = (p(bases), p(offsets), n_reads, None, None, 0, K, W, F, 3, 250, 1000, 0.8, index_bases, index_bases,
                     1, 0, 0)

    def run(self, L, counts):
        self.hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        if counts is None:
            h = L.gw_mapper_map_batched(*self.head, None)
        else:
            h = L.gw_mapper_map_batched_cached(*self.head, 0, 0, *counts, None)
        self.hip.hipDeviceSynchronize()
        wall = time.perf_counter() - t0
        if not h:
            raise RuntimeError(L.gw_mapper_last_error().decode())
        out = np.zeros(int(L.gw_mapper_overlaps_count(h)), cudamapper.OVERLAP)
        ms, pairs = np.zeros(3, np.float32), i64(0)
        L.gw_mapper_overlaps_copy(h, p(out), len(out), p(ms), C.byref(pairs))
        info = {"index_pairs": pairs.value}
        if counts is not None:
            builds, restores, cache_ms = i64(0), i64(0), np.zeros(2, np.float32)
            L.gw_mapper_overlaps_cache_counts(h, C.byref(builds), C.byref(restores), p(cache_ms))
            info.update(index_builds=builds.value, index_restores=restores.value, pack_ms=round(float(cache_ms[0]), 3),
                        unpack_ms=round(float(cache_ms[1]), 3))
        L.gw_mapper_overlaps_destroy(h)
        return wall, out, info


def expected_in_batch_order(base, indices, counts):
    """the records of the one-pair-at-a-time run, regrouped into the pair order of the batches"""
    starts = np.array([first for first, count in indices])
    qi = np.searchsorted(starts, base["query_read_id"], side="right") - 1
    ti = np.searchsorted(starts, base["target_read_id"], side="right") - 1
    order = {pair: i for i, pair in enumerate(B.walk(indices, indices, True, *counts)[0])}
    rank = np.array([order[(indices[a], indices[b])] for a, b in zip(qi, ti)])
    return base[np.argsort(rank, kind="stable")]


def per_index(baseline, reads, groups):
    rows = []
    for first, count in groups:
        part = reads[first:first + count]
        bases, offsets = cudamapper.pack_reads(part)
        h = baseline.gw_mapper_index_create(p(bases), p(offsets), len(part), first, K, W, 1, F, None)
        if not h:
            raise RuntimeError(baseline.gw_mapper_last_error().decode())
        ms = np.zeros(4, np.float32)
        baseline.gw_mapper_index_info(h, None, None, p(ms))
        baseline.gw_mapper_index_destroy(h)
        index = cudamapper.Index(part, K, W, True, F, first_read_id=first)
        copy = index.to_host()
        restored = [copy.to_device() for _ in range(3)]
        same = all(getattr(index, a).tobytes() == getattr(restored[-1], a).tobytes()
                   for a in ("representations", "read_ids", "positions_in_reads", "directions_of_reads",
                             "unique_representations", "first_occurrence_of_representations"))
        n, n_unique = len(index.representations), len(index.unique_representations)
        rows.append({"first_read": first, "reads": count, "n": n, "n_unique": n_unique,
                     "baseline_build_ms": round(float(ms.sum()), 3),
                     "this_tree_build_ms": round(sum(index.stage_ms.values()), 3), "pack_ms": round(copy.pack_ms, 3),
                     "restore_ms": round(statistics.median(r.restore_ms for r in restored), 3),
                     "packed_bytes": copy.nbytes, "plain_bytes": 17 * n + 12 * n_unique, "round_trip_equal": same})
        for r in restored:
            r.close()
        copy.close()
        index.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--index-mbp", type=float, default=15.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--genome-mbp", type=float, default=5.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--like-for-like", action="store_true",
                    help="call the baseline through gw_mapper_map_batched_cached at the same counts as this tree")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")

    tree = _native.mapper()
    baseline = load_baseline(args.baseline_lib)
    hip = C.CDLL("libamdhip64.so")
    t0 = time.perf_counter()
    reads = MC.synthetic_reads(2024, int(args.genome_mbp * 1e6), args.coverage, 10_000, 0.05)
    generation = time.perf_counter() - t0
    index_bases = int(args.index_mbp * 1e6)
    groups = P.group_reads_into_indices([len(r) for r in reads], index_bases)
    if len(groups) < 8 or any(count == 0 for first, count in groups):
        sys.exit("the index size gives %d indices; at least 8 are asked for" % len(groups))
    bases, offsets = cudamapper.pack_reads(reads)
    runner = Runner(hip, bases, offsets, len(reads), index_bases)
    runs = (("baseline", baseline, None), ("cached", tree, CACHED), ("one_pair_at_a_time", tree, (1, 1, 1, 1)))
    if args.like_for_like:
        runs = (("baseline_one_pair_at_a_time", baseline, (1, 1, 1, 1)), ("one_pair_at_a_time", tree, (1, 1, 1, 1)),
                ("baseline_cached", baseline, CACHED), ("cached", tree, CACHED))

    results, infos, walls = {}, {}, {name: [] for name, L, counts in runs}
    for name, L, counts in runs:  # warm-up: code objects, pinned and device allocations
        runner.run(L, counts)
    for _ in range(args.repeats):
        for name, L, counts in runs:
            wall, results[name], infos[name] = runner.run(L, counts)
            walls[name].append(wall)

    record = {"metric": "cudamapper batched driver, all-vs-all, wall seconds per run", "device": "gpu0", "k": K, "w": W,
              "F": F, "genome_mbp": args.genome_mbp, "coverage": args.coverage, "reads": len(reads),
              "bases": int(offsets[-1]), "index_mbp": args.index_mbp, "indices": len(groups),
              "repeats": args.repeats, "generation_s": round(generation, 1), "cached_setting": list(CACHED),
              "like_for_like": args.like_for_like}
    for name, L, counts in runs:
        w = walls[name]
        record[name] = dict(infos[name], wall_s=[round(x, 4) for x in w], median_s=round(statistics.median(w), 4),
                            spread_s=round(max(w) - min(w), 4), overlaps=len(results[name]))
    if args.like_for_like:
        return finish(record, like_for_like_checks(record, results), ["the --cigar path (covered by the tests only)"],
                      args.out)
    spread = max(record["baseline"]["spread_s"], record["cached"]["spread_s"])
    spread_ones = max(record["baseline"]["spread_s"], record["one_pair_at_a_time"]["spread_s"])
    rows = per_index(baseline, reads, groups)
    record["per_index"] = rows
    record["packed_over_plain_bytes"] = round(sum(r["packed_bytes"] for r in rows) / sum(r["plain_bytes"] for r in rows), 4)
    checks = {
        "overlaps_one_pair_at_a_time_equal_baseline": bool(np.array_equal(results["one_pair_at_a_time"], results["baseline"])),
        "overlaps_cached_equal_baseline_in_batch_order": bool(np.array_equal(
            results["cached"], expected_in_batch_order(results["one_pair_at_a_time"], groups, CACHED))),
        "cached_faster_than_baseline_beyond_spread":
            record["baseline"]["median_s"] - record["cached"]["median_s"] > spread,
        "one_pair_at_a_time_not_slower_beyond_spread":
            record["one_pair_at_a_time"]["median_s"] - record["baseline"]["median_s"] <= spread_ones,
        "every_restore_faster_than_its_build": all(r["restore_ms"] < r["baseline_build_ms"] for r in rows),
        "every_round_trip_equal": all(r["round_trip_equal"] for r in rows),
    }
    record["speedup_cached_over_baseline"] = round(record["baseline"]["median_s"] / record["cached"]["median_s"], 3)
    return finish(record, checks, [], args.out)


def like_for_like_checks(record, results):
    checks = {}
    for name in ("one_pair_at_a_time", "cached"):
        tree, base = record[name], record["baseline_" + name]
        checks[name + "_not_slower_beyond_spread"] = \
            tree["median_s"] - base["median_s"] <= max(tree["spread_s"], base["spread_s"])
        checks[name + "_overlaps_equal"] = bool(np.array_equal(results[name], results["baseline_" + name]))
        checks[name + "_builds_and_restores_equal"] = all(tree[k] == base[k] for k in ("index_builds", "index_restores"))
    return checks


def finish(record, checks, also_not_measured, out):
    record["checks"] = checks
    record["not_measured"] = ["other k / w settings", "host memory pressure at large -Q",
                              "more than one device"] + also_not_measured
    line = json.dumps(record)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    return 0 if all(checks.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
