#!/usr/bin/env python3
"""The infix / prefix alignment types of cudaaligner on three workloads, one JSON record on stdout:

  1 024 pairs of 2 kbp in 6 kbp, 64 pairs of 10 kbp in 100 kbp, 4 096 pairs of 150 bp in 1 kbp (infix; the query is a
  slice of its target with 5 % edits): HIP-event times of the ends scan (forward + anchored pass) and of the gather +
  traceback, best of `--repeats` align_all() calls after a warm-up, and the scan's rate in DP cells per second, where a
  cell is one (query base, target base) of either pass: n m + n min(te, n + d) per pair.

  The yardstick: on 1 024 pairs of 2 kbp against targets of the same length, the forward ends pass alone (a prefix
  batch) next to the kernels of the default global aligner on the same pairs in the same process
  (relaunch_timed), and their ratio.

  The single-thread numpy oracle (tests/oracle_semiglobal.py) on a few pairs of the first workload, for scale."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genomeworks_amd import cudaaligner  # noqa: E402

CACHE = 16 << 30
_BASES = np.frombuffer(b"ACGT", np.uint8)


def random_bases(rng, n):
    return _BASES[rng.integers(0, 4, n)]


def edited(rng, s, rate):
    """s with about rate * len(s) substitutions, insertions and deletions."""
    out, at = [], 0
    for p in np.sort(rng.choice(len(s), max(1, int(len(s) * rate)), replace=False)):
        out.append(s[at:p])
        kind = rng.integers(0, 3)
        if kind == 0:
            out.append(_BASES[(np.searchsorted(_BASES, s[p]) + 1 + rng.integers(0, 3)) % 4][None])
        elif kind == 1:
            out.append(np.concatenate((random_bases(rng, 1), s[p:p + 1])))
        at = p + 1
    out.append(s[at:])
    return np.concatenate(out)


def make_pairs(seed, count, n, m):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(count):
        t = random_bases(rng, m)
        at = int(rng.integers(0, m - n + 1))
        pairs.append((edited(rng, t[at:at + n], 0.05).tobytes(), t.tobytes()))
    return pairs


def run_typed(pairs, mode, repeats):
    max_q = max(len(q) for q, _ in pairs)
    max_t = max(len(t) for _, t in pairs)
    al = cudaaligner.CudaAlignerBatch(max_q, max_t, len(pairs), alignment_type=mode, max_device_memory_allocator_caching_size=CACHE)
    best = None
    for k in range(repeats + 1):            # the first call is the warm-up
        for q, t in pairs:
            assert al.add_alignment(q, t) == 0
        al.align_all()
        assert al.sync() == len(pairs)
        stage = al.stage_ms()
        if k > 0:
            best = stage if best is None else (min(best[0], stage[0]), min(best[1], stage[1]))
        if k < repeats:
            al.reset()
    results = al.get_alignments()
    return best, results


def workload(name, seed, count, n, m, repeats):
    pairs = make_pairs(seed, count, n, m)
    (ends_ms, traceback_ms), results = run_typed(pairs, "infix", repeats)
    cells = 0
    for (q, t), r in zip(pairs, results):
        assert r.status == 0
        cells += len(q) * len(t)
        if r.edit_distance < len(q):
            cells += len(q) * min(r.target_end, len(q) + r.edit_distance)
    return {"workload": name, "pairs": count, "query": n, "target": m, "ends_ms": round(ends_ms, 3),
            "traceback_ms": round(traceback_ms, 3), "ends_cells": cells, "ends_gcells_per_s": round(cells / ends_ms / 1e6, 2),
            "mean_edit_distance": round(sum(r.edit_distance for r in results) / count, 1)}, pairs


def yardstick(seed, count, n, repeats):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(count):                          # m == n exactly: both cut from sequences a tenth longer
        t = random_bases(rng, n + n // 10)
        pairs.append((edited(rng, t, 0.05)[:n].tobytes(), t[:n].tobytes()))
    assert all(len(q) == n and len(t) == n for q, t in pairs)
    (forward_ms, _), _ = run_typed(pairs, "prefix", repeats)
    al = cudaaligner.CudaAlignerBatch(n, n, count, max_device_memory_allocator_caching_size=CACHE)
    for q, t in pairs:
        assert al.add_alignment(q, t) == 0
    al.align_all()
    assert al.sync() == count
    global_ms = min(al.relaunch_timed() for _ in range(repeats + 1))
    return {"pairs": count, "length": n, "forward_ends_ms": round(forward_ms, 3), "default_global_aligner_kernels_ms": round(global_ms, 3),
            "ratio_ends_over_global": round(forward_ms / global_ms, 3)}


def oracle_time(pairs, count):
    import oracle_semiglobal as S
    t0 = time.perf_counter()
    cells = 0
    for q, t in pairs[:count]:
        d, te, tb = S.semiglobal(q.decode(), t.decode(), "infix")
        cells += len(q) * len(t) + len(q) * te
    dt = time.perf_counter() - t0
    return {"pairs": count, "seconds": round(dt, 3), "gcells_per_s": round(cells / dt / 1e9, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the pairs (a rehearsal, not a measurement)")
    args = ap.parse_args()
    scale = 10 if args.quick else 1
    record = {"tool": "bench_semiglobal", "quick": args.quick, "workloads": []}
    first_pairs = None
    for name, seed, count, n, m in (("2kbp_in_6kbp", 1, 1024, 2000, 6000), ("10kbp_in_100kbp", 2, 64, 10000, 100000),
                                    ("150bp_in_1kbp", 3, 4096, 150, 1000)):
        row, pairs = workload(name, seed, max(4, count // scale), n, m, args.repeats)
        first_pairs = first_pairs or pairs
        record["workloads"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    record["yardstick_m_equals_n"] = yardstick(4, max(4, 1024 // scale), 2048, args.repeats)
    record["numpy_oracle"] = oracle_time(first_pairs, 4)
    print(json.dumps(record))
