"""Throughput of cudaextender (libcudaextender.so) on one GPU. Prints one JSON record.

Workloads:
  sample     the reference's end-to-end sample (tests/golden/cudaextender_sample.npz: 250 kbp against itself, 143 670
             seeds), checked against its 1 337 expected rows;
  synthetic  a seeded target / query pair of --mbp Mbp each: random sequence with planted homologous blocks (the query
             carries mutated copies of target blocks at other offsets), seeded the way a k-mer seeder would (every
             --stride columns along each planted block's diagonal, with jitter) plus random off-diagonal seeds.

Per workload: device time of each extend call from HIP events, split into the extension kernel and compaction + sort +
de-duplication; seeds/s and columns examined/s; and a single-thread CPU baseline with the C oracle on a subsample.

    python tools/bench_extender.py [--mbp 64] [--seeds 30000000] [--repeats 3] [--out record.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extender_cases as K  # noqa: E402
import oracle_extender as X  # noqa: E402
from genomeworks_amd import cudaextender  # noqa: E402


def synthetic(mbp, n_seeds, seed=12345, stride=24):
    rng = np.random.default_rng(seed)
    n = int(mbp * 1_000_000)
    T = rng.integers(0, 4, n, dtype=np.int8)
    Q = rng.integers(0, 4, n, dtype=np.int8)
    # planted blocks: 2-20 kbp copies of target blocks at random query offsets, 1-15 % substitutions
    blocks, covered = [], 0
    while covered < n // 3:
        L = int(rng.integers(2000, 20000))
        t0, q0 = int(rng.integers(0, n - L)), int(rng.integers(0, n - L))
        copy = T[t0:t0 + L].copy()
        hit = rng.random(L) < rng.uniform(0.01, 0.15)
        copy[hit] = rng.integers(0, 4, int(hit.sum()))
        Q[q0:q0 + L] = copy
        blocks.append((t0, q0, L))
        covered += L
    # seeds: along each block's diagonal every `stride` columns (jittered), then random seeds to fill up
    st, sq = [], []
    for t0, q0, L in blocks:
        off = np.arange(0, L, stride) + rng.integers(0, stride // 2, (L + stride - 1) // stride)
        off = off[off < L]
        st.append(t0 + off)
        sq.append(q0 + off)
    st, sq = np.concatenate(st), np.concatenate(sq)
    if st.size < n_seeds:
        k = n_seeds - st.size
        st = np.concatenate([st, rng.integers(0, n, k)])
        sq = np.concatenate([sq, rng.integers(0, n, k)])
    seeds = np.stack([st, sq], 1)[:n_seeds]
    seeds = seeds[np.argsort(seeds[:, 0], kind="stable")]  # seeder output is ordered by target position
    return T, Q, seeds, len(blocks)


def run(ext, query, target, thr, seeds, repeats):
    ext.set_instrumentation(True)
    times = []
    for _ in range(repeats + 1):  # the first call warms up (code objects, allocator pool)
        t = time.perf_counter()
        out = ext.extend(query, target, thr, seeds)
        wall = time.perf_counter() - t
        k, p, cols = ext.last_timing()
        times.append((wall * 1e3, k, p, cols))
    times = times[1:]
    wall, k, p = (float(np.median([x[i] for x in times])) for i in range(3))
    cols = times[-1][3]
    n = len(seeds)
    return out, dict(seeds=n, segments=int(len(out)), wall_ms=round(wall, 3), kernel_ms=round(k, 3),
                     sort_unique_ms=round(p, 3), device_ms=round(k + p, 3), columns=int(cols),
                     seeds_per_s_device=round(n / ((k + p) * 1e-3)), seeds_per_s_kernel=round(n / (k * 1e-3)),
                     columns_per_s_kernel=round(cols / (k * 1e-3)), repeats=repeats)


def cpu_baseline(T, Q, M, xdrop, thr, no_entropy, seeds, max_seeds):
    sub = seeds[:max_seeds]
    t = time.perf_counter()
    X.extend(T, Q, M, xdrop, thr, no_entropy, sub)
    dt = time.perf_counter() - t
    return dict(seeds=int(len(sub)), seconds=round(dt, 4), seeds_per_s=round(len(sub) / dt))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mbp", type=float, default=64)
    ap.add_argument("--seeds", type=int, default=30_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-seeds", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = dict(tool="bench_extender", device=None)
    try:
        import torch
        rec["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass

    s = K.load_sample()
    seq, M = s["sequence"], s["score_matrix"]
    ext = cudaextender.UngappedXDropExtender(M, s["xdrop"], s["no_entropy"], max_device_memory=4 << 30)
    out, r = run(ext, seq, seq, s["score_threshold"], s["seeds"], a.repeats)
    r["matches_golden"] = X.rows(out) == s["expected"]
    r["cpu_oracle_1thread"] = cpu_baseline(seq, seq, M, s["xdrop"], s["score_threshold"], s["no_entropy"], s["seeds"],
                                           len(s["seeds"]))
    rec["sample"] = r
    del ext

    t0 = time.perf_counter()
    T, Q, seeds, nblocks = synthetic(a.mbp, a.seeds)
    gen_s = time.perf_counter() - t0
    ext = cudaextender.UngappedXDropExtender(M, s["xdrop"], s["no_entropy"], max_device_memory=24 << 30)
    out, r = run(ext, Q, T, s["score_threshold"], seeds, a.repeats)
    r.update(mbp=a.mbp, planted_blocks=nblocks, generate_s=round(gen_s, 2))
    # correctness spot check: the first --cpu-seeds seeds on their own, GPU against the oracle
    sub = seeds[: a.cpu_seeds]
    r["subsample_matches_oracle"] = X.rows(ext.extend(Q, T, s["score_threshold"], sub)) == X.rows(
        X.extend(T, Q, M, s["xdrop"], s["score_threshold"], s["no_entropy"], sub))
    r["cpu_oracle_1thread"] = cpu_baseline(T, Q, M, s["xdrop"], s["score_threshold"], s["no_entropy"], seeds, a.cpu_seeds)
    rec["synthetic"] = r
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
