"""Overlap alignment of cudamapper on one GPU: the on-device path against the host path, on the same records in the
same process. Prints one JSON record.

Workload: the synthetic set of tools/bench_mapper.py (a seeded 5 Mbp genome at 30x coverage of ~10 kbp reads with 5 %
errors, both strands, k=15 w=10 F=1e-5, r=3 l=250 b=1000 z=0.8), mapped all-to-all once by the batched driver with
fusion and end rescue: its final overlaps are the records (--max-overlaps N keeps N of them, evenly spaced, when the
whole set does not fit the time at hand; the record says so). Then, after a warm-up of each and alternating,
--repeats times:

  device   gw_mapper_align_overlaps: reads and overlap records uploaded, gather -> default aligner -> CIGAR text on
           the device, text + offsets + edit distances copied back;
  host 1   gw_align_overlaps, i.e. cudamapper::align_overlaps() of overlap_alignment.hpp as the align_overlaps tool runs
  host 4   it, with one and with four alignment engines: slices cut and reverse-complemented on the host and
           uploaded, one state byte per column copied back, Alignment::convert_to_cigar() per alignment. The batch
           size is the reference's heuristic over the tool's default 2 GiB pool (a few hundred alignments);
  host 1 / --host-pool-gib   the same with one engine and the pool the tool's -m would give (default 64 GiB), i.e.
           batches of thousands of alignments: the host path without the small-batch handicap.

Both are timed from packed reads and records in host memory to CIGAR text and offsets in host memory. The yardstick of
the device path is the host path of the same run; the spread is that of the repeats. Bytes moved are counted from the
shapes, not measured.

    python tools/bench_mapper_align.py [--index-mbp 30] [--repeats 3] [--max-overlaps 0] [--host-pool-gib 64]
                                        [--out profiles/mapper_align.json]
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
from genomeworks_amd import _native, cudamapper  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_path(o, bases, offsets, n_reads):
    """-> (text, offsets, stage_ms) through the C API, reads given once: all against all"""
    L = _native.mapper()
    h = L.gw_mapper_align_overlaps(_p(o), len(o), _p(bases), _p(offsets), n_reads, 0, None, None, 0, 0, 0, None)
    if not h:
        raise cudamapper.MapperError(L.gw_mapper_last_error().decode())
    try:
        text = np.zeros(int(L.gw_mapper_cigars_text_bytes(h)), np.uint8)
        offs, edits, ms = np.zeros(len(o) + 1, np.int64), np.zeros(len(o), np.int32), np.zeros(3, np.float32)
        if L.gw_mapper_cigars_copy(h, _p(text), _p(offs), _p(edits), _p(ms)) != 0:
            raise cudamapper.MapperError(L.gw_mapper_last_error().decode())
    finally:
        L.gw_mapper_cigars_destroy(h)
    return text, offs, ms


def host_path(o, bases, offsets, n_reads, engines, pool_gib=0):
    L = _native.host()
    L.gw_align_overlaps.restype = C.c_void_p
    L.gw_align_overlaps.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    L.gw_overlap_cigars_text_bytes.restype = C.c_int64
    L.gw_overlap_cigars_text_bytes.argtypes = [C.c_void_p]
    L.gw_overlap_cigars_copy.restype = None
    L.gw_overlap_cigars_copy.argtypes = [C.c_void_p] * 3
    L.gw_overlap_cigars_destroy.restype = None
    L.gw_overlap_cigars_destroy.argtypes = [C.c_void_p]
    h = L.gw_align_overlaps(_p(o), len(o), _p(bases), _p(offsets), n_reads, None, None, 0, engines, 0, pool_gib << 30)
    if not h:
        raise RuntimeError(L.gw_last_error().decode())
    try:
        text, offs = np.zeros(int(L.gw_overlap_cigars_text_bytes(h)), np.uint8), np.zeros(len(o) + 1, np.int64)
        L.gw_overlap_cigars_copy(h, _p(text), _p(offs))
    finally:
        L.gw_overlap_cigars_destroy(h)
    return text, offs


def spread(seconds):
    return dict(median_s=round(statistics.median(seconds), 4), min_s=round(min(seconds), 4),
                max_s=round(max(seconds), 4), runs_s=[round(s, 4) for s in seconds])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mbp", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-overlaps", type=int, default=0)
    ap.add_argument("--host-pool-gib", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    k, w, F = 15, 10, 1e-5
    genome_mbp, coverage = 5.0, 30.0
    reads = MC.synthetic_reads(2024, int(genome_mbp * 1e6), coverage, 10_000, 0.05)
    t0 = time.perf_counter()
    final = cudamapper.map_reads_batched(reads, k=k, w=w, filtering_parameter=F,
                                         max_basepairs_per_index=int(args.index_mbp * 1e6), rescue_overlap_ends=True)
    map_s = time.perf_counter() - t0
    o = final
    if 0 < args.max_overlaps < len(final):
        o = np.ascontiguousarray(final[np.linspace(0, len(final) - 1, args.max_overlaps).astype(np.int64)])
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    print(len(reads), "reads,", len(final), "final overlaps,", len(o), "aligned", file=sys.stderr, flush=True)
    bases, offsets = cudamapper.pack_reads(reads)

    paths = [("device", lambda x: device_path(x, bases, offsets, len(reads))[:2]),
             ("host_1_engine", lambda x: host_path(x, bases, offsets, len(reads), 1)),
             ("host_4_engines", lambda x: host_path(x, bases, offsets, len(reads), 4)),
             ("host_1_engine_large_pool", lambda x: host_path(x, bases, offsets, len(reads), 1, args.host_pool_gib))]
    warm = np.ascontiguousarray(o[:256])
    for _, run in paths:  # code objects, allocators
        run(warm)
    seconds = {name: [] for name, _ in paths}
    stage_ms, results = [], {}
    for _ in range(args.repeats):
        for name, run in paths:
            t0 = time.perf_counter()
            if name == "device":
                text, offs, ms = device_path(o, bases, offsets, len(reads))
                stage_ms.append([float(x) for x in ms])
            else:
                text, offs = run(o)
            seconds[name].append(time.perf_counter() - t0)
            results[name] = (text, offs)
            print(name, round(seconds[name][-1], 3), "s", file=sys.stderr, flush=True)
    same = all(np.array_equal(results["device"][0], results[n][0]) and np.array_equal(results["device"][1], results[n][1])
               for n in seconds if n != "device")
    n, aligned_bases, text_bytes = len(o), int(ql.sum() + tl.sum()), int(len(results["device"][0]))
    med = {name: statistics.median(v) for name, v in seconds.items()}
    best_host = min(v for name, v in med.items() if name != "device")
    rec = {"metric": "cudamapper overlap alignment to CIGAR text, device path vs host path", "device": "gpu0",
           "k": k, "w": w, "F": F, "genome_mbp": genome_mbp, "coverage": coverage, "reads": len(reads),
           "read_bases": int(offsets[-1]), "final_overlaps": len(final), "overlaps_aligned": n,
           "subsampled": n != len(final), "mapping_wall_s": round(map_s, 3),
           "bases_aligned": aligned_bases, "longest_query_slice": int(ql.max()), "longest_target_slice": int(tl.max()),
           "cigar_text_bytes": text_bytes, "repeats": args.repeats, "host_pool_gib": {"default": 2, "large": args.host_pool_gib}, "device_equals_host": bool(same),
           "wall": {name: spread(v) for name, v in seconds.items()},
           "overlaps_per_s": {name: round(n / med[name], 1) for name in med},
           "device_stage_ms": dict(zip(("gather", "align", "cigar_text"),
                                       (round(statistics.median(c), 3) for c in zip(*stage_ms)))),
           "device_speedup_over_best_host": round(best_host / med["device"], 3),
           "bytes_from_shapes": {
               "device": {"h2d": int(offsets[-1]) + offsets.nbytes + n * 36,
                          "d2h": n * 36 + text_bytes + 8 * (n + 1) + 4 * n},
               "host": {"h2d": aligned_bases + 8 * (2 * n + 1), "d2h": aligned_bases + 4 * n}}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
