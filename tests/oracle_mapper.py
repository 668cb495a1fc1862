"""ctypes view of the cudamapper oracle (tests/oracle_mapper.c), compiled with gcc into tests/build/ on first use --
TEST INFRASTRUCTURE ONLY. Results use the dtypes of genomeworks_amd.cudamapper (ANCHOR, OVERLAP), so the GPU path and
the oracle compare with a plain array equality."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_mapper.c")
BUILD = os.path.join(HERE, "build")
CFLAGS = ["-O2", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]

# same layouts as genomeworks_amd.cudamapper (kept here so the CPU tests need no native library)
ANCHOR = np.dtype([("query_read_id", "<u4"), ("target_read_id", "<u4"),
                   ("query_position_in_read", "<u4"), ("target_position_in_read", "<u4")])
OVERLAP = np.dtype({"names": ["query_read_id", "target_read_id", "query_start_position_in_read",
                              "target_start_position_in_read", "query_end_position_in_read",
                              "target_end_position_in_read", "relative_strand", "num_residues", "overlap_complete"],
                    "formats": ["<u4"] * 6 + ["u1", "<u4", "u1"],
                    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32], "itemsize": 36})

_L = None
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


def lib():
    global _L
    if _L is None:
        with open(SRC, "rb") as f:
            tag = hashlib.sha256(f.read() + repr(CFLAGS).encode()).hexdigest()[:12]
        path = os.path.join(BUILD, "liboracle_mapper_%s.so" % tag)
        if not os.path.exists(path):
            os.makedirs(BUILD, exist_ok=True)
            fd, tmp = tempfile.mkstemp(suffix=".so", dir=BUILD)
            os.close(fd)
            subprocess.run(["gcc"] + CFLAGS + ["-shared", "-o", tmp, SRC], check=True)
            os.replace(tmp, path)
        L = C.CDLL(path)
        L.om_sketch.restype = i64
        L.om_sketch.argtypes = [vp, vp, i32, C.c_uint32, i32, i32, i32, i32, vp, vp, vp, vp]
        L.om_index.restype = None
        L.om_index.argtypes = [i64, vp, vp, vp, vp, C.c_double, vp, vp, C.POINTER(i64), C.POINTER(i64)]
        L.om_count_anchors.restype = i64
        L.om_count_anchors.argtypes = [vp, vp, i64, vp, vp, i64]
        L.om_anchors.restype = i64
        L.om_anchors.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp]
        L.om_overlaps.restype = i64
        L.om_overlaps.argtypes = [vp, i64, i32, i64, i64, i64, C.c_float, vp]
        _L = L
    return _L


def _p(a):
    return a.ctypes.data_as(vp)


def pack_reads(reads):
    """list of str / bytes -> (bases uint8, offsets int64[n+1])"""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(bs) + 1, np.int64)
    offsets[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs) or b"\0", np.uint8).copy(), offsets


TRUE_DIRECTIONS, REFERENCE_DIRECTIONS, ALIASED_DIRECTIONS = 0, 1, 2


def sketch(reads, k, w, hash_representations=True, first_read_id=0, direction_mode=TRUE_DIRECTIONS):
    """Minimizers in read / position order: dict of representations, read_ids, positions_in_reads, directions.
    direction_mode: TRUE_DIRECTIONS (0 forward, 1 reverse: what the GPU path gives), REFERENCE_DIRECTIONS (the bytes
    the reference gives: a byte of a window position where its direction array is overrun, oracle_mapper.c), or
    ALIASED_DIRECTIONS (1 for exactly those elements)."""
    bases, offsets = pack_reads(reads)
    cap = int(sum(max(0, int(offsets[i + 1] - offsets[i]) - k + w) for i in range(len(reads)))) + 1
    rep, rid, pos, d = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    n = lib().om_sketch(_p(bases), _p(offsets), len(reads), first_read_id, k, w, int(bool(hash_representations)),
                        direction_mode, _p(rep), _p(rid), _p(pos), _p(d))
    return dict(representations=rep[:n], read_ids=rid[:n], positions_in_reads=pos[:n], directions=d[:n])


def index(reads, k, w, hash_representations=True, filtering_parameter=1.0, first_read_id=0,
          direction_mode=TRUE_DIRECTIONS):
    """The index arrays of the reads, with the reference's names, plus number_of_reads / smallest_read_id /
    largest_read_id / number_of_basepairs_in_longest_read."""
    s = sketch(reads, k, w, hash_representations, first_read_id, direction_mode)
    n = len(s["representations"])
    rep, rid = s["representations"].copy(), s["read_ids"].copy()
    pos, d = s["positions_in_reads"].copy(), s["directions"].copy()
    uq, fo = np.zeros(n + 1, np.uint64), np.zeros(n + 2, np.uint32)
    n_out, nu = i64(0), i64(0)
    lib().om_index(n, _p(rep), _p(rid), _p(pos), _p(d), float(filtering_parameter), _p(uq), _p(fo), C.byref(n_out),
                   C.byref(nu))
    lens = [len(r) for r in reads if len(r) >= k + w - 1]
    nreads = len(reads) if lens else 0
    m, u = n_out.value, nu.value
    return dict(representations=rep[:m], read_ids=rid[:m], positions_in_reads=pos[:m], directions=d[:m],
                unique_representations=uq[:u], first_occurrence_of_representations=fo[:u + 1] if n else fo[:0],
                number_of_reads=nreads, smallest_read_id=first_read_id if nreads else 0,
                largest_read_id=first_read_id + nreads - 1 if nreads else 0,
                number_of_basepairs_in_longest_read=max(lens) if lens else 0)


def anchors(q, t):
    """All anchors of two oracle indices, sorted by (query read, target read, query position, target position)."""
    if len(q["unique_representations"]) == 0 or len(t["unique_representations"]) == 0:
        return np.zeros(0, ANCHOR)
    args = (_p(q["unique_representations"]), _p(q["first_occurrence_of_representations"]), len(q["unique_representations"]),
            _p(t["unique_representations"]), _p(t["first_occurrence_of_representations"]), len(t["unique_representations"]))
    n = lib().om_count_anchors(*args)
    out = np.zeros(max(n, 1), ANCHOR)
    m = lib().om_anchors(args[0], args[1], args[2], _p(q["read_ids"]), _p(q["positions_in_reads"]),
                         args[3], args[4], args[5], _p(t["read_ids"]), _p(t["positions_in_reads"]), _p(out))
    assert m == n
    return out[:n]


def overlaps(anchor_array, all_to_all=True, min_residues=3, min_overlap_len=250, min_bases_per_residue=1000,
             min_overlap_fraction=0.8):
    a = np.ascontiguousarray(anchor_array, ANCHOR)
    out = np.zeros(max(len(a), 1), OVERLAP)
    n = lib().om_overlaps(_p(a), len(a), int(bool(all_to_all)), min_residues, min_overlap_len, min_bases_per_residue,
                          min_overlap_fraction, _p(out))
    return out[:n]


def map_reads(queries, targets=None, k=15, w=10, filtering_parameter=1e-5, min_residues=3, min_overlap_len=250,
              min_bases_per_residue=1000, min_overlap_fraction=0.8, hash_representations=True):
    q = index(queries, k, w, hash_representations, filtering_parameter)
    t = q if targets is None else index(targets, k, w, hash_representations, filtering_parameter)
    return overlaps(anchors(q, t), targets is None, min_residues, min_overlap_len, min_bases_per_residue,
                    min_overlap_fraction)
