"""ctypes view of the cudaextender oracle (tests/oracle_extender.c), compiled with gcc into tests/build/ on first use --
TEST INFRASTRUCTURE ONLY. Segments come back as the structured dtype SEGMENT (memory order of ScoredSegmentPair)."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_extender.c")
BUILD = os.path.join(HERE, "build")
CFLAGS = ["-O2", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]

SEGMENT = np.dtype([("query", "<u4"), ("target", "<u4"), ("length", "<i4"), ("score", "<i4")])

# encoding of cudaextender/utils.hpp: A C G T, lower-case acgt (L), N/n, anything else (X), '&' (E)
_CODE = np.full(256, 6, np.int8)
for _s, _v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("a", 4), ("c", 4), ("g", 4), ("t", 4), ("N", 5), ("n", 5), ("&", 7)):
    _CODE[ord(_s)] = _v

_L = None


def encode(seq):
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    return _CODE[np.frombuffer(b, np.uint8)]


def lib():
    global _L
    if _L is None:
        with open(SRC, "rb") as f:
            tag = hashlib.sha256(f.read() + repr(CFLAGS).encode()).hexdigest()[:12]
        path = os.path.join(BUILD, "liboracle_extender_%s.so" % tag)
        if not os.path.exists(path):
            os.makedirs(BUILD, exist_ok=True)
            fd, tmp = tempfile.mkstemp(suffix=".so", dir=BUILD)
            os.close(fd)
            subprocess.run(["gcc"] + CFLAGS + ["-shared", "-o", tmp, SRC, "-lm"], check=True)
            os.replace(tmp, path)  # atomic: concurrent first uses never load a half-written library
        _L = C.CDLL(path)
        _L.gwx_oracle_extend.restype = C.c_int64
        _L.gwx_oracle_extend.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        _L.gwx_oracle_sort_unique.restype = C.c_int64
        _L.gwx_oracle_sort_unique.argtypes = [C.c_void_p, C.c_int64]
    return _L


def extend(target, query, score_matrix, xdrop, thr, no_entropy, seeds, chunk=0):
    """target/query: encoded int8 arrays (or str); seeds: [N, 2] (target, query) positions. Returns SEGMENT rows."""
    T = np.ascontiguousarray(encode(target) if isinstance(target, (str, bytes)) else target, np.int8)
    Q = np.ascontiguousarray(encode(query) if isinstance(query, (str, bytes)) else query, np.int8)
    M = np.ascontiguousarray(score_matrix, np.int32).reshape(-1)
    assert M.size == 64
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    st = np.ascontiguousarray(seeds[:, 0], np.uint32)
    sq = np.ascontiguousarray(seeds[:, 1], np.uint32)
    out = np.zeros(max(len(seeds), 1), SEGMENT)
    n = lib().gwx_oracle_extend(T.ctypes.data, T.size, Q.ctypes.data, Q.size, M.ctypes.data, int(xdrop), int(thr),
                                int(bool(no_entropy)), st.ctypes.data, sq.ctypes.data, len(seeds), int(chunk),
                                out.ctypes.data)
    return out[:n].copy()


def sort_unique(segments):
    """The sort + adjacent de-duplication step alone, on a SEGMENT array (input order = compaction order)."""
    s = np.ascontiguousarray(segments, SEGMENT).copy()
    n = lib().gwx_oracle_sort_unique(s.ctypes.data, s.size)
    return s[:n]


def rows(segments):
    """(target, query, length, score) tuples: the column order of the reference's CSV files."""
    return [(int(s["target"]), int(s["query"]), int(s["length"]), int(s["score"])) for s in segments]
