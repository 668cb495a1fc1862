"""Python interface of cudamapper: minimizer index, anchor matcher and overlapper on the GPU (libcudamapper.so, HIP for
gfx950), over the flat C API of include/gw_mapper_capi.h.

    index = Index(reads, k=15, w=10, filtering_parameter=1e-5)     # reads: list of str / bytes
    matcher = Matcher(index, index)                                # anchors stay on the device
    overlaps = find_overlaps(matcher, all_to_all=True)             # numpy structured array of OVERLAP records
    overlaps = map_reads(reads)                                    # the same in one call

Index arrays carry the reference's names (representations, read_ids, positions_in_reads, directions_of_reads,
unique_representations, first_occurrence_of_representations) and come back as numpy arrays."""
import ctypes as C

import numpy as np

from . import _native

ANCHOR = np.dtype([("query_read_id", "<u4"), ("target_read_id", "<u4"),
                   ("query_position_in_read", "<u4"), ("target_position_in_read", "<u4")])
# cudamapper::Overlap: six uint32, relative_strand (b'+' / b'-'), num_residues_, overlap_complete; 36 B with padding
OVERLAP = np.dtype({"names": ["query_read_id", "target_read_id", "query_start_position_in_read",
                              "target_start_position_in_read", "query_end_position_in_read",
                              "target_end_position_in_read", "relative_strand", "num_residues", "overlap_complete"],
                    "formats": ["<u4"] * 6 + ["u1", "<u4", "u1"],
                    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32], "itemsize": 36})

FORWARD, REVERSE = 0, 1  # SketchElement::DirectionOfRepresentation


class MapperError(RuntimeError):
    pass


def maximum_kmer_size():
    """Index::maximum_kmer_size(): sizeof(representation_t) * CHAR_BIT / 2"""
    return 32


def _err(L):
    return MapperError(L.gw_mapper_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _stream(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream or None
    for attr in ("cuda_stream", "stream"):
        if hasattr(stream, attr):
            v = getattr(stream, attr)
            return v() if callable(v) else v
    raise TypeError("stream must be None, an integer handle, a torch.cuda.Stream or a CudaStream")


def pack_reads(reads):
    """list of str / bytes -> (bases uint8, offsets int64[n + 1]) as the C API takes them"""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(bs) + 1, np.int64)
    offsets[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs) or b"\0", np.uint8).copy(), offsets


class Index:
    """Index::create_index_async + wait_to_be_ready over `reads`, whose ids are first_read_id, first_read_id + 1, ...
    (reads shorter than k + w - 1 are skipped and, as in the reference, the reads after them take their ids)."""

    def __init__(self, reads, k=15, w=10, hash_representations=True, filtering_parameter=1.0, first_read_id=0,
                 stream=None):
        if not 1 <= k <= maximum_kmer_size():
            raise ValueError("k must be in 1..%d" % maximum_kmer_size())
        if w < 1:
            raise ValueError("w must be >= 1")
        self._L = _native.mapper()
        bases, offsets = pack_reads(reads)
        self.kmer_size, self.window_size = k, w
        self._h = self._L.gw_mapper_index_create(_p(bases), _p(offsets), len(reads), first_read_id, k, w,
                                                 int(bool(hash_representations)), float(filtering_parameter),
                                                 _stream(stream))
        self._fill()

    @classmethod
    def from_arrays(cls, read_ids, positions_in_reads, unique_representations, first_occurrence_of_representations,
                    first_read_id, number_of_reads, number_of_basepairs_in_longest_read):
        """An index given by its arrays (the matcher on hand-built indices): elements grouped by representation,
        unique_representations ascending, first_occurrence_of_representations with the trailing total."""
        self = cls.__new__(cls)
        self._L = _native.mapper()
        self.kmer_size = self.window_size = None
        rid = np.ascontiguousarray(read_ids, np.uint32)
        pos = np.ascontiguousarray(positions_in_reads, np.uint32)
        uq = np.ascontiguousarray(unique_representations, np.uint64)
        fo = np.ascontiguousarray(first_occurrence_of_representations, np.uint32)
        if len(rid) != len(pos) or (len(uq) and len(fo) != len(uq) + 1):
            raise ValueError("read_ids / positions_in_reads or unique / first_occurrence sizes disagree")
        self._h = self._L.gw_mapper_index_from_arrays(len(rid), _p(rid), _p(pos), len(uq), _p(uq), _p(fo),
                                                      first_read_id, number_of_reads,
                                                      number_of_basepairs_in_longest_read)
        self._fill()
        return self

    def _fill(self):
        if not self._h:
            raise _err(self._L)
        sizes, info, ms = np.zeros(3, np.int64), np.zeros(4, np.uint32), np.zeros(4, np.float32)
        self._L.gw_mapper_index_info(self._h, _p(sizes), _p(info), _p(ms))
        n, nu, nf = (int(x) for x in sizes)
        (self.number_of_reads, self.smallest_read_id, self.largest_read_id,
         self.number_of_basepairs_in_longest_read) = (int(x) for x in info)
        self.stage_ms = dict(zip(("sketch", "sort", "unique", "filter"), (float(x) for x in ms)))
        self.representations = np.zeros(n, np.uint64)
        self.read_ids = np.zeros(n, np.uint32)
        self.positions_in_reads = np.zeros(n, np.uint32)
        self.directions_of_reads = np.zeros(n, np.uint8)
        self.unique_representations = np.zeros(nu, np.uint64)
        self.first_occurrence_of_representations = np.zeros(nf, np.uint32)
        if self._L.gw_mapper_index_copy(self._h, _p(self.representations), _p(self.read_ids),
                                        _p(self.positions_in_reads), _p(self.directions_of_reads),
                                        _p(self.unique_representations),
                                        _p(self.first_occurrence_of_representations)) != 0:
            raise _err(self._L)

    def close(self):
        if getattr(self, "_h", None):
            self._L.gw_mapper_index_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Matcher:
    """Matcher::create_matcher(query_index, target_index): anchors sorted by (query read, target read, query position,
    target position), kept on the device for find_overlaps; anchors() copies them out. stage_ms holds the device time
    of the match and anchor-sort stages, and of chain/fuse/filter once find_overlaps ran on it."""

    def __init__(self, query_index, target_index, stream=None):
        self._L = _native.mapper()
        self._query, self._target = query_index, target_index  # keep the indices alive as long as the anchors
        self._stream = _stream(stream)
        self._h = self._L.gw_mapper_matcher_create(query_index._h, target_index._h, self._stream)
        if not self._h:
            raise _err(self._L)
        self.n_anchors = int(self._L.gw_mapper_matcher_anchor_count(self._h))
        self._anchors = None
        ms = np.zeros(2, np.float32)
        if self._L.gw_mapper_matcher_copy_anchors(self._h, None, 0, _p(ms)) != 0:
            raise _err(self._L)
        self.stage_ms = {"match": float(ms[0]), "anchor_sort": float(ms[1])}

    def anchors(self):
        if self._anchors is None:
            out = np.zeros(self.n_anchors, ANCHOR)
            if self._L.gw_mapper_matcher_copy_anchors(self._h, _p(out), self.n_anchors, None) != 0:
                raise _err(self._L)
            self._anchors = out
        return self._anchors

    def close(self):
        if getattr(self, "_h", None):
            self._L.gw_mapper_matcher_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def find_anchors(query_index, target_index, stream=None):
    """All anchors between two indices, as an ANCHOR array."""
    m = Matcher(query_index, target_index, stream)
    try:
        return m.anchors()
    finally:
        m.close()


def find_overlaps(anchors, all_to_all=True, min_residues=3, min_overlap_len=250, min_bases_per_residue=1000,
                  min_overlap_fraction=0.8, stream=None):
    """Overlapper::get_overlaps on a Matcher (device anchors) or on a sorted ANCHOR array (uploaded first).
    Returns an OVERLAP array; a Matcher also records the chain/fuse/filter device time in matcher.stage_ms."""
    L = _native.mapper()
    args = (int(bool(all_to_all)), int(min_residues), int(min_overlap_len), int(min_bases_per_residue),
            float(min_overlap_fraction))
    if isinstance(anchors, Matcher):
        out = np.empty(anchors.n_anchors // 3 + 1, OVERLAP)  # a kept chain holds >= 3 anchors
        ms = C.c_float(0.0)
        n = L.gw_mapper_get_overlaps(anchors._h, *args, _p(out), C.byref(ms), _stream(stream) or anchors._stream)
        anchors.stage_ms["chain_fuse_filter"] = ms.value
    else:
        a = np.ascontiguousarray(anchors, ANCHOR)
        out = np.empty(len(a) // 3 + 1, OVERLAP)
        n = L.gw_mapper_get_overlaps_host(_p(a), len(a), *args, _p(out), _stream(stream))
    if n < 0:
        raise _err(L)
    return out[:n]


def map_reads(queries, targets=None, k=15, w=10, filtering_parameter=1e-5, min_residues=3, min_overlap_len=250,
              min_bases_per_residue=1000, min_overlap_fraction=0.8, stream=None):
    """Overlaps of `queries` against `targets`, or all against all (self-mappings dropped) when targets is None, with
    hashed representations as in the reference's cudamapper. One index per read set: batching into several indices
    (the CLI's -i / -t) is the caller's."""
    q = Index(queries, k, w, True, filtering_parameter, stream=stream)
    t = q if targets is None else Index(targets, k, w, True, filtering_parameter, stream=stream)
    m = Matcher(q, t, stream)
    try:
        return find_overlaps(m, targets is None, min_residues, min_overlap_len, min_bases_per_residue,
                             min_overlap_fraction, stream)
    finally:
        m.close()
        q.close()
        t.close()
