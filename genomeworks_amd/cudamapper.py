"""Python interface of cudamapper: minimizer index, anchor matcher and overlapper on the GPU (libcudamapper.so, HIP for
gfx950), over the flat C API of include/gw_mapper_capi.h.

    index = Index(reads, k=15, w=10, filtering_parameter=1e-5)     # reads: list of str / bytes
    matcher = Matcher(index, index)                                # anchors stay on the device
    overlaps = find_overlaps(matcher, all_to_all=True)             # numpy structured array of OVERLAP records
    overlaps = map_reads(reads)                                    # the same in one call
    overlaps, scores = chain_overlaps(matcher, return_scores=True)  # chaining DP instead; map_reads(overlapper="chained")
    overlaps = post_process_overlaps(overlaps)                     # fuse neighbouring overlaps (the CLI's -D drops)
    overlaps = rescue_overlap_ends(overlaps, reads, reads)         # extend ends over similar flanks (the CLI's -R)
    overlaps = map_reads_batched(reads, max_basepairs_per_index=30_000_000)   # what the cudamapper tool runs
    text = format_paf(overlaps, names, lengths, names, lengths, 15)
    cigars, edit_distances = align_overlaps(overlaps, reads)       # the default aligner, nothing but text comes back
    overlaps, cigars = map_reads_batched(reads, align=True)        # the tool's --cigar
    overlaps = map_reads_batched(reads, query_indices_in_host_memory=10, query_indices_in_device_memory=5)  # -Q -q
    copy = index.to_host(); index = copy.to_device()               # packed copy in pinned host memory and back
    text = format_paf(overlaps, names, lengths, names, lengths, 15, cigars=cigars)
    segments, offsets, edit_distances = window_segments(overlaps, reads, targets, window_length=500)
    windows = overlap_windows(overlaps, reads, targets, window_length=500, max_depth=30)   # polisher.polish feeds on it
    pairs = overlaps[select_pairs(overlaps)]                       # read correction: one record per pair of reads
    (target_role, offsets, edit_distances), (query_role, query_role_offsets) = pair_segments(pairs, reads, 500)
    windows = correction_windows(overlaps, reads, window_length=500, max_depth=30)   # polisher.correct_reads feeds on it
    windows = overlap_windows_weighted(overlaps, reads, targets, query_qualities=phred33)   # + weights per sequence
    windows = correction_windows_weighted(overlaps, reads, phred33)
    piles = overlap_pileup(overlaps, reads, targets)               # uint32 (6, len(target)) per target: PILEUP_CHANNELS
    piles = pair_pileup(pairs, reads)                              # both reads of every pair, one array per read
    records = overlap_variants(overlaps, reads, targets)           # VARIANT records: SNVs, deletions, insertion alleles

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

# gwm_segment: what one overlap's alignment covers of one window of its target read
SEGMENT = np.dtype([("overlap", "<u4"), ("window", "<u4"), ("target_first", "<u4"), ("target_last", "<u4"),
                    ("query_begin", "<u4"), ("query_end", "<u4")])

# the rows of a pileup array: what the aligned overlaps put at a base of the read that owns it
PILEUP_CHANNELS = ("A", "C", "G", "T", "deletion", "insertion")

# gwm_variant: one called variant of a target read; 32 B
VARIANT = np.dtype({"names": ["target_read", "position", "count", "depth", "kind", "ref", "alt", "length", "key"],
                    "formats": ["<u4", "<u4", "<u4", "<u4", "u1", "u1", "u1", "u1", "<u8"],
                    "offsets": [0, 4, 8, 12, 16, 17, 18, 19, 24], "itemsize": 32})
VARIANT_KINDS = ("snv", "deletion", "insertion")  # the values of VARIANT's kind

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


def _read_set_args(query_reads, target_reads):
    """(bases, offsets, number of reads) of the queries and of the targets as the C API takes them; no target set,
    which there means the query set, is (None, None, 0)"""
    qb, qo = pack_reads(query_reads)
    if target_reads is None:
        return (_p(qb), _p(qo), len(query_reads)), (None, None, 0)
    tb, to = pack_reads(target_reads)
    return (_p(qb), _p(qo), len(query_reads)), (_p(tb), _p(to), len(target_reads))


def pack_qualities(qualities, reads, who="qualities"):
    """The qualities of a read set as the C API takes them: Phred+33 bytes back to back, which share the offsets of
    the set's bases. `qualities` is a list of str / bytes, one per read and of the read's length, every byte in
    33..126; anything else raises ValueError. None gives None: the set has no qualities."""
    if qualities is None:
        return None
    if len(qualities) != len(reads):
        raise ValueError("%s: %d quality strings for %d reads" % (who, len(qualities), len(reads)))
    qs = [q.encode("latin-1") if isinstance(q, str) else bytes(q) for q in qualities]
    for i, (q, r) in enumerate(zip(qs, reads)):
        if len(q) != len(r):
            raise ValueError("%s: read %d has %d bases and %d qualities" % (who, i, len(r), len(q)))
    flat = np.frombuffer(b"".join(qs) or b"!", np.uint8).copy()
    if any(qs) and (flat.min() < 33 or flat.max() > 126):
        raise ValueError("%s: a quality byte outside 33..126" % who)
    return flat


def _threshold(min_mean_quality):
    if int(min_mean_quality) < 0:
        raise ValueError("min_mean_quality must be >= 0")
    return int(min_mean_quality)


def _copy_weights(L, h, n_bases, n_records, n_query_role_records):
    """what a handle of the weighted calls holds beyond the others: (weights, quality_sums, query_role_quality_sums,
    ms[2]); arrays the call did not fill stay zero and are cut by the caller"""
    weights, ms = np.zeros(max(n_bases, 1), np.int8), np.zeros(2, np.float32)
    sums, query_role_sums = np.zeros(max(n_records, 1), np.uint32), np.zeros(max(n_query_role_records, 1), np.uint32)
    L.gw_mapper_windows_copy_weights(h, _p(weights), _p(sums), _p(query_role_sums), _p(ms))
    return weights[:n_bases], sums[:n_records], query_role_sums[:n_query_role_records], ms


class _Handle:
    """What Index, IndexHostCopy and Matcher share: self._h, a handle of the C API (self._L), is destroyed once, by the
    entry point their _destroy names: on close(), at the end of a `with` block or when the object is collected."""

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Index(_Handle):
    """Index::create_index_async + wait_to_be_ready over `reads`, whose ids are first_read_id, first_read_id + 1, ...
    (reads shorter than k + w - 1 are skipped and, as in the reference, the reads after them take their ids)."""
    _destroy = "gw_mapper_index_destroy"

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

    def to_host(self, stream=None):
        """IndexHostCopy of this index: read ids, positions, one direction bit per element and the unique-representation
        tables in one pinned host slab (gwm_index_pack). The index stays as it is."""
        return IndexHostCopy(self, stream)


class IndexHostCopy(_Handle):
    """A packed copy of an Index in pinned host memory (the reference's IndexHostCopy): nbytes is
    8 n + 8 ceil(n / 64) + 12 n_unique plus a constant, against 17 n + 12 n_unique for the arrays themselves, because
    the representation of every element is filled in again on the device. to_device() gives an Index equal to the
    packed one in all arrays and attributes. pack_ms is the device time of packing."""
    _destroy = "gw_mapper_index_host_copy_destroy"

    def __init__(self, index, stream=None):
        self._L = _native.mapper()
        self.kmer_size, self.window_size = index.kmer_size, index.window_size
        ms = C.c_float(0.0)
        self._h = self._L.gw_mapper_index_host_copy_create(index._h, _stream(stream), C.byref(ms))
        if not self._h:
            raise _err(self._L)
        self.pack_ms = ms.value
        self.nbytes = int(self._L.gw_mapper_index_host_copy_bytes(self._h))

    def to_device(self, stream=None):
        """The index again, in one device allocation (gwm_index_unpack); its restore_ms is the device time of the copy
        and the two kernels."""
        if not self._h:
            raise MapperError("the host copy is closed")
        index = Index.__new__(Index)
        index._L = self._L
        index.kmer_size, index.window_size = self.kmer_size, self.window_size
        ms = C.c_float(0.0)
        index._h = self._L.gw_mapper_index_host_copy_to_device(self._h, _stream(stream), C.byref(ms))
        index._fill()
        index.restore_ms = ms.value
        return index


class Matcher(_Handle):
    """Matcher::create_matcher(query_index, target_index): anchors sorted by (query read, target read, query position,
    target position), kept on the device for find_overlaps; anchors() copies them out. stage_ms holds the device time
    of the match and anchor-sort stages, and of chain/fuse/filter once find_overlaps ran on it."""
    _destroy = "gw_mapper_matcher_destroy"

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


def find_anchors(query_index, target_index, stream=None):
    """All anchors between two indices, as an ANCHOR array."""
    with Matcher(query_index, target_index, stream) as m:
        return m.anchors()


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


CHAINING_DEFAULTS = dict(max_gap=5000, bandwidth=500, min_chain_score=40, max_chains=4)  # minimap2's -g -r -m; not tuned


def chain_overlaps(anchors, kmer_size=15, max_gap=5000, bandwidth=500, min_chain_score=40, max_chains=4,
                   all_to_all=True, min_residues=3, min_overlap_len=250, min_bases_per_residue=1000,
                   min_overlap_fraction=0.8, return_scores=False, stream=None, return_anchors=False):
    """The chaining overlapper on a Matcher (device anchors) or on a sorted ANCHOR array (uploaded first): the anchors
    of every read pair are chained by dynamic programming, '+' and '-' each on their own, over a look-back of 64
    anchors; up to max_chains chains of at least min_chain_score per pair and orientation become OVERLAP records, which
    pass the filter of find_overlaps. Rules C1-C8 are in include/gwhip_mapper.h. Where
    find_overlaps compares an anchor with its neighbour in sort order only, a stray anchor or a second diagonal between
    two collinear anchors does not cut a chain here, and the strand is the orientation the chain was found in.
    The defaults of max_gap, bandwidth and min_chain_score are minimap2's conventions (-g, -r, -m) and are not tuned.
    Returns an OVERLAP array, or (overlaps, int32 chain scores) with return_scores; a Matcher also records the device
    time in matcher.stage_ms["chain_dp"]. Parameters out of range raise MapperError.
    return_anchors adds (anchor_offsets, anchor_positions) behind the overlaps (and the scores): the anchors of every
    record's chain in chain order, record i's as the uint32 (query_position_in_read, target_position_in_read) rows
    anchor_positions[anchor_offsets[i]:anchor_offsets[i + 1]], num_residues of them -- what align_overlaps(anchors=)
    takes. Records and scores are the same with and without it."""
    L = _native.mapper()
    chaining = np.array([kmer_size, max_gap, bandwidth, min_chain_score, max_chains], np.int32)
    args = (_p(chaining), int(bool(all_to_all)), int(min_residues), int(min_overlap_len), int(min_bases_per_residue),
            float(min_overlap_fraction))
    on_device = isinstance(anchors, Matcher)
    a = None if on_device else np.ascontiguousarray(anchors, ANCHOR)
    n_anchors = anchors.n_anchors if on_device else len(a)
    # a record holds at least max(min_residues, 1) anchors, and the chains of one orientation share none
    capacity = 2 * (n_anchors // max(int(min_residues), 1)) + 1
    out, scores, ms = np.zeros(capacity, OVERLAP), np.zeros(capacity, np.int32), C.c_float(0.0)
    if return_anchors:
        # an anchor is in at most one chain of each orientation
        offsets, positions = np.zeros(capacity + 1, np.int64), np.zeros((2 * n_anchors, 2), np.uint32)
        members = C.c_int64(0)
        more = (_p(offsets), _p(positions), len(positions), C.byref(members), C.byref(ms))
        if on_device:
            n = L.gw_mapper_chain_overlaps_anchored(anchors._h, *args, _p(out), _p(scores), capacity, *more,
                                                    _stream(stream) or anchors._stream)
        else:
            n = L.gw_mapper_chain_overlaps_anchored_host(_p(a), len(a), *args, _p(out), _p(scores), capacity, *more,
                                                         _stream(stream))
    elif on_device:
        n = L.gw_mapper_chain_overlaps(anchors._h, *args, _p(out), _p(scores), capacity, C.byref(ms),
                                       _stream(stream) or anchors._stream)
    else:
        n = L.gw_mapper_chain_overlaps_host(_p(a), len(a), *args, _p(out), _p(scores), capacity, C.byref(ms),
                                            _stream(stream))
    if n < 0:
        raise _err(L)
    if on_device:
        anchors.stage_ms["chain_dp"] = ms.value
    result = (out[:n], scores[:n]) if return_scores else (out[:n],)
    if return_anchors:
        result += (offsets[:n + 1], positions[:members.value].copy())
    return result if len(result) > 1 else result[0]


def _overlapper(overlapper, chaining):
    """the chaining values of a call that names its overlapper: None for "triggered", which takes none"""
    if overlapper not in ("triggered", "chained"):
        raise ValueError('overlapper must be "triggered" or "chained", not %r' % (overlapper,))
    if overlapper == "triggered":
        if chaining is not None:
            raise ValueError('chaining parameters are for overlapper="chained"')
        return None
    unknown = set(chaining or ()) - set(CHAINING_DEFAULTS)
    if unknown:
        raise ValueError("chaining: unknown keys %s" % sorted(unknown))
    return dict(CHAINING_DEFAULTS, **(chaining or {}))


def map_reads(queries, targets=None, k=15, w=10, filtering_parameter=1e-5, min_residues=3, min_overlap_len=250,
              min_bases_per_residue=1000, min_overlap_fraction=0.8, stream=None, overlapper="triggered",
              chaining=None, return_anchors=False):
    """Overlaps of `queries` against `targets`, or all against all (self-mappings dropped) when targets is None, with
    hashed representations as in the reference's cudamapper. One index per read set: batching into several indices
    (the CLI's -i / -t) is the caller's. overlapper="chained" finds them with chain_overlaps instead of find_overlaps;
    `chaining` is then a dict of max_gap, bandwidth, min_chain_score and max_chains (chain_overlaps' defaults for
    those left out), and the k of the chains is `k`. Any other overlapper is a ValueError. return_anchors, with the
    chained overlapper only (a ValueError otherwise), returns (overlaps, anchor_offsets, anchor_positions) as
    chain_overlaps(return_anchors=True) does."""
    chaining = _overlapper(overlapper, chaining)
    if return_anchors and chaining is None:
        raise ValueError('return_anchors is for overlapper="chained"')
    with Index(queries, k, w, True, filtering_parameter, stream=stream) as q, \
            (q if targets is None else Index(targets, k, w, True, filtering_parameter, stream=stream)) as t, \
            Matcher(q, t, stream) as m:
        if chaining is not None:
            return chain_overlaps(m, k, all_to_all=targets is None, min_residues=min_residues,
                                  min_overlap_len=min_overlap_len, min_bases_per_residue=min_bases_per_residue,
                                  min_overlap_fraction=min_overlap_fraction, stream=stream,
                                  return_anchors=bool(return_anchors), **chaining)
        return find_overlaps(m, targets is None, min_residues, min_overlap_len, min_bases_per_residue,
                             min_overlap_fraction, stream)


def post_process_overlaps(overlaps, drop_fused_overlaps=False, stream=None, timings=None):
    """Overlapper::post_process_overlaps: the overlaps (in the order find_overlaps gave them), then one fused record per
    run of neighbours that fuse; drop_fused_overlaps removes the members of fusing pairs. The rules are in
    include/gwhip_mapper.h. `timings`, if a dict, receives the device time as timings["fuse"] (ms)."""
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    out = np.zeros(len(o) + len(o) // 2, OVERLAP)
    ms = C.c_float(0.0)
    n = L.gw_mapper_post_process_overlaps(_p(o), len(o), int(bool(drop_fused_overlaps)), _p(out), len(out),
                                          _stream(stream), C.byref(ms))
    if n < 0:
        raise _err(L)
    if timings is not None:
        timings["fuse"] = ms.value
    return out[:n]


def rescue_overlap_ends(overlaps, query_reads, target_reads=None, extension=50, required_similarity=0.5,
                        first_query_read_id=0, first_target_read_id=0, stream=None, timings=None):
    """Overlapper::rescue_overlap_ends: a copy of `overlaps` with the ends moved over flanks whose 15-mer similarity is
    at least required_similarity (three rounds of up to `extension` bases, 0 <= extension <= 78). Read id r is
    query_reads[r - first_query_read_id] / target_reads[r - first_target_read_id]; target_reads None means the query
    reads. A read id outside its set or an overlap beyond its read raises MapperError."""
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP).copy()
    q, t = _read_set_args(query_reads, target_reads)
    ms = C.c_float(0.0)
    rc = L.gw_mapper_rescue_overlap_ends(_p(o), len(o), *q, *t, first_query_read_id, first_target_read_id,
                                         int(extension), float(required_similarity), _stream(stream), C.byref(ms))
    if rc != 0:
        raise _err(L)
    if timings is not None:
        timings["rescue"] = ms.value
    return o


_EXTENSION_KEYS = ("match", "mismatch", "gap_open", "gap_extend", "band", "xdrop")
_EXTENSION_DEFAULTS = (2, 4, 4, 2, 64, 200)


def _extension_args(extension):
    """extension of extend_overlaps as the C API takes it: six int32 (match, mismatch, gap_open, gap_extend, band, xdrop)
    from None (the defaults 2, 4, 4, 2, 64, 200), a 6-tuple, or a dict with these keys that may leave out any."""
    if extension is None:
        values = list(_EXTENSION_DEFAULTS)
    elif isinstance(extension, dict):
        unknown = set(extension) - set(_EXTENSION_KEYS)
        if unknown:
            raise ValueError("extension: unknown keys %s" % sorted(unknown))
        values = [extension.get(k, d) for k, d in zip(_EXTENSION_KEYS, _EXTENSION_DEFAULTS)]
    else:
        values = list(extension)
        if len(values) != 6:
            raise ValueError("extension: a dict or (match, mismatch, gap_open, gap_extend, band, xdrop)")
    a, x, o, e, b, xd = values = [int(v) for v in values]
    if not (a >= 1 and x >= 0 and a + x <= 127 and 0 <= o <= 127 and e >= 1 and a + 2 * e <= 255 and 0 <= b <= 511
            and -1 <= xd <= 2 ** 20):
        raise ValueError("extension (match %d, mismatch %d, gap_open %d, gap_extend %d, band %d, xdrop %d) outside match >= 1, "
                         "mismatch >= 0, match + mismatch <= 127, gap_open 0..127, gap_extend >= 1, match + 2 gap_extend <= 255, "
                         "band 0..511, xdrop -1..2^20" % tuple(values))
    return np.array(values, np.int32)


def extend_overlaps(overlaps, query_reads, target_reads=None, first_query_read_id=0, first_target_read_id=0,
                    extension=None, max_extension=1024, max_device_bytes=0, stream=None):
    """The ends of every overlap moved over what the affine X-drop extension aligns beyond
    them, on the device: behind the tail the up to max_extension (0 .. 2^19) bases of the query and of the target in the
    target's strand coordinates are extended from the overlap's end, in front of the head the same read back to front.
    Returns (overlaps, extensions, scores): a copy of the records with the four positions moved and every other field
    as it was, an int32 array [n][4] of the bases gained (head query, head target, tail query, tail target) and an int32
    array [n][2] of the two extensions' scores. extension: None, a dict or (match, mismatch, gap_open, gap_extend, band,
    xdrop); out of range raises ValueError. max_extension 0 returns the input. Reads, read ids, chunking within
    max_device_bytes and the refusals are align_overlaps'; align_overlaps and every consumer work on the result."""
    ext = _extension_args(extension)
    if not 0 <= int(max_extension) <= 2 ** 19:
        raise ValueError("max_extension %d outside 0..2^19" % int(max_extension))
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP).copy()
    moved, scores = np.zeros((len(o), 4), np.int32), np.zeros((len(o), 2), np.int32)
    q, t = _read_set_args(query_reads, target_reads)
    rc = L.gw_mapper_extend_overlaps(_p(o), len(o), *q, *t, first_query_read_id, first_target_read_id, _p(ext),
                                     int(max_extension), int(max_device_bytes), _stream(stream), _p(moved), _p(scores))
    if rc != 0:
        raise _err(L)
    return o, moved, scores


def _split_cigars(text, offsets):
    t = text.tobytes().decode("ascii")
    return [t[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def align_bytes_needed(query_length, target_length, max_query_length):
    """Device bytes align_overlaps counts for one overlap with slices of these lengths in a call whose longest query
    slice is max_query_length: the smallest max_device_bytes it can be aligned with (gwm_align_bytes_needed)."""
    return int(_native.mapper().gwm_align_bytes_needed(int(query_length), int(target_length), int(max_query_length)))


def align_bytes_needed_scored(query_length, target_length, band):
    """align_bytes_needed for a call of align_overlaps with a scoring of this band (gwm_align_bytes_needed_scored)."""
    return int(_native.mapper().gwm_align_bytes_needed_scored(int(query_length), int(target_length), int(band)))


def align_bytes_needed_anchored(piece_lengths, scoring=None, max_query_length=None):
    """align_bytes_needed for one overlap that align_overlaps(anchors=) cuts into pieces of these (query, target)
    lengths, under `scoring` as align_overlaps takes it; max_query_length, for scoring None, is the longest query side
    of a piece of the call (None: of these pieces) (gwm_align_bytes_needed_anchored)."""
    sc = _scoring_args(scoring)
    lengths = np.asarray(piece_lengths, np.int64).reshape(-1, 2)
    starts = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    longest = int(lengths[:, 0].max()) if max_query_length is None else int(max_query_length)
    return int(_native.mapper().gwm_align_bytes_needed_anchored(_p(starts), len(lengths), 0 if sc is None else len(sc) // 2 - 1,
                                                                0 if sc is None else int(sc[-1]), longest))


def _scoring_args(scoring):
    """scoring of align_overlaps / overlap_variants as the C API takes it: None, or four int32 (mismatch, gap_open,
    gap_extend, band) from a 4-tuple or a dict with these keys (a dict may leave out any: 4, 6, 2, 128), or, for
    two-piece gap costs, six int32 (mismatch, gap_open, gap_extend, gap_open2, gap_extend2, band) from a 6-tuple or a
    dict that has both gap_open2 and gap_extend2 (what such a dict leaves out: 6, 4, 3, 24, 2, 128)."""
    if scoring is None:
        return None
    if isinstance(scoring, dict):
        unknown = set(scoring) - {"mismatch", "gap_open", "gap_extend", "gap_open2", "gap_extend2", "band"}
        if unknown:
            raise ValueError("scoring: unknown keys %s" % sorted(unknown))
        if ("gap_open2" in scoring) != ("gap_extend2" in scoring):
            raise ValueError("scoring: gap_open2 and gap_extend2 go together")
        if "gap_open2" in scoring:
            values = [scoring.get("mismatch", 6), scoring.get("gap_open", 4), scoring.get("gap_extend", 3),
                      scoring["gap_open2"], scoring["gap_extend2"], scoring.get("band", 128)]
        else:
            values = [scoring.get("mismatch", 4), scoring.get("gap_open", 6), scoring.get("gap_extend", 2), scoring.get("band", 128)]
    else:
        values = list(scoring)
        if len(values) not in (4, 6):
            raise ValueError("scoring: a dict, (mismatch, gap_open, gap_extend, band) or "
                             "(mismatch, gap_open, gap_extend, gap_open2, gap_extend2, band)")
    values = [int(v) for v in values]
    x, o, e, b = values[0], values[1], values[2], values[-1]
    if not (1 <= x <= 255 and 0 <= o <= 255 and 1 <= e <= 255 and 0 <= b < 2 ** 31):
        raise ValueError("scoring (mismatch %d, gap_open %d, gap_extend %d, band %d) outside 1..255, 0..255, 1..255, >= 0"
                         % (x, o, e, b))
    if len(values) == 6 and not (0 <= values[3] <= 255 and 1 <= values[4] <= 255):
        raise ValueError("scoring (gap_open2 %d, gap_extend2 %d) outside 0..255, 1..255" % (values[3], values[4]))
    return np.array(values, np.int32)


def align_overlaps(overlaps, query_reads, target_reads=None, first_query_read_id=0, first_target_read_id=0,
                   max_device_bytes=0, stream=None, timings=None, scoring=None, anchors=None, anchor_kmer_size=15,
                   anchor_spacing=256):
    """Global alignment of every overlap over its own slices, on the device from the reads to the CIGAR text: query
    slice [query start, query end) against target slice [target start, target end), on '-' against that target
    slice's reverse complement as cudaaligner takes it ("TGAC"[(c >> 1) & 3] for every byte), with the default aligner
    (Hirschberg + Myers) at max_query_length = the longest query slice of the call. Returns (cigars, edit_distances):
    the strings of Alignment::convert_to_cigar() in its basic format (M for match and mismatch, I / D as cudaaligner
    names them) and an int32 array of the columns that are not a match (-1 where the aligner gave no result). Read id
    r is query_reads[r - first_query_read_id] / target_reads[r - first_target_read_id]; target_reads None means the
    query reads. Overlaps are aligned in chunks that keep within max_device_bytes (0: half of the free device memory);
    the result does not depend on it, and an overlap that does not fit alone raises, as do a read id outside its set,
    start > end and an end beyond its read. `timings`, if a dict, receives gather, align and cigar_text (device ms).
    scoring: None, or (mismatch, gap_open, gap_extend, band) as a 4-tuple or a dict -- the slices are then aligned under
    affine gap costs inside a diagonal band (include/gwhip_affine.h) instead; the edit
    distances stay the columns that are not a match, an overlap whose band |m - n| + 2 band + 1 exceeds 2048 diagonals has
    an empty CIGAR and -1, and values out of range raise ValueError before anything is launched. A 6-tuple (mismatch,
    gap_open, gap_extend, gap_open2, gap_extend2, band), or a dict with gap_open2 and gap_extend2, asks for two-piece gap
    costs, min(gap_open + L gap_extend, gap_open2 + L gap_extend2) for a run of L columns;
    the capacity is then 1024 diagonals.
    anchors: None, or (anchor_offsets, anchor_positions) as chain_overlaps(return_anchors=True) returns them -- every
    overlap is then cut at anchors of its chain and aligned piece by piece under the same aligner and scoring (rules
    G1-G6 of include/gwhip_mapper.h): anchors whose k-mer of anchor_kmer_size (1..32) bases
    does not start strictly inside both slices are dropped, the others must be strictly increasing in query and target
    (MapperError that names the overlap otherwise), one anchor per anchor_spacing (>= 1; 256 is a convention, not
    tuned) bases of the query slice becomes a cut, and the band of the scoring applies to every piece. The CIGAR is
    that of the pieces' alignments one after the other; an overlap with a piece that has no result has none. Every
    piece is what its aligner returns for that pair alone: the whole is a valid global alignment, not re-priced across
    cuts, and not claimed to be optimal. Out of range, or offsets that do not start at 0, decrease or do not end at the
    number of anchors: ValueError before anything is launched."""
    sc = _scoring_args(scoring)
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    q, t = _read_set_args(query_reads, target_reads)
    if anchors is not None:
        offsets, positions = anchors
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        positions = np.ascontiguousarray(positions, np.uint32).reshape(-1, 2)
        if not (1 <= int(anchor_kmer_size) <= 32 and int(anchor_spacing) >= 1):
            raise ValueError("anchor_kmer_size %d, anchor_spacing %d outside 1..32, >= 1"
                             % (int(anchor_kmer_size), int(anchor_spacing)))
        if len(offsets) != len(o) + 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != len(positions):
            raise ValueError("anchors: %d offsets for %d overlaps that must start at 0, never decrease and end at the %d anchors"
                             % (len(offsets), len(o), len(positions)))
        h = L.gw_mapper_align_overlaps_anchored(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id,
                                                _p(offsets), _p(positions), len(positions), int(anchor_kmer_size),
                                                int(anchor_spacing), None if sc is None else _p(sc),
                                                0 if sc is None else len(sc), int(max_device_bytes), _stream(stream))
    elif sc is None:
        h = L.gw_mapper_align_overlaps(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id,
                                       int(max_device_bytes), _stream(stream))
    else:
        scored = L.gw_mapper_align_overlaps_scored if len(sc) == 4 else L.gw_mapper_align_overlaps_scored2
        h = scored(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id, _p(sc), int(max_device_bytes),
                   _stream(stream))
    if not h:
        raise _err(L)
    try:
        n = int(L.gw_mapper_cigars_count(h))
        text = np.zeros(int(L.gw_mapper_cigars_text_bytes(h)), np.uint8)
        offsets, edits, ms = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), np.zeros(3, np.float32)
        if L.gw_mapper_cigars_copy(h, _p(text), _p(offsets), _p(edits), _p(ms)) != 0:
            raise _err(L)
    finally:
        L.gw_mapper_cigars_destroy(h)
    if timings is not None:
        timings.update(gather=float(ms[0]), align=float(ms[1]), cigar_text=float(ms[2]))
    return _split_cigars(text, offsets), edits


def _window_overlaps(overlaps, query_reads, target_reads, window_length, max_depth, first_query_read_id,
                     first_target_read_id, max_device_bytes, stream, timings, weighted=None):
    """gw_mapper_window_overlaps and everything it holds, as host arrays; max_depth None: gw_mapper_window_segments, the
    segments pass alone. weighted: None, or a dict with query_qualities, target_qualities (pack_qualities) and
    min_mean_quality for gw_mapper_window_overlaps_weighted, which receives weights and quality_sums."""
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    q, t = _read_set_args(query_reads, target_reads)
    if weighted is not None:
        qq, tq = weighted["query_qualities"], weighted["target_qualities"]
        h = L.gw_mapper_window_overlaps_weighted(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id,
                                                 None if qq is None else _p(qq), None if tq is None else _p(tq),
                                                 weighted["min_mean_quality"], int(window_length), int(max_depth),
                                                 int(max_device_bytes), _stream(stream))
    elif max_depth is None:
        h = L.gw_mapper_window_segments(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id,
                                        int(window_length), int(max_device_bytes), _stream(stream))
    else:
        h = L.gw_mapper_window_overlaps(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id,
                                        int(window_length), int(max_depth), int(max_device_bytes), _stream(stream))
    if not h:
        raise _err(L)
    try:
        counts = np.zeros(4, np.int64)
        L.gw_mapper_windows_counts(h, _p(counts))
        n_win, n_seq, n_bases, n_seg = (int(x) for x in counts)
        segments, seg_offsets = np.zeros(n_seg, SEGMENT), np.zeros(len(o) + 1, np.int64)
        edits, ms = np.zeros(len(o), np.int32), np.zeros(4, np.float32)
        L.gw_mapper_windows_copy_segments(h, _p(segments), _p(seg_offsets), _p(edits), _p(ms))
        bases, seq_offsets = np.zeros(max(n_bases, 1), np.uint8), np.zeros(n_seq + 1, np.int64)
        per_window, reads, index = np.zeros(n_win, np.int32), np.zeros(n_win, np.uint32), np.zeros(n_win, np.uint32)
        L.gw_mapper_windows_copy_windows(h, _p(bases), _p(seq_offsets), _p(per_window), _p(reads), _p(index))
        if weighted is not None:
            weights, sums, _, quality_ms = _copy_weights(L, h, n_bases, n_seg if qq is not None else 0, 0)
            weighted.update(weights=weights, quality_sums=sums)
    finally:
        L.gw_mapper_windows_destroy(h)
    if timings is not None:
        timings.update(gather=float(ms[0]), align=float(ms[1]), segments=float(ms[2]), window_gather=float(ms[3]),
                       bytes_to_host=o.nbytes + segments.nbytes + seg_offsets.nbytes + edits.nbytes + n_bases,
                       segment_bytes=segments.nbytes, window_bases=n_bases)
        if weighted is not None:
            timings.update(quality_sums=float(quality_ms[0]), weight_gather=float(quality_ms[1]),
                           bytes_to_host=timings["bytes_to_host"] + weights.nbytes + sums.nbytes)
    return (segments, seg_offsets, edits), (bases[:n_bases], seq_offsets, per_window, reads, index)


def window_segments(overlaps, query_reads, target_reads=None, window_length=500, first_query_read_id=0,
                    first_target_read_id=0, max_device_bytes=0, stream=None, timings=None):
    """What every overlap's alignment covers of every window of its target read, computed on the device from the
    alignment states (gwm_window_segments): the overlaps are aligned exactly as align_overlaps aligns them, and per
    window k = target position // window_length that holds an aligned column (match or mismatch) one SEGMENT record
    gives the smallest and largest target position (forward coordinates) and the query positions [query_begin,
    query_end) of those columns. Returns (segments, segment_offsets, edit_distances): records ordered by overlap, then
    by ascending window; those of overlap i are segments[segment_offsets[i]:segment_offsets[i + 1]]; edit_distances as
    align_overlaps returns them. Arguments, chunking and errors as for align_overlaps; window_length < 1 raises.
    Nothing but the records, their offsets and the edit distances comes back: no window is selected or gathered.
    `timings`, if a dict, receives gather, align and segments (device ms; window_gather is 0) and bytes_to_host."""
    return _window_overlaps(overlaps, query_reads, target_reads, window_length, None, first_query_read_id,
                            first_target_read_id, max_device_bytes, stream, timings)[0]


def overlap_windows(overlaps, query_reads, target_reads=None, window_length=500, max_depth=30, first_query_read_id=0,
                    first_target_read_id=0, max_device_bytes=0, stream=None, timings=None):
    """The POA windows of the target reads: [(target_read, window, [backbone, layer, ...]), ...] by target read (its
    position in the target set), then by window; every target read of L > 0 bases has windows 0 .. (L - 1) //
    window_length. The backbone is the target's bases of the window; the layers are the query slices whose alignment
    spans it, chosen by select_layers from the records of window_segments and cut out of the reads on the device ('-'
    layers reversed through the aligner's table, "TGAC"[(c >> 1) & 3]). Sequences are bytes. `timings` as for
    window_segments, plus bytes_to_host."""
    _, (bases, offsets, per_window, reads, index) = _window_overlaps(
        overlaps, query_reads, target_reads, window_length, max_depth, first_query_read_id, first_target_read_id,
        max_device_bytes, stream, timings)
    return _split_windows(bases, offsets, per_window, reads, index)


def _split_windows(bases, offsets, per_window, reads, index):
    flat = bases.tobytes()
    out, at = [], 0
    for n, r, k in zip(per_window.tolist(), reads.tolist(), index.tolist()):
        out.append((r, k, [flat[offsets[i]:offsets[i + 1]] for i in range(at, at + n)]))
        at += n
    return out


def _split_weighted_windows(bases, weights, offsets, per_window, reads, index):
    """_split_windows with the weights of every sequence as a fourth entry: views of the one array of the call"""
    out, at = [], 0
    offsets = offsets.tolist()
    for r, k, seqs in _split_windows(bases, offsets, per_window, reads, index):
        out.append((r, k, seqs, [weights[offsets[i]:offsets[i + 1]] for i in range(at, at + len(seqs))]))
        at += len(seqs)
    return out


def segment_quality_sums(segments, overlaps, qualities, first_read_id=0, query_role=False, stream=None, timings=None):
    """Q1 of INTEGRATION.md section 3l on the device (gwm_segment_quality_sums): per SEGMENT record the sum of c - 33
    over the quality bytes [query_begin, query_end) of the read that supplies its layer -- its overlap's query read,
    or with query_role its target read (the query-role records of pair_segments) --, a uint32 array in record order,
    saturating at 2**32 - 1. `qualities`: the supplying set's Phred+33 strings (str / bytes, bytes in 33..126, else
    ValueError), read ids counting from first_read_id. A record that names an overlap or a read that does not exist,
    or a range beyond its read, raises MapperError. `timings` receives quality_sums (device ms)."""
    L = _native.mapper()
    s = np.ascontiguousarray(segments, SEGMENT)
    o = np.ascontiguousarray(overlaps, OVERLAP)
    flat = pack_qualities(qualities, qualities)
    _, offsets = pack_reads(qualities)
    sums, ms = np.zeros(max(len(s), 1), np.uint32), C.c_float(0.0)
    if L.gw_mapper_segment_quality_sums(_p(s), len(s), _p(o), len(o), int(bool(query_role)), _p(flat), _p(offsets),
                                        len(qualities), first_read_id, _p(sums), _stream(stream), C.byref(ms)) != 0:
        raise _err(L)
    if timings is not None:
        timings.update(quality_sums=float(ms.value))
    return sums[:len(s)]


def overlap_windows_weighted(overlaps, query_reads, target_reads=None, query_qualities=None, target_qualities=None,
                             window_length=500, max_depth=30, min_mean_quality=10, first_query_read_id=0,
                             first_target_read_id=0, max_device_bytes=0, stream=None, timings=None):
    """overlap_windows with base qualities: [(target_read, window, [backbone, layer, ...],
    [weights, ...]), ...], the weights of a sequence an np.int8 array with one entry per base. Qualities are lists of
    Phred+33 str / bytes, one per read and of its length, or None for a set that has none (a FASTA draft). They are
    uploaded once and stay on the device. With query qualities, a record is a layer only if its quality sum
    (segment_quality_sums) is > 0 and >= min_mean_quality * its bases (racon's -q), before the ordering and the
    max_depth cut; without, the layers are those of overlap_windows. Weights are c - 33, cut out on the device by the
    plan of the bases, reversed and not complemented on '-' layers; sequences of a set without qualities get 1
    throughout. Without target_reads the targets are the queries, with the queries' qualities. Wrong lengths, bytes
    outside 33..126 and a negative min_mean_quality raise ValueError before any device call. `timings` as for
    overlap_windows, plus quality_sums and weight_gather (device ms); bytes_to_host grows by 4 B per record and one
    byte per window base."""
    weighted = dict(query_qualities=pack_qualities(query_qualities, query_reads, "query_qualities"),
                    target_qualities=None if target_reads is None else
                    pack_qualities(target_qualities, target_reads, "target_qualities"),
                    min_mean_quality=_threshold(min_mean_quality))
    _, (bases, offsets, per_window, reads, index) = _window_overlaps(
        overlaps, query_reads, target_reads, window_length, max_depth, first_query_read_id, first_target_read_id,
        max_device_bytes, stream, timings, weighted)
    return _split_weighted_windows(bases, weighted["weights"], offsets, per_window, reads, index)


def select_layers(segments, overlaps, n_queries, target_lengths, window_length=500, max_depth=30,
                  first_query_read_id=0, first_target_read_id=0, quality_sums=None, min_mean_quality=0):
    """Polishing's layer selection over host arrays, without a device (gw_mapper_select_layers; the rules are in
    INTEGRATION.md section 3j): one overlap per query read is kept (the longest query span, the first on ties); a
    SEGMENT record of a kept overlap is a layer when it reaches within window_length // 100 of both ends of its window
    and holds 1 .. 2 * window_length query bases; the layers of a window are ordered by (target_first, overlap) and
    cut at max_depth. Returns (plan, windows): plan[i] = (set, read, begin, end, reversed) of sequence i, set 0 the
    queries and 1 the targets; windows[j] = (target_read, window, first_sequence, n_sequences), backbone first.
    quality_sums (one per record, as segment_quality_sums gives them; None: no filter): a record is a layer only if
    its sum is also > 0 and >= min_mean_quality * (query_end - query_begin), rule Q2 of section 3l
    (gw_mapper_select_layers_weighted); a negative min_mean_quality raises MapperError."""
    L = _native.mapper()
    s = np.ascontiguousarray(segments, SEGMENT)
    o = np.ascontiguousarray(overlaps, OVERLAP)
    lengths = np.ascontiguousarray(target_lengths, np.int64)
    args = (_p(s), len(s), _p(o), len(o), int(n_queries), first_query_read_id, _p(lengths), len(lengths),
            first_target_read_id, int(window_length), int(max_depth))
    if quality_sums is None and min_mean_quality == 0:
        return _plan_and_table(L.gw_mapper_select_layers, args)
    sums = _sums_for(quality_sums, len(s))
    return _plan_and_table(L.gw_mapper_select_layers_weighted,
                           args + (None if sums is None else _p(sums), int(min_mean_quality)))


def _sums_for(quality_sums, n_records):
    if quality_sums is None:
        return None
    sums = np.ascontiguousarray(quality_sums, np.uint32)
    if len(sums) != n_records:
        raise ValueError("%d quality sums for %d records" % (len(sums), n_records))
    return sums


def select_pairs(overlaps):
    """Read correction's pair selection over host records, without a device (gw_mapper_select_pairs; rule C1 of
    INTEGRATION.md section 3k): records of a read with itself are dropped, and of the records of an unordered pair of
    reads, in either direction, the one with the greatest query span is kept, the first on ties. Returns the kept
    positions (int64, ascending): overlaps[select_pairs(overlaps)] are the pairs."""
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    positions = np.zeros(len(o), np.int64)
    n = L.gw_mapper_select_pairs(_p(o), len(o), _p(positions), len(positions))
    if n < 0:
        raise _err(L)
    return positions[:n]


def _correction_windows(overlaps, reads, window_length, max_depth, first_read_id, max_device_bytes, stream, timings,
                        weighted=None):
    """gw_mapper_correction_windows and everything it holds, as host arrays; max_depth None: gw_mapper_pair_segments,
    the segments pass alone over records that are pairs already. weighted: None, or a dict with qualities
    (pack_qualities) and min_mean_quality for gw_mapper_correction_windows_weighted, which receives weights,
    quality_sums and query_role_quality_sums."""
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    (bases_p, offsets_p, n_reads), _ = _read_set_args(reads, None)
    if weighted is not None:
        qq = weighted["qualities"]
        h = L.gw_mapper_correction_windows_weighted(_p(o), len(o), bases_p, offsets_p, n_reads, first_read_id,
                                                    None if qq is None else _p(qq), weighted["min_mean_quality"],
                                                    int(window_length), int(max_depth), int(max_device_bytes),
                                                    _stream(stream))
    elif max_depth is None:
        h = L.gw_mapper_pair_segments(_p(o), len(o), bases_p, offsets_p, n_reads, first_read_id, int(window_length),
                                      int(max_device_bytes), _stream(stream))
    else:
        h = L.gw_mapper_correction_windows(_p(o), len(o), bases_p, offsets_p, n_reads, first_read_id,
                                           int(window_length), int(max_depth), int(max_device_bytes), _stream(stream))
    if not h:
        raise _err(L)
    try:
        counts, n_pairs, query_ms = np.zeros(4, np.int64), C.c_int64(0), C.c_float(0.0)
        L.gw_mapper_windows_counts(h, _p(counts))
        n_win, n_seq, n_bases, n_seg = (int(x) for x in counts)
        n_query_role = L.gw_mapper_windows_copy_query_role_segments(h, None, 0, None, None, C.byref(n_pairs), None)
        n_pairs = n_pairs.value
        segments, seg_offsets = np.zeros(n_seg, SEGMENT), np.zeros(n_pairs + 1, np.int64)
        edits, ms = np.zeros(n_pairs, np.int32), np.zeros(4, np.float32)
        L.gw_mapper_windows_copy_segments(h, _p(segments), _p(seg_offsets), _p(edits), _p(ms))
        query_role, query_offsets = np.zeros(n_query_role, SEGMENT), np.zeros(n_pairs + 1, np.int64)
        positions = np.zeros(n_pairs, np.int64)
        L.gw_mapper_windows_copy_query_role_segments(h, _p(query_role), n_query_role, _p(query_offsets), _p(positions),
                                                     None, C.byref(query_ms))
        bases, seq_offsets = np.zeros(max(n_bases, 1), np.uint8), np.zeros(n_seq + 1, np.int64)
        per_window, owners, index = np.zeros(n_win, np.int32), np.zeros(n_win, np.uint32), np.zeros(n_win, np.uint32)
        L.gw_mapper_windows_copy_windows(h, _p(bases), _p(seq_offsets), _p(per_window), _p(owners), _p(index))
        if weighted is not None:
            weights, sums, query_role_sums, quality_ms = _copy_weights(
                L, h, n_bases, n_seg if qq is not None else 0, n_query_role if qq is not None else 0)
            weighted.update(weights=weights, quality_sums=sums, query_role_quality_sums=query_role_sums)
    finally:
        L.gw_mapper_windows_destroy(h)
    if timings is not None:
        timings.update(gather=float(ms[0]), align=float(ms[1]), segments=float(ms[2]), window_gather=float(ms[3]),
                       query_role_segments=float(query_ms.value), overlaps_in=len(o), pairs=n_pairs,
                       bytes_to_host=(n_pairs * OVERLAP.itemsize + segments.nbytes + query_role.nbytes +
                                      2 * seg_offsets.nbytes + edits.nbytes + n_bases),
                       segment_bytes=segments.nbytes + query_role.nbytes, window_bases=n_bases)
        if weighted is not None:
            timings.update(quality_sums=float(quality_ms[0]), weight_gather=float(quality_ms[1]),
                           bytes_to_host=timings["bytes_to_host"] + weights.nbytes + sums.nbytes +
                           query_role_sums.nbytes)
    return ((segments, seg_offsets, edits), (query_role, query_offsets), positions,
            (bases[:n_bases], seq_offsets, per_window, owners, index))


def pair_segments(pairs, reads, window_length=500, first_read_id=0, max_device_bytes=0, stream=None, timings=None):
    """The segments of both reads of every pair out of one alignment (gwm_pair_segments): `pairs` are OVERLAP records
    whose query and target ids both name reads of `reads`, each aligned once, exactly as align_overlaps(pairs, reads)
    aligns it. Returns ((target_role, segment_offsets, edit_distances), (query_role, query_role_offsets)): the first is
    what window_segments(pairs, reads) returns, byte for byte; the second holds, per window k = query position //
    window_length of the *query* read that holds an aligned column, one SEGMENT record whose target_first / target_last
    are the smallest and largest query position and whose [query_begin, query_end) are the target positions of those
    columns -- target_* describe the read that owns the window and query_* the read that supplies the layer, in either
    role. Records are ordered by pair, then by ascending window. No pair is selected here: see select_pairs. Arguments,
    chunking and errors as for window_segments. `timings` additionally receives query_role_segments (device ms)."""
    target_role, query_role, _, _ = _correction_windows(pairs, reads, window_length, None, first_read_id,
                                                        max_device_bytes, stream, timings)
    return target_role, query_role


def _plan_and_table(call, args):
    """the two calls of a selection entry point of the C API: sizes first, then the arrays"""
    L = _native.mapper()
    n_windows = C.c_int64(0)
    n = call(*args, None, 0, C.byref(n_windows), None, 0)
    if n < 0:
        raise _err(L)
    plan, table = np.zeros((n, 5), np.uint32), np.zeros((n_windows.value, 4), np.uint32)
    if call(*args, _p(plan), n, C.byref(n_windows), _p(table), len(table)) != n:
        raise _err(L)
    return [tuple(int(x) for x in row) for row in plan], [tuple(int(x) for x in row) for row in table]


def select_correction_layers(target_role, query_role, pairs, read_lengths, window_length=500, max_depth=30,
                             first_read_id=0, target_role_quality_sums=None, query_role_quality_sums=None,
                             min_mean_quality=0):
    """Read correction's layer selection over host arrays, without a device (gw_mapper_select_correction_layers; rules
    C3 and C4 of INTEGRATION.md section 3k): every record of either role of pair_segments is a layer of (its owner,
    its window) when it reaches within window_length // 100 of both ends of the window and holds 1 .. 2 * window_length
    bases of the other read; the owner is the pair's target read for target-role records and its query read for
    query-role ones. The layers of a window are ordered by (target_first, pair, target role first) and cut at
    max_depth. Returns (plan, windows) as select_layers does, with every plan entry of set 0 and windows[j][0] the
    owner. The quality sums of the records of either role (None: that role is not filtered) and min_mean_quality as
    for select_layers (gw_mapper_select_correction_layers_weighted)."""
    L = _native.mapper()
    a = np.ascontiguousarray(target_role, SEGMENT)
    b = np.ascontiguousarray(query_role, SEGMENT)
    o = np.ascontiguousarray(pairs, OVERLAP)
    lengths = np.ascontiguousarray(read_lengths, np.int64)
    args = (_p(a), len(a), _p(b), len(b), _p(o), len(o), _p(lengths), len(lengths), first_read_id, int(window_length),
            int(max_depth))
    if target_role_quality_sums is None and query_role_quality_sums is None and min_mean_quality == 0:
        return _plan_and_table(L.gw_mapper_select_correction_layers, args)
    sa, sb = _sums_for(target_role_quality_sums, len(a)), _sums_for(query_role_quality_sums, len(b))
    return _plan_and_table(L.gw_mapper_select_correction_layers_weighted,
                           args + (None if sa is None else _p(sa), None if sb is None else _p(sb),
                                   int(min_mean_quality)))


def correction_windows(overlaps, reads, window_length=500, max_depth=30, first_read_id=0, max_device_bytes=0,
                       stream=None, timings=None):
    """The POA windows of every read of a set mapped against itself: [(read, window, [backbone, layer, ...]), ...] by
    read, then by window; every read of L > 0 bases has windows 0 .. (L - 1) // window_length. `overlaps` are the
    records of the all-against-all mapping as cudamapper returned them, self overlaps and both directions included:
    select_pairs keeps one per pair of reads, that one is aligned once, and both of its reads get layers from it
    (pair_segments, select_correction_layers). Sequences are bytes. All windows are built at once and come back
    together: host memory for up to (1 + max_depth) sequences of up to 2 * window_length bases per window. `timings`
    as for pair_segments, plus overlaps_in, pairs, window_gather and bytes_to_host."""
    _, _, _, (bases, offsets, per_window, owners, index) = _correction_windows(
        overlaps, reads, window_length, max_depth, first_read_id, max_device_bytes, stream, timings)
    return _split_windows(bases, offsets, per_window, owners, index)


def correction_windows_weighted(overlaps, reads, qualities, window_length=500, max_depth=30, min_mean_quality=10,
                                first_read_id=0, max_device_bytes=0, stream=None, timings=None):
    """correction_windows with the base qualities of the set: [(read, window, [backbone,
    layer, ...], [weights, ...]), ...] as overlap_windows_weighted returns them. The records of both roles are
    filtered by their quality sums -- a target-role record's layer comes from the pair's query read, a query-role
    record's from its target read --, and every sequence, backbones included, gets the weights c - 33 of its bases.
    qualities None: unit weights and the layers of correction_windows. Refusals and `timings` as for
    overlap_windows_weighted."""
    weighted = dict(qualities=pack_qualities(qualities, reads), min_mean_quality=_threshold(min_mean_quality))
    _, _, _, (bases, offsets, per_window, owners, index) = _correction_windows(
        overlaps, reads, window_length, max_depth, first_read_id, max_device_bytes, stream, timings, weighted)
    return _split_weighted_windows(bases, weighted["weights"], offsets, per_window, owners, index)


def _copy_pileup(L, h, offsets, n_records, timings):
    """the counters of a pileup handle, copied once and cut per read of the owner set: [uint32 (6, len(read)), ...],
    views of the one buffer; the handle is destroyed"""
    if not h:
        raise _err(L)
    try:
        n_bases = int(L.gw_mapper_pileup_bases(h))
        counts, ms = np.zeros((len(PILEUP_CHANNELS), n_bases), np.uint32), np.zeros(3, np.float32)
        if L.gw_mapper_pileup_copy(h, _p(counts), _p(ms)) != 0:
            raise _err(L)
    finally:
        L.gw_mapper_pileup_destroy(h)
    if timings is not None:
        timings.update(gather=float(ms[0]), align=float(ms[1]), pileup=float(ms[2]),
                       bytes_to_host=n_records * OVERLAP.itemsize + counts.nbytes)
    return [counts[:, int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def overlap_pileup(overlaps, query_reads, target_reads=None, first_query_read_id=0, first_target_read_id=0,
                   max_device_bytes=0, stream=None, timings=None):
    """Per-base counts of the aligned overlaps over the target reads, added up on the device from the alignment states
    (gwm_overlap_pileup): a list with one uint32 array of shape (6, len(target)) per target
    read, rows as PILEUP_CHANNELS. Every overlap is aligned exactly as align_overlaps aligns it and counted as given
    -- nothing is selected, a record given twice counts twice --: an aligned column (match or mismatch) adds 1 to the
    channel of the query's base at its target position (forward target coordinates, the complement channel on '-'), a
    column with a target base only adds 1 to `deletion` there, and a run of columns with query bases only adds 1 to
    `insertion` at the smaller target position of its two neighbours, when it has one on both sides within the
    alignment. Bytes other than ACGT count as the letter the aligner folds them to, (c >> 1) & 3. depth(pile) is the
    number of records whose target slice covers a position. The arrays are views of one buffer, the only thing copied
    from the device besides the overlap records that size the chunks. Arguments, chunking and errors as for
    align_overlaps. `timings`, if a dict, receives gather, align and pileup (device ms) and bytes_to_host."""
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    q, t = _read_set_args(query_reads, target_reads)
    _, offsets = pack_reads(query_reads if target_reads is None else target_reads)
    h = L.gw_mapper_overlap_pileup(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id,
                                   int(max_device_bytes), _stream(stream))
    return _copy_pileup(L, h, offsets, len(o), timings)


def pair_pileup(pairs, reads, first_read_id=0, max_device_bytes=0, stream=None, timings=None):
    """Per-base counts over every read of a set from records whose query and target ids both name reads of it
    (gwm_pair_pileup): each pair is aligned once, as align_overlaps(pairs, reads) aligns it, and counted for both of
    its reads into one array -- for the target read as overlap_pileup counts it, and for the query read with the roles
    changed: an aligned column adds 1 to the channel of the target's base at its query position (the complement
    channel on '-'), a column with a query base only adds 1 to `deletion`, and a run of columns with target bases only
    adds 1 to `insertion` at the query position before it. Returns one uint32 array of shape (6, len(read)) per read.
    No pair is selected here: see select_pairs. Arguments, chunking, errors and `timings` as for overlap_pileup."""
    L = _native.mapper()
    o = np.ascontiguousarray(pairs, OVERLAP)
    bases, offsets = pack_reads(reads)
    h = L.gw_mapper_pair_pileup(_p(o), len(o), _p(bases), _p(offsets), len(reads), first_read_id,
                                int(max_device_bytes), _stream(stream))
    return _copy_pileup(L, h, offsets, len(o), timings)


def overlap_variants(overlaps, query_reads, target_reads=None, min_count=3, min_percent=30, first_query_read_id=0,
                     first_target_read_id=0, max_device_bytes=0, stream=None, timings=None, return_pileup=False,
                     scoring=None):
    """The variants of the target reads under their aligned overlaps, called on the device from one alignment pass
    (gwm_overlap_variants): a numpy array of VARIANT records, ascending by target read and
    position, within a position SNV, deletion, insertion. With n[0..5] the counters of overlap_pileup at a base, r the
    channel of the target's own base and d = n[0] + ... + n[4], a count k passes when k >= min_count and 100 * k >=
    min_percent * d. An SNV (kind 0) is the channel other than r with the greatest count, the smallest on a tie, when
    that count passes; a deletion (kind 1) is called per base when n[4] passes; an insertion (kind 2) after a base
    is the allele most of the insertion runs there spell -- on a tie the shorter, then the alphabetically smaller --
    when the number of runs that spell it passes: `length` and `key` hold it, insertion_allele(length, key) is its
    text, in forward target coordinates. Runs of more than 32 bases are counted in the pileup and never called.
    The defaults min_count = 3 and min_percent = 30 are conventions and are not tuned on any data. With return_pileup:
    (records, piles), piles what overlap_pileup returns for the same input, out of the same pass. Nothing but the
    records (and the counters when asked for) is copied from the device, besides the overlap records that size the
    chunks. min_count < 1 or min_percent outside 0..100 raise ValueError before anything is launched; other
    arguments, chunking and errors as for overlap_pileup. `timings`, if a dict, receives gather, align, pileup (with
    the insertion-run records) and call (device ms) and bytes_to_host. scoring as for align_overlaps: the alignments
    that are counted are then the affine-gap ones."""
    sc = _scoring_args(scoring)
    if int(min_count) < 1:
        raise ValueError("min_count must be >= 1")
    if not 0 <= int(min_percent) <= 100:
        raise ValueError("min_percent must be within 0..100")
    L = _native.mapper()
    o = np.ascontiguousarray(overlaps, OVERLAP)
    q, t = _read_set_args(query_reads, target_reads)
    _, offsets = pack_reads(query_reads if target_reads is None else target_reads)
    if sc is None:
        h = L.gw_mapper_overlap_variants(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id, int(min_count),
                                         int(min_percent), int(max_device_bytes), _stream(stream))
    else:
        scored = L.gw_mapper_overlap_variants_scored if len(sc) == 4 else L.gw_mapper_overlap_variants_scored2
        h = scored(_p(o), len(o), *q, first_query_read_id, *t, first_target_read_id, int(min_count), int(min_percent),
                   _p(sc), int(max_device_bytes), _stream(stream))
    if not h:
        raise _err(L)
    try:
        records, ms = np.zeros(int(L.gw_mapper_variants_count(h)), VARIANT), np.zeros(4, np.float32)
        if L.gw_mapper_variants_copy(h, _p(records), _p(ms)) != 0:
            raise _err(L)
        counts = None
        if return_pileup:
            counts = np.zeros((len(PILEUP_CHANNELS), int(offsets[-1])), np.uint32)
            if L.gw_mapper_variants_pileup_copy(h, _p(counts)) != 0:
                raise _err(L)
    finally:
        L.gw_mapper_variants_destroy(h)
    if timings is not None:
        timings.update(gather=float(ms[0]), align=float(ms[1]), pileup=float(ms[2]), call=float(ms[3]),
                       bytes_to_host=len(o) * OVERLAP.itemsize + records.nbytes + (counts.nbytes if return_pileup else 0))
    if not return_pileup:
        return records
    return records, [counts[:, int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def insertion_allele(length, key):
    """the text of an insertion allele of VARIANT records: `length` bases, two bits each from the top of the
    2 * length low bits of `key`, A, C, G, T = 0..3"""
    length, key = int(length), int(key)
    if not 0 <= length <= 32 or key >> (2 * length):
        raise ValueError("an allele of %d bases with key %d" % (length, key))
    return "".join("ACGT"[(key >> (2 * (length - 1 - i))) & 3] for i in range(length))


def group_reads_into_indices(read_lengths, max_basepairs_per_index):
    """group_reads_into_indices of the reference: [(first_read, number_of_reads)] over consecutive reads whose base
    count stays <= max_basepairs_per_index (a longer read stands alone). As there, a first read longer than the limit
    leaves a descriptor of zero reads in front, and no reads give [(0, 0)]."""
    L = _native.mapper()
    lengths = np.ascontiguousarray(read_lengths, np.int64)
    out = np.zeros((len(lengths) + 1, 2), np.uint32)
    n = L.gw_mapper_group_reads_into_indices(_p(lengths), len(lengths), int(max_basepairs_per_index), _p(out), len(out))
    if n < 0:
        raise _err(L)
    return [(int(a), int(b)) for a, b in out[:n]]


def generate_batches_of_indices(query_lengths, target_lengths=None, query_indices_in_host_memory=1,
                                query_indices_in_device_memory=1, target_indices_in_host_memory=None,
                                target_indices_in_device_memory=None, max_basepairs_per_index=30_000_000,
                                max_basepairs_per_target_index=None):
    """generate_batches_of_indices of the reference's index batcher: reads grouped into indices, indices into host
    batches of query_indices_in_host_memory x target_indices_in_host_memory, every host batch into device batches of
    the two device counts. target_lengths None means the target set is the query set: upper triangle only. The target
    counts default to the query's. Returns [(host_batch, [device_batch, ...]), ...] where a batch is
    (query_indices, target_indices), lists of (first_read, number_of_reads). The same set with different counts or
    index sizes, a count below 1, or fewer indices in host than in device memory raise MapperError."""
    L = _native.mapper()
    ql = np.ascontiguousarray(query_lengths, np.int64)
    tl = None if target_lengths is None else np.ascontiguousarray(target_lengths, np.int64)
    C_ = query_indices_in_host_memory if target_indices_in_host_memory is None else target_indices_in_host_memory
    c_ = query_indices_in_device_memory if target_indices_in_device_memory is None else target_indices_in_device_memory
    t_limit = max_basepairs_per_index if max_basepairs_per_target_index is None else max_basepairs_per_target_index
    args = (_p(ql), len(ql), None if tl is None else _p(tl), 0 if tl is None else len(tl), int(max_basepairs_per_index),
            int(t_limit), int(query_indices_in_host_memory), int(query_indices_in_device_memory), int(C_), int(c_))
    words = L.gw_mapper_generate_batches_of_indices(*args, None, 0)
    if words < 0:
        raise _err(L)
    flat = np.zeros(words, np.uint32)
    if L.gw_mapper_generate_batches_of_indices(*args, _p(flat), len(flat)) != words:
        raise _err(L)
    flat, at = [int(x) for x in flat], [0]

    def take(n):
        at[0] += n
        return flat[at[0] - n:at[0]]

    def batch():
        nq, nt = take(2)
        q, t = take(2 * nq), take(2 * nt)
        return list(zip(q[0::2], q[1::2])), list(zip(t[0::2], t[1::2]))

    out = []
    for _ in range(take(1)[0]):
        host = batch()
        out.append((host, [batch() for _ in range(take(1)[0])]))
    return out


def map_reads_batched(queries, targets=None, k=15, w=10, filtering_parameter=1e-5, min_residues=3, min_overlap_len=250,
                      min_bases_per_residue=1000, min_overlap_fraction=0.8, max_basepairs_per_index=30_000_000,
                      max_basepairs_per_target_index=None, post_process=True, drop_fused_overlaps=False,
                      rescue_overlap_ends=False, stream=None, timings=None, align=False, max_device_bytes=0,
                      query_indices_in_host_memory=1, query_indices_in_device_memory=1,
                      target_indices_in_host_memory=None, target_indices_in_device_memory=None,
                      overlapper="triggered", chaining=None):
    """What the cudamapper tool does on one device: queries and targets (None: all against all) grouped into indices
    of at most max_basepairs_per_index / max_basepairs_per_target_index bases (the CLI's -i / -t, given there in
    millions), every index pair mapped, its overlaps post-processed (post_process; drop_fused_overlaps is -D) and
    their ends rescued (-R) on the device, results appended in pair order. Read ids are positions in `queries` /
    `targets`. `timings`, if a dict, receives the summed device times chain_fuse_filter, fuse and rescue (ms) and the
    number of index pairs.

    The four *_indices_in_*_memory keywords are the tool's -Q -q -C -c (the target ones default to the query's): the
    index pairs are walked in host batches of Q x C indices, each in device batches of q x c
    (generate_batches_of_indices). The indices of a host batch are built once; those a later device batch needs are
    kept as packed host copies (Index.to_host) and restored on a second stream while the current device batch is
    mapped. An index that is still on the device from the previous device batch, or among the host copies of the
    previous host batch, is not built again. The overlaps are those of 1, 1, 1, 1 in the order of the batches' pairs.
    Up to 2 x (q + c) indices are on the device at a time. timings also gets index_builds, index_restores and the
    device times pack and unpack (ms).

    align=True (the tool's --cigar) aligns what is left of every index pair as align_overlaps does, one call per pair,
    with overlaps and reads staying on the device, and returns (overlaps, cigars), one CIGAR per overlap; timings
    also gets gather, align, cigar_text and the int32 array edit_distances. A read shorter than k + w - 1 then raises
    before any device work: the index would skip it and shift the read ids behind it, so the wrong sequences would be
    aligned. (The reference's -a aligns before fusion appends its records; this aligns the records returned.)

    overlapper="chained" (the tool's --chain) runs chain_overlaps in the place of find_overlaps in every index pair,
    with `chaining` as map_reads takes it; everything behind the overlapper stays as it is, and timings'
    chain_fuse_filter is then the device time of the chaining. Any other overlapper is a ValueError."""
    chaining = _overlapper(overlapper, chaining)
    L = _native.mapper()
    q, t = _read_set_args(queries, targets)
    t_limit = max_basepairs_per_index if max_basepairs_per_target_index is None else max_basepairs_per_target_index
    args = (*q, *t, k, w, float(filtering_parameter), int(min_residues), int(min_overlap_len),
            int(min_bases_per_residue), float(min_overlap_fraction), int(max_basepairs_per_index), int(t_limit),
            int(bool(post_process)), int(bool(drop_fused_overlaps)), int(bool(rescue_overlap_ends)))
    C_ = query_indices_in_host_memory if target_indices_in_host_memory is None else target_indices_in_host_memory
    c_ = query_indices_in_device_memory if target_indices_in_device_memory is None else target_indices_in_device_memory
    args += (int(bool(align)), int(max_device_bytes), int(query_indices_in_host_memory),
             int(query_indices_in_device_memory), int(C_), int(c_))
    if chaining is None:
        h = L.gw_mapper_map_batched_cached(*args, _stream(stream))
    else:
        h = L.gw_mapper_map_batched_chained(*args, *(int(chaining[name]) for name in (
            "max_gap", "bandwidth", "min_chain_score", "max_chains")), _stream(stream))
    if not h:
        raise _err(L)
    try:
        out = np.zeros(int(L.gw_mapper_overlaps_count(h)), OVERLAP)
        ms, pairs = np.zeros(3, np.float32), C.c_int64(0)
        L.gw_mapper_overlaps_copy(h, _p(out), len(out), _p(ms), C.byref(pairs))
        builds, restores, cache_ms = C.c_int64(0), C.c_int64(0), np.zeros(2, np.float32)
        L.gw_mapper_overlaps_cache_counts(h, C.byref(builds), C.byref(restores), _p(cache_ms))
        if align:
            text = np.zeros(int(L.gw_mapper_overlaps_cigar_text_bytes(h)), np.uint8)
            offsets, edits, align_ms = np.zeros(len(out) + 1, np.int64), np.zeros(len(out), np.int32), np.zeros(3, np.float32)
            if L.gw_mapper_overlaps_copy_cigars(h, _p(text), _p(offsets), _p(edits), _p(align_ms)) != 0:
                raise _err(L)
    finally:
        L.gw_mapper_overlaps_destroy(h)
    if timings is not None:
        timings.update(chain_fuse_filter=float(ms[0]), fuse=float(ms[1]), rescue=float(ms[2]), index_pairs=pairs.value,
                       index_builds=builds.value, index_restores=restores.value, pack=float(cache_ms[0]),
                       unpack=float(cache_ms[1]))
        if align:
            timings.update(gather=float(align_ms[0]), align=float(align_ms[1]), cigar_text=float(align_ms[2]),
                           edit_distances=edits)
    return (out, _split_cigars(text, offsets)) if align else out


def format_paf(overlaps, query_names, query_lengths, target_names, target_lengths, kmer_size, cigars=None):
    """The reference's PAF text (print_paf): per overlap the tab-separated line
    qname qlen qstart qend strand tname tlen tstart tend num_residues*kmer_size max(|tspan|, |qspan|) 255.
    Read ids index the name and length lists; positions and the residue product print as the reference's %i does.
    With `cigars` (one per overlap) every line continues with a tab and cg:Z:<cigar>, as the tool's --cigar and
    align_overlaps print it."""
    if cigars is not None and len(cigars) != len(overlaps):
        raise ValueError("one CIGAR per overlap")
    def i32(x):
        x &= 0xFFFFFFFF
        return x - (1 << 32) if x >= 1 << 31 else x
    lines = []
    for o in np.ascontiguousarray(overlaps, OVERLAP):
        q, t = int(o["query_read_id"]), int(o["target_read_id"])
        qs, qe = int(o["query_start_position_in_read"]), int(o["query_end_position_in_read"])
        ts, te = int(o["target_start_position_in_read"]), int(o["target_end_position_in_read"])
        lines.append("%s\t%d\t%d\t%d\t%c\t%s\t%d\t%d\t%d\t%d\t%d\t255%s\n" % (
            query_names[q], query_lengths[q], i32(qs), i32(qe), int(o["relative_strand"]), target_names[t],
            target_lengths[t], i32(ts), i32(te), i32(int(o["num_residues"]) * kmer_size),
            max(abs(ts - te), abs(qs - qe)), "" if cigars is None else "\tcg:Z:" + cigars[len(lines)]))
    return "".join(lines)
