"""Python mirror of pygenomeworks' genomeworks.cudaaligner (cudaaligner.pyx) over the object-level C API.

CudaAlignerBatch keeps the reference's constructor (the default, fixed-stride factory); `max_bandwidth=` selects the
banded Myers aligner (create_aligner(global_alignment, max_bandwidth, ...)), which is what the benchmarks use.
`alignment_type="infix"` / `"prefix"` (not in pygenomeworks) place the whole query on the best slice / the best prefix of
its target: CudaAlignment.target_begin / .target_end name the slice that the states, the CIGARs and the distance describe.
`algorithm="affine"` (not in pygenomeworks) aligns globally under gap-open / gap-extend costs inside a diagonal band
(include/gwhip_affine.h states the rules): its alignments carry `.cost`.
`algorithm="extend"` (not in pygenomeworks) is the affine X-drop extension of the same header: from the first base of both
sequences to where the similarity stops; its alignments carry `.query_end`, `.target_end`, `.score` and `.dropped`."""
import ctypes as C

import numpy as np

from . import _native
from .cuda import CudaStream

# cudaaligner::StatusType (cudaaligner.hpp:34-42)
success = 0
uninitialized = 1
exceeded_max_alignments = 2
exceeded_max_length = 3
exceeded_max_alignment_difference = 4
generic_error = 5

# cudaaligner::AlignmentType (cudaaligner.hpp); the reference has global_alignment and unset only
_ALIGNMENT_TYPES = {"global": 0, "infix": 2, "prefix": 3}

_STATUS = {0: "success", 1: "uninitialized", 2: "exceeded_max_alignments", 3: "exceeded_max_length",
           4: "exceeded_max_alignment_difference", 5: "generic_error"}


def status_to_str(status):
    if status not in _STATUS:
        raise RuntimeError("Unknown error status : " + str(status))
    return _STATUS[status]


def _bind(L):
    if getattr(L, "_gw_aln_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.gw_aligner_create_banded.restype = vp
    L.gw_aligner_create_banded.argtypes = [i32, vp, i32, C.c_int64]
    L.gw_aligner_create.restype = vp
    L.gw_aligner_create.argtypes = [i32, i32, i32, vp, i32, C.c_int64]
    L.gw_aligner_create_typed.restype = vp
    L.gw_aligner_create_typed.argtypes = [i32, i32, i32, i32, vp, i32, C.c_int64]
    L.gw_alignment_target_range.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.gw_aligner_stage_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.gw_aligner_create_affine.restype = vp
    L.gw_aligner_create_affine.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, i32, C.c_int64]
    L.gw_aligner_create_affine2.restype = vp
    L.gw_aligner_create_affine2.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, C.c_int64]
    L.gw_alignment_cost.argtypes = [vp, i32]
    L.gw_aligner_create_extension.restype = vp
    L.gw_aligner_create_extension.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, C.c_int64]
    L.gw_alignment_extension.argtypes = [vp, i32, C.POINTER(i32 * 4)]
    L.gw_aligner_create_algorithm.restype = vp
    L.gw_aligner_create_algorithm.argtypes = [C.c_char_p, i32, i32, i32, vp, i32, C.c_int64]
    L.gw_aligner_destroy.argtypes = [vp]
    L.gw_aligner_add_alignment.argtypes = [vp, C.c_char_p, i32, C.c_char_p, i32, C.c_int, C.c_int]
    for n in ("gw_aligner_align_all", "gw_aligner_sync_alignments", "gw_aligner_num_alignments", "gw_aligner_reset",
              "gw_aligner_relaunch"):
        getattr(L, n).argtypes = [vp]
    for n in ("gw_alignment_status", "gw_alignment_is_optimal", "gw_alignment_edit_distance"):
        getattr(L, n).argtypes = [vp, i32]
    L.gw_alignment_cigar.restype = C.POINTER(C.c_char)
    L.gw_alignment_cigar.argtypes = [vp, i32, i32, C.POINTER(i32)]
    L.gw_alignment_states.argtypes = [vp, i32, vp, i32]
    L.gw_aligner_band_cells.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.gw_aligner_relaunch_timed.argtypes = [vp, C.POINTER(C.c_float)]
    L.gw_aligner_get_runs.restype = C.c_int64
    L.gw_aligner_get_runs.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp]
    L.gw_aligner_device_alignments.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_int64)]
    L.gw_aligner_copy_device_alignments.argtypes = [vp, vp, vp, vp, vp]
    L._gw_aln_bound = True
    return L


class CudaAlignment:
    """One alignment result (pygenomeworks CudaAlignment): query, target, cigar, status, alignment states."""

    def __init__(self, query, target, cigar, cigar_extended, status, is_optimal, edit_distance, states,
                 target_begin=0, target_end=None, cost=-1, extension=None):
        self.query = query
        self.target = target
        self.cigar = cigar
        self.cigar_extended = cigar_extended
        self.status = status
        self.is_optimal = is_optimal
        self.edit_distance = edit_distance
        self.alignment = states
        # the slice of the target that the alignment covers: all of it unless the batch is "infix" or "prefix"
        self.target_begin = target_begin
        self.target_end = len(target) if target_end is None else target_end
        # algorithm="affine": the alignment's cost under the batch's scoring; -1 for every other aligner
        self.cost = cost
        # algorithm="extend": query[:query_end] is aligned with target[:target_end] at `score`; dropped: the stop rule ended
        # the extension. -1, -1 and False for every other aligner, whose target_end is the one above
        self.query_end, self.score, self.dropped = -1, -1, False
        if extension is not None:
            self.query_end, self.target_end, self.score, self.dropped = extension[0], extension[1], extension[2], bool(extension[3])

    def format_alignment(self):
        """(query line, pairing line, target line) like Alignment::format_alignment, over target[target_begin:target_end]."""
        q, p, t, qi, ti = [], [], [], 0, self.target_begin
        for s in self.alignment:
            if s in (0, 1):
                q.append(self.query[qi]); t.append(self.target[ti]); p.append("|" if s == 0 else "x"); qi += 1; ti += 1
            elif s == 3:
                q.append(self.query[qi]); t.append("-"); p.append(" "); qi += 1
            else:
                q.append("-"); t.append(self.target[ti]); p.append(" "); ti += 1
        return "".join(q), "".join(p), "".join(t)


class CudaAlignerBatch:
    """Python API for GPU-accelerated global pairwise alignment (pygenomeworks CudaAlignerBatch)."""

    def __init__(self, max_query_length=None, max_target_length=None, max_alignments=None, alignment_type="global",
                 stream=None, device_id=0, max_device_memory_allocator_caching_size=-1, max_bandwidth=None,
                 algorithm=None, mismatch=None, gap_open=None, gap_extend=None, band_width=None, gap_open2=None,
                 gap_extend2=None, match=None, xdrop=None):
        """algorithm (not in pygenomeworks): one of the reference's non-public aligner classes that its C++ tests and
        benchmarks construct directly -- "hirschberg_myers" (the default), "ukkonen", "myers" -- or "affine": global
        alignment under the costs mismatch (4), gap_open (6), gap_extend (2) -- minimised, a gap run of L columns costs
        gap_open + L * gap_extend -- within band_width (128) diagonals on either side of the corners' diagonals. With
        gap_open2 and gap_extend2 (both, or neither) the gap costs are two-piece, min(gap_open + L * gap_extend,
        gap_open2 + L * gap_extend2), and what is left out of (mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        is taken from (6, 4, 3, 24, 2). "extend": the affine X-drop extension under the scores match (2), mismatch (4),
        gap_open (4), gap_extend (2) -- maximised, a gap run of L columns scores -(gap_open + L * gap_extend) -- within
        band_width (64) diagonals on either side of the start's, stopping xdrop (200; -1: never) below the best score."""
        self._L = _bind(_native.host())
        extension = dict(match=match, xdrop=xdrop)
        if algorithm != "extend" and any(v is not None for v in extension.values()):
            raise RuntimeError("%s: only algorithm=\"extend\" takes these" % ", ".join(k for k, v in extension.items() if v is not None))
        if algorithm == "extend" and (gap_open2 is not None or gap_extend2 is not None):
            raise RuntimeError("gap_open2, gap_extend2: the extension has one-piece gap costs")
        scoring = dict(mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend, band_width=band_width)
        second = dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
        given = [k for k, v in second.items() if v is not None]
        if algorithm != "affine" and given:
            raise RuntimeError("%s: only algorithm=\"affine\" takes these" % ", ".join(given))
        if len(given) == 1:
            raise RuntimeError("%s without %s: two-piece gap costs take both" % (given[0], (set(second) - set(given)).pop()))
        if algorithm not in ("affine", "extend") and any(v is not None for v in scoring.values()):
            raise RuntimeError("%s: only algorithm=\"affine\" takes these" % ", ".join(k for k, v in scoring.items() if v is not None))
        if alignment_type not in _ALIGNMENT_TYPES:
            raise RuntimeError("Unknown alignment_type provided. Must be global, infix or prefix.")
        if alignment_type != "global" and (max_bandwidth is not None or algorithm is not None):
            raise RuntimeError("alignment_type %r has one aligner: max_bandwidth and algorithm select global aligners" % alignment_type)
        self.alignment_type = alignment_type
        if stream is not None and not isinstance(stream, CudaStream):
            raise RuntimeError("Type for stream option must be CudaStream")
        self.stream = stream
        st = stream.stream if stream is not None else None
        if alignment_type != "global":
            self._h = self._L.gw_aligner_create_typed(_ALIGNMENT_TYPES[alignment_type], int(max_query_length),
                                                      int(max_target_length), int(max_alignments), st, device_id,
                                                      int(max_device_memory_allocator_caching_size))
        elif max_bandwidth is not None:
            self._h = self._L.gw_aligner_create_banded(int(max_bandwidth), st, device_id,
                                                       int(max_device_memory_allocator_caching_size))
        elif algorithm == "affine" and given:
            x, o, e, b = (d if v is None else int(v) for v, d in zip(scoring.values(), (6, 4, 3, 128)))
            self._h = self._L.gw_aligner_create_affine2(int(max_query_length), int(max_target_length), int(max_alignments),
                                                        x, o, e, int(gap_open2), int(gap_extend2), b, st, device_id,
                                                        int(max_device_memory_allocator_caching_size))
        elif algorithm == "affine":
            x, o, e, b = (d if v is None else int(v) for v, d in zip(scoring.values(), (4, 6, 2, 128)))
            self._h = self._L.gw_aligner_create_affine(int(max_query_length), int(max_target_length), int(max_alignments),
                                                       x, o, e, b, st, device_id,
                                                       int(max_device_memory_allocator_caching_size))
        elif algorithm == "extend":
            a, x, o, e, b, X = (d if v is None else int(v) for v, d in
                                zip((match, mismatch, gap_open, gap_extend, band_width, xdrop), (2, 4, 4, 2, 64, 200)))
            self._h = self._L.gw_aligner_create_extension(int(max_query_length), int(max_target_length), int(max_alignments),
                                                          a, x, o, e, b, X, st, device_id,
                                                          int(max_device_memory_allocator_caching_size))
        elif algorithm is not None:
            self._h = self._L.gw_aligner_create_algorithm(algorithm.encode(), int(max_query_length), int(max_target_length),
                                                          int(max_alignments), st, device_id,
                                                          int(max_device_memory_allocator_caching_size))
        else:
            self._h = self._L.gw_aligner_create(int(max_query_length), int(max_target_length), int(max_alignments), st,
                                                device_id, int(max_device_memory_allocator_caching_size))
        if not self._h:
            raise RuntimeError(self._L.gw_last_error().decode())
        self._pairs = []
        self._extends = algorithm == "extend"

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.gw_aligner_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def add_alignment(self, query, target, reverse_complement_query=False, reverse_complement_target=False):
        """Queue one pair. Returns the StatusType (exceeded_max_alignments: run the batch, reset, retry)."""
        q = query.encode("utf-8") if isinstance(query, str) else bytes(query)
        t = target.encode("utf-8") if isinstance(target, str) else bytes(target)
        st = self._L.gw_aligner_add_alignment(self._h, q, len(q), t, len(t), int(reverse_complement_query),
                                              int(reverse_complement_target))
        if st < 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        if st == success:
            self._pairs.append((q.decode(), t.decode()))
        return st

    def align_all(self):
        st = self._L.gw_aligner_align_all(self._h)
        if st != 0:
            raise RuntimeError("align_all failed: %s" % (self._L.gw_last_error().decode() if st < 0 else status_to_str(st)))

    def relaunch(self):
        """Benchmark helper: run the kernels again on the inputs resident in HBM (before get_alignments)."""
        if self._L.gw_aligner_relaunch(self._h) != 0:
            raise RuntimeError(self._L.gw_last_error().decode())

    def relaunch_timed(self):
        """Benchmark helper: relaunch and return the kernels' time in ms (HIP events on the aligner's stream)."""
        ms = C.c_float(0)
        if self._L.gw_aligner_relaunch_timed(self._h, C.byref(ms)) != 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        return ms.value

    def device_sync(self):
        """Wait for align_all() and report what get_alignments_device() holds: (n_alignments, total runs)."""
        n, total = C.c_int32(0), C.c_int64(0)
        if self._L.gw_aligner_device_alignments(self._h, C.byref(n), C.byref(total)) < 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        return n.value, total.value

    def stage_ms(self):
        """Measurement aid for "infix" / "prefix" batches: (ends scan ms, gather + traceback ms) of the last align_all();
        for algorithm="affine": (forward pass ms, traceback ms)."""
        ends, tb = C.c_float(0), C.c_float(0)
        if self._L.gw_aligner_stage_ms(self._h, C.byref(ends), C.byref(tb)) != 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        return ends.value, tb.value

    def band_cells(self):
        v = C.c_uint64(0)
        if self._L.gw_aligner_band_cells(self._h, C.byref(v)) != 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        return v.value

    def sync(self):
        """sync_alignments() only (host materialisation in the library, no Python marshalling). Returns the count."""
        st = self._L.gw_aligner_sync_alignments(self._h)
        if st != 0:
            raise RuntimeError("sync_alignments failed")
        return self._L.gw_aligner_num_alignments(self._h)

    def get_runs(self):
        """sync_alignments() + every alignment as a run-length CIGAR in forward order, without per-alignment Python
        objects: dict(offsets[n + 1], ops, counts, status[n], optimal[n]) of numpy arrays."""
        n = self.sync()
        total = self._L.gw_aligner_get_runs(self._h, None, None, None, 0, None, None)
        if total < 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        offsets = np.zeros(n + 1, np.int64)
        ops = np.zeros(max(total, 1), np.int8)
        counts = np.zeros(max(total, 1), np.int32)
        status = np.zeros(max(n, 1), np.int32)
        optimal = np.zeros(max(n, 1), np.int32)
        self._L.gw_aligner_get_runs(self._h, offsets.ctypes.data, ops.ctypes.data, counts.ctypes.data, total,
                                    status.ctypes.data, optimal.ctypes.data)
        return dict(offsets=offsets, ops=ops[:total], counts=counts[:total], status=status[:n], optimal=optimal[:n])

    def get_alignments_device(self):
        """Aligner::get_alignments_device() read back for inspection (stream synchronised first): dict of numpy arrays
        cigar_operations, cigar_runlengths (each alignment back to front), cigar_offsets[n + 1], metadata[n] (bit 31
        is_optimal, bits 26-0 index as added), or None for aligners without a device-resident form."""
        n, total = C.c_int32(0), C.c_int64(0)
        rc = self._L.gw_aligner_device_alignments(self._h, C.byref(n), C.byref(total))
        if rc < 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        if rc != 0:
            return None
        ops = np.zeros(max(total.value, 1), np.int8)
        runs = np.zeros(max(total.value, 1), np.int32)
        offs = np.zeros(n.value + 1, np.int32)
        meta = np.zeros(max(n.value, 1), np.uint32)
        if self._L.gw_aligner_copy_device_alignments(self._h, ops.ctypes.data, runs.ctypes.data, offs.ctypes.data, meta.ctypes.data) != 0:
            raise RuntimeError(self._L.gw_last_error().decode())
        return dict(cigar_operations=ops[:total.value], cigar_runlengths=runs[:total.value], cigar_offsets=offs,
                    metadata=meta[:n.value], total_length=total.value, n_alignments=n.value)

    def get_alignments(self):
        """sync_alignments() + list of CudaAlignment in the order the pairs were added."""
        n = self.sync()
        out = []
        for i in range(n):
            ln = C.c_int32(0)
            p = self._L.gw_alignment_cigar(self._h, i, 0, C.byref(ln))
            cigar = C.string_at(p, ln.value).decode()
            p = self._L.gw_alignment_cigar(self._h, i, 1, C.byref(ln))
            cigar_x = C.string_at(p, ln.value).decode()
            ns = self._L.gw_alignment_states(self._h, i, None, 0)
            states = np.zeros(max(ns, 1), np.int8)
            self._L.gw_alignment_states(self._h, i, states.ctypes.data, ns)
            q, t = self._pairs[i] if i < len(self._pairs) else ("", "")
            st, opt, ed = (self._L.gw_alignment_status(self._h, i), self._L.gw_alignment_is_optimal(self._h, i),
                           self._L.gw_alignment_edit_distance(self._h, i))
            tb, te, rng = C.c_int32(0), C.c_int32(len(t)), 0
            if self.alignment_type != "global":  # a global alignment covers its whole target
                rng = self._L.gw_alignment_target_range(self._h, i, C.byref(tb), C.byref(te))
            if ns < 0 or st < 0 or opt < 0 or ed < 0 or rng < 0:  # the C ABI reports a bad index / a thrown accessor as -1 + error string
                raise RuntimeError("alignment %d: %s" % (i, self._L.gw_last_error().decode()))
            extension = None
            if self._extends:
                four = (C.c_int32 * 4)()
                if self._L.gw_alignment_extension(self._h, i, C.byref(four)) != 0:
                    raise RuntimeError("alignment %d: %s" % (i, self._L.gw_last_error().decode()))
                extension = list(four)
            out.append(CudaAlignment(q, t, cigar, cigar_x, st, bool(opt), ed, [int(x) for x in states[:ns]], tb.value, te.value,
                                     self._L.gw_alignment_cost(self._h, i), extension))
        return out

    def reset(self):
        self._L.gw_aligner_reset(self._h)
        self._pairs = []
