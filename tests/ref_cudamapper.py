"""TEST INFRASTRUCTURE: ctypes binding of oracle/_ref/libref_cudamapper_simt.so -- the REFERENCE's own cudamapper sketch, index,
matcher and overlapper (its CUDA sources compiled by g++ where they lie, kernels run on the CPU by oracle/simt/simt.hpp;
`make -C oracle -f Makefile.ref ref_cudamapper_simt`). Results come in the shapes of tests/oracle_mapper.py, so the oracle and the
reference compare with plain array equality. Only what checks the mapper oracle and writes
tests/golden/cudamapper_reference_simt.npz uses it."""
import ctypes as C
import os

import numpy as np

from oracle_mapper import ANCHOR, OVERLAP, pack_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "oracle", "_ref", "libref_cudamapper_simt.so")
INDEX_ARRAYS = ("representations", "read_ids", "positions_in_reads", "directions", "unique_representations",
                "first_occurrence_of_representations")
INDEX_SCALARS = ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read")
_lib = None
vp, ll, u32 = C.c_void_p, C.c_longlong, C.c_uint


def available():
    return os.path.exists(PATH)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(PATH)
        L.rcm_index_create.restype = vp
        L.rcm_index_create.argtypes = [vp, vp, C.c_int, u32, C.c_int, C.c_int, C.c_int, C.c_double]
        L.rcm_index_from_arrays.restype = vp
        L.rcm_index_from_arrays.argtypes = [ll, vp, vp, vp, vp, ll, vp, vp, ll, u32, u32, u32, u32]
        L.rcm_index_destroy.argtypes = [vp]
        L.rcm_index_sizes.argtypes = [vp, vp, vp]
        L.rcm_index_arrays.argtypes = [vp] * 7
        L.rcm_anchors_create.restype = vp
        L.rcm_anchors_create.argtypes = [vp, vp]
        L.rcm_anchors_size.restype = ll
        L.rcm_anchors_size.argtypes = [vp]
        L.rcm_anchors_copy.argtypes = [vp, vp]
        L.rcm_anchors_destroy.argtypes = [vp]
        L.rcm_overlaps.restype = ll
        L.rcm_overlaps.argtypes = [vp, ll, C.c_int, ll, ll, ll, C.c_float, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(vp)


def _read_index(h):
    L = lib()
    sizes, scalars = np.zeros(3, np.int64), np.zeros(4, np.uint32)
    L.rcm_index_sizes(h, _p(sizes), _p(scalars))
    n, nu, nf = (int(x) for x in sizes)
    rep, rid, pos, d = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    uq, fo = np.zeros(nu, np.uint64), np.zeros(nf, np.uint32)
    L.rcm_index_arrays(h, _p(rep), _p(rid), _p(pos), _p(d), _p(uq), _p(fo))
    out = dict(zip(INDEX_ARRAYS, (rep, rid, pos, d, uq, fo)))
    out.update((name, int(v)) for name, v in zip(INDEX_SCALARS, scalars))
    return out


def index(reads, k, w, hash_representations=True, filtering_parameter=1.0, first_read_id=0):
    """The reference's IndexGPU<Minimizer> of the reads: the dict of tests/oracle_mapper.index."""
    bases, offsets = pack_reads(reads)
    h = lib().rcm_index_create(_p(bases), _p(offsets), len(reads), first_read_id, k, w, int(bool(hash_representations)),
                               float(filtering_parameter))
    if not h:
        raise RuntimeError("the reference's IndexGPU threw")
    try:
        return _read_index(h)
    finally:
        lib().rcm_index_destroy(h)


def _handle(ix):
    a = [np.ascontiguousarray(ix[name]) for name in INDEX_ARRAYS]
    h = lib().rcm_index_from_arrays(len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), len(a[4]), _p(a[4]), _p(a[5]), len(a[5]),
                                    *(int(ix[name]) for name in INDEX_SCALARS))
    if not h:
        raise RuntimeError("no index from arrays")
    return h


def anchors(q, t):
    """The reference's MatcherGPU on two index dicts (of index() above, of the oracle, or built by hand)."""
    L = lib()
    hq, ht = _handle(q), _handle(t)
    try:
        ha = L.rcm_anchors_create(hq, ht)
        if not ha:
            raise RuntimeError("the reference's MatcherGPU threw")
        try:
            out = np.zeros(L.rcm_anchors_size(ha), ANCHOR)
            L.rcm_anchors_copy(ha, _p(out))
            return out
        finally:
            L.rcm_anchors_destroy(ha)
    finally:
        L.rcm_index_destroy(hq)
        L.rcm_index_destroy(ht)


def overlaps(anchor_array, all_to_all=True, min_residues=3, min_overlap_len=250, min_bases_per_residue=1000,
             min_overlap_fraction=0.8):
    """The reference's OverlapperTriggered::get_overlaps on sorted anchors."""
    a = np.ascontiguousarray(anchor_array, ANCHOR)
    out = np.zeros(max(len(a), 1), OVERLAP)
    n = lib().rcm_overlaps(_p(a), len(a), int(bool(all_to_all)), min_residues, min_overlap_len, min_bases_per_residue,
                           min_overlap_fraction, _p(out))
    if n < 0:
        raise RuntimeError("the reference's OverlapperTriggered threw")
    return out[:n]
