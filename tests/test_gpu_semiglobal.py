"""cudaaligner's infix / prefix alignment types on the GPU, through genomeworks_amd.cudaaligner and through ctypes on the C
API. Every pair is held to all of:

  * (d, target_begin, target_end) equals the DP oracle (tests/oracle_semiglobal.py);
  * the states equal those of a "global" batch of the same limits on (Q, T[target_begin:target_end]);
  * the extended CIGAR replays on that slice (tests/cigar_replay.py) with cost d.

Query lengths sit on the word (32), round (2 048) and third-round (4 100) boundaries of the ends scan, plus one beyond
16 384 bases, where the scan keeps its column in the workspace instead of registers."""
import ctypes as C
import random

import pytest

import cigar_replay
import oracle_semiglobal as S
import semiglobal_cases as K

pytestmark = pytest.mark.gpu

CACHE = 2 << 30
DELETION = 3


def _oracle(pairs, mode, _memo={}):
    """One DP per (pair, mode) for the whole module."""
    out = []
    for q, t in pairs:
        key = (q, t, mode)
        if key not in _memo:
            _memo[key] = S.semiglobal(q, t, mode)
        out.append(_memo[key])
    return out


def _run(pairs, mode, max_q=None, max_t=None, batch=None):
    from genomeworks_amd import cudaaligner
    max_q = max_q or max(len(q) for q, _ in pairs) + 1
    max_t = max_t or max(len(t) for _, t in pairs) + 1
    al = batch or cudaaligner.CudaAlignerBatch(max_q, max_t, len(pairs), alignment_type=mode,
                                               max_device_memory_allocator_caching_size=CACHE)
    for q, t in pairs:
        assert al.add_alignment(q, t) == 0, (len(q), len(t))
    al.align_all()
    return al.get_alignments(), max_q, max_t


def _check(pairs, mode, max_q=None, max_t=None, batch=None):
    from genomeworks_amd import cudaaligner
    results, max_q, max_t = _run(pairs, mode, max_q, max_t, batch)
    assert len(results) == len(pairs)
    expected = _oracle(pairs, mode)
    for i, (r, (q, t), (d, te, tb)) in enumerate(zip(results, pairs, expected)):
        where = (i, len(q), len(t), mode)
        assert (r.status, r.is_optimal) == (0, True), where
        assert (r.edit_distance, r.target_begin, r.target_end) == (d, tb, te), where
        assert (r.query, r.target) == (q, t), where
    # the same limits, so that the default aligner's choice of leaves is the same
    slices = [(i, q, t[tb:te]) for i, ((q, t), (d, te, tb)) in enumerate(zip(pairs, expected)) if te > tb]
    if slices:
        ref = cudaaligner.CudaAlignerBatch(max_q, max_t, len(slices), max_device_memory_allocator_caching_size=CACHE)
        for _, q, piece in slices:
            assert ref.add_alignment(q, piece) == 0
        ref.align_all()
        for (i, q, piece), g in zip(slices, ref.get_alignments()):
            assert g.status == 0
            assert results[i].alignment == g.alignment, (i, len(q), len(piece), mode)
            assert (results[i].cigar, results[i].cigar_extended) == (g.cigar, g.cigar_extended)
    for r, (q, t), (d, te, tb) in zip(results, pairs, expected):
        if te == tb:
            assert r.alignment == [DELETION] * len(q)
            continue
        record = ["q", str(len(q)), "0", str(len(q)), "+", "t", str(len(t)), str(tb), str(te), "0", "0", "0",
                  "cg:Z:" + r.cigar_extended]
        replay = cigar_replay.replay_paf(record, {"q": q}, {"t": t})
        assert replay.edits == d and replay.target_span == (tb, te)
    return results


# ---- the query planted in a target of 3 n bases: d = 0 and known ends; then with 5 % edits ----
@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_planted_queries_every_length(mode):
    rng = random.Random(101)
    pairs, begins = [], []
    for n in K.QUERY_LENGTHS:
        for where in ("start", "middle", "end"):
            q, t, begin = K.planted(rng, n, where, edits=False)
            pairs.append((q, t))
            begins.append((n, begin))
    results = _check(pairs, mode)
    for r, (n, begin) in zip(results, begins):
        if mode == "infix" and n >= 31:      # (a query of one base also occurs earlier in a random target)
            assert (r.edit_distance, r.target_begin, r.target_end) == (0, begin, begin + n)
        if mode == "prefix" and begin == 0:
            assert (r.edit_distance, r.target_begin, r.target_end) == (0, 0, n)


@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_planted_queries_with_edits(mode):
    rng = random.Random(202)
    pairs = [K.planted(rng, n, where, edits=True)[:2] for n in K.QUERY_LENGTHS for where in ("start", "middle", "end")]
    _check(pairs, mode)


@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_every_query_length_against_every_target_length(mode):
    rng = random.Random(303)
    pairs = [K.sized_pair(rng, n, m) for n in K.QUERY_LENGTHS for m in K.target_lengths(n)]
    _check(pairs, mode)


def test_known_small_cases():
    r = _check([("AAAA", "CCCC"), ("ACG", "ACGACG"), ("GAC", "TTAC")], "infix")
    assert (r[0].edit_distance, r[0].target_begin, r[0].target_end, r[0].alignment) == (4, 0, 0, [DELETION] * 4)
    assert r[0].cigar == "4D"
    assert (r[1].edit_distance, r[1].target_begin, r[1].target_end) == (0, 0, 3)
    assert (r[2].edit_distance, r[2].target_begin, r[2].target_end) == (1, 2, 4)   # AC, not TAC: the largest begin
    assert r[2].cigar_extended == "1D2=" and r[2].format_alignment() == ("GAC", " ||", "-AC")


def test_prefix_differs_from_infix_when_the_hit_is_not_at_the_start():
    rng = random.Random(404)
    q = K.bases(rng, 64)
    t = K.bases(rng, 200) + q + K.bases(rng, 30)
    infix = _check([(q, t)], "infix")[0]
    prefix = _check([(q, t)], "prefix")[0]
    assert (infix.edit_distance, infix.target_begin, infix.target_end) == (0, 200, 264)
    assert prefix.edit_distance > 0 and prefix.target_begin == 0


@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_mixed_batch_twice_in_different_orders(mode):
    pairs = K.mixed_batch(505)
    assert len(pairs) >= 130
    first = _check(pairs, mode, max_q=4200, max_t=12400)
    order = list(range(len(pairs)))
    random.Random(6).shuffle(order)
    second, _, _ = _run([pairs[i] for i in order], mode, max_q=4200, max_t=12400)
    for k, i in enumerate(order):
        a, b = first[i], second[k]
        assert (a.edit_distance, a.target_begin, a.target_end, a.alignment, a.cigar) == \
               (b.edit_distance, b.target_begin, b.target_end, b.alignment, b.cigar), (i, k)


def test_query_beyond_the_register_variants():
    """More than 16 384 query bases: nine rounds per column, state and patterns in the workspace."""
    rng = random.Random(606)
    long_pair = K.sized_pair(rng, 16400, 16400)
    short_target = (K.bases(rng, 16400), K.bases(rng, 200))
    _check([long_pair, short_target, ("ACGT", "TTACGTT")], "infix")


def test_reset_and_reuse():
    from genomeworks_amd import cudaaligner
    rng = random.Random(707)
    al = cudaaligner.CudaAlignerBatch(300, 900, 8, alignment_type="infix", max_device_memory_allocator_caching_size=CACHE)
    for round_ in range(3):
        pairs = [K.planted(rng, rng.choice([33, 65, 200]), "middle", edits=True)[:2] for _ in range(5 + round_)]
        _check(pairs, "infix", max_q=300, max_t=900, batch=al)
        al.reset()
    assert al.get_alignments() == []


@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_limits_as_for_global(mode):
    from genomeworks_amd import cudaaligner
    al = cudaaligner.CudaAlignerBatch(10, 20, 2, alignment_type=mode, max_device_memory_allocator_caching_size=CACHE)
    gl = cudaaligner.CudaAlignerBatch(10, 20, 2, max_device_memory_allocator_caching_size=CACHE)
    for b in (al, gl):
        assert b.add_alignment("A" * 11, "ACGT") == cudaaligner.exceeded_max_length
        assert b.add_alignment("ACGT", "A" * 21) == cudaaligner.exceeded_max_length
        assert b.add_alignment("ACGT", "ACGT") == 0
        assert b.add_alignment("ACGT", "AGT") == 0
        assert b.add_alignment("ACGT", "AGT") == cudaaligner.exceeded_max_alignments
    al.align_all()
    assert [r.edit_distance for r in al.get_alignments()] == [0, 1]


def test_empty_sequences_have_the_status_global_gives_them():
    from genomeworks_amd import cudaaligner
    pairs = [("", "ACGT"), ("ACGT", ""), ("", "")]
    gl = cudaaligner.CudaAlignerBatch(10, 10, 3, max_device_memory_allocator_caching_size=CACHE)
    for q, t in pairs:
        assert gl.add_alignment(q, t) == 0
    gl.align_all()
    assert [r.status for r in gl.get_alignments()] == [0, 0, 0]
    for mode in ("infix", "prefix"):
        r = _check(pairs, mode, max_q=10, max_t=10)
        assert [x.status for x in r] == [0, 0, 0]
        assert [(x.edit_distance, x.target_begin, x.target_end, x.cigar) for x in r] == [(0, 0, 0, ""), (4, 0, 0, "4D"), (0, 0, 0, "")]


def test_constructor_refuses_band_and_algorithm():
    from genomeworks_amd import cudaaligner
    for kw in (dict(max_bandwidth=64), dict(algorithm="myers")):
        with pytest.raises(RuntimeError):
            cudaaligner.CudaAlignerBatch(10, 10, 1, alignment_type="infix", **kw)
    with pytest.raises(RuntimeError):
        cudaaligner.CudaAlignerBatch(10, 10, 1, alignment_type="local")


def test_format_alignment_prints_the_slice():
    r = _check([("ACGTACGT", "TTTTTACGTTCGTGGGG")], "infix")[0]
    query_line, pairing, target_line = r.format_alignment()
    assert target_line.replace("-", "") == r.target[r.target_begin:r.target_end]
    assert query_line.replace("-", "") == r.query and len(pairing) == len(query_line) == len(target_line)


def test_c_api_through_ctypes():
    """gw_aligner_create_typed / gw_alignment_target_range / gw_alignment_type without the Python class."""
    from genomeworks_amd import _native
    L = _native.host()
    vp, i32 = C.c_void_p, C.c_int32
    L.gw_aligner_create_typed.restype = vp
    L.gw_aligner_create_typed.argtypes = [i32, i32, i32, i32, vp, i32, C.c_int64]
    L.gw_aligner_add_alignment.argtypes = [vp, C.c_char_p, i32, C.c_char_p, i32, C.c_int, C.c_int]
    L.gw_alignment_target_range.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.gw_alignment_states.argtypes = [vp, i32, vp, i32]
    L.gw_aligner_device_alignments.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_int64)]
    for name in ("gw_alignment_status", "gw_alignment_type", "gw_alignment_edit_distance", "gw_alignment_is_optimal"):
        getattr(L, name).argtypes = [vp, i32]
    for name in ("gw_aligner_align_all", "gw_aligner_sync_alignments", "gw_aligner_destroy", "gw_aligner_relaunch"):
        getattr(L, name).argtypes = [vp]
    L.gw_last_error.restype = C.c_char_p
    assert not L.gw_aligner_create_typed(1, 100, 100, 4, None, 0, CACHE)         # AlignmentType::unset
    assert b"alignment_type" in L.gw_last_error()
    rng = random.Random(808)
    pairs = [K.planted(rng, 65, "middle", edits=True)[:2], ("GAC", "TTAC"), ("AAAA", "CCCC")]
    for code, mode in ((2, "infix"), (3, "prefix")):
        h = L.gw_aligner_create_typed(code, 100, 300, 4, None, 0, CACHE)
        assert h, L.gw_last_error()
        try:
            for q, t in pairs:
                assert L.gw_aligner_add_alignment(h, q.encode(), len(q), t.encode(), len(t), 0, 0) == 0
            assert L.gw_aligner_align_all(h) == 0 and L.gw_aligner_sync_alignments(h) == 0
            for i, ((q, t), (d, te, tb)) in enumerate(zip(pairs, _oracle(pairs, mode))):
                begin, end = i32(-1), i32(-1)
                assert L.gw_alignment_target_range(h, i, C.byref(begin), C.byref(end)) == 0
                assert (begin.value, end.value, L.gw_alignment_edit_distance(h, i)) == (tb, te, d)
                assert (L.gw_alignment_status(h, i), L.gw_alignment_type(h, i), L.gw_alignment_is_optimal(h, i)) == (0, code, 1)
                count = L.gw_alignment_states(h, i, None, 0)
                states = (C.c_int8 * max(count, 1))()
                L.gw_alignment_states(h, i, states, count)
                consumed_q = sum(1 for s in states[:count] if s != 2)
                consumed_t = sum(1 for s in states[:count] if s != 3)
                assert (consumed_q, consumed_t) == (len(q), te - tb)
            assert L.gw_alignment_target_range(h, 99, None, None) == -1
            # no device-resident results for these types: said, not crashed
            n_dev, total = i32(0), C.c_int64(0)
            assert L.gw_aligner_device_alignments(h, C.byref(n_dev), C.byref(total)) == 1
            assert L.gw_aligner_relaunch(h) == -1 and b"relaunch" in L.gw_last_error()
        finally:
            L.gw_aligner_destroy(h)
    # a global aligner answers 0 and the target's length
    h = L.gw_aligner_create_typed(0, 100, 100, 2, None, 0, CACHE)
    try:
        assert L.gw_aligner_add_alignment(h, b"ACGT", 4, b"ACGGT", 5, 0, 0) == 0
        assert L.gw_aligner_align_all(h) == 0 and L.gw_aligner_sync_alignments(h) == 0
        begin, end = i32(-1), i32(-1)
        assert L.gw_alignment_target_range(h, 0, C.byref(begin), C.byref(end)) == 0
        assert (begin.value, end.value, L.gw_alignment_type(h, 0)) == (0, 5, 0)
    finally:
        L.gw_aligner_destroy(h)
