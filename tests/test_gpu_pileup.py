"""Pileups on the device (tests/oracle_pileup.py is the oracle). The expected counts are the
CIGAR formulation applied to what align_overlaps() returns on the device for the same records, so the aligner's
tie-breaks cannot make a test pass or fail: the cases worked out on paper (their literal cells asserted too), perfect
matches around the tile boundaries, insertion runs across a tile boundary, many atomics on the same words, every cell
of the mapped small cases in both roles, independence of the chunking, the two polisher entry points and the
refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle_correct as OC
import oracle_mapper as O
import oracle_pileup as OPi
import oracle_polish as OPo
import pileup_cases as PC

pytestmark = pytest.mark.gpu

INSERTION = PC.CHANNELS.index("insertion")


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


def by_cigar(cm, o, queries, targets=None, **ids):
    """the oracle's alignments of the CIGAR formulation: the device's own CIGARs of the records"""
    cigars, _ = cm.align_overlaps(o, queries, targets, **ids)
    return OPi.of_cigars(cigars)


def run_starts(cigar, op):
    """the columns at which the runs of `op` of a CIGAR begin"""
    at, out = 0, []
    for n, c in OPi.CR.parse_cigar(cigar, "MID"):
        if c == op:
            out.append(at)
        at += n
    return out


@pytest.fixture(scope="module")
def polishing(cm):
    """the small case against two 3 % drafts of its genome, mapped on the device: reads, drafts, overlaps, alignments"""
    reads, genome = OPo.small_case()
    drafts = [OPo.draft_of(genome, 0.03, OPo.SMALL["seed"]), PC.rc(OPo.draft_of(genome, 0.03, 5))]
    o = cm.map_reads_batched(reads, drafts, rescue_overlap_ends=True, **OPo.MAPPING)
    assert len(o) >= 30 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    assert set(o["target_read_id"].tolist()) == {0, 1}
    return reads, drafts, o, by_cigar(cm, o, reads, drafts)


@pytest.fixture(scope="module")
def correction(cm):
    """the small case mapped against itself as two sets on the device: reads, all records, the pairs, their alignments"""
    reads, _ = OPo.small_case()
    o = cm.map_reads_batched(reads, reads, rescue_overlap_ends=True, **OPo.MAPPING)
    pairs = o[cm.select_pairs(o)]
    assert len(pairs) >= 100 and {chr(s) for s in pairs["relative_strand"]} == {"+", "-"}
    return reads, o, pairs, by_cigar(cm, pairs, reads)


@pytest.mark.parametrize("name", PC.NAMES)
def test_hand_cases(cm, name):
    reads, o = PC.reads(), PC.records([name])
    alignments = by_cigar(cm, o, reads)
    timings = {}
    got = cm.overlap_pileup(o, reads, reads, timings=timings)
    assert all(p.dtype == np.uint32 and p.shape == (6, len(r)) for p, r in zip(got, reads))
    assert PC.same(got, OPi.overlap_pileup(o, reads, reads, alignments, "cigar"))
    assert PC.same(got, PC.expected([name], (False,)))
    assert PC.same(cm.overlap_pileup(o, reads), got)  # no target set: the queries
    assert all(timings[k] > 0 for k in ("gather", "align", "pileup"))
    assert timings["bytes_to_host"] == o.nbytes + 24 * sum(len(r) for r in reads)
    both = cm.pair_pileup(o, reads, timings=timings)
    assert PC.same(both, OPi.pair_pileup(o, reads, alignments, "cigar"))
    assert PC.same(both, PC.expected([name]))
    assert all(timings[k] > 0 for k in ("gather", "align", "pileup"))


def test_records_count_as_given(cm):
    reads = PC.reads()
    names = ["insertion_of_two", "insertion_of_two", "mismatch_reverse", "insertion_of_two"]
    got = cm.pair_pileup(PC.records(names), reads)
    assert PC.same(got, PC.expected(names)) and got[0][INSERTION, PC.TS + 5] == 3
    # all cases in one call: the target read collects them all
    assert PC.same(cm.pair_pileup(PC.records(PC.NAMES), reads), PC.expected(PC.NAMES))
    # 40 copies of one record: atomics on the same words
    for name in ("insertion_of_two", "deleted_target_base_reverse"):
        once = cm.pair_pileup(PC.records([name]), reads)
        many = cm.pair_pileup(PC.records([name] * 40), reads)
        assert PC.same(many, [40 * p for p in once]) and once[0].sum() > 0
    # two empty slices and no records at all: zeros of the right shapes
    empty = np.array([(1, 0, 3, 4, 3, 4, ord("-"), 0, 0)], O.OVERLAP)
    for o in (empty, empty[:0]):
        for got in (cm.pair_pileup(o, reads), cm.overlap_pileup(o, reads[1:], reads[:1])):
            assert all(p.dtype == np.uint32 and p.shape[0] == 6 and not p.any() for p in got)
        assert [p.shape[1] for p in cm.pair_pileup(o, reads)] == [len(r) for r in reads]
    assert cm.pair_pileup(empty[:0], []) == []


COLUMNS = (1, 63, 64, 65, 128, 129)


def test_perfect_matches_around_the_tile_boundaries(cm):
    rng = np.random.default_rng(64)
    targets = ["".join(rng.choice(list("ACGT"), 200)) for _ in range(2 * len(COLUMNS))]
    queries, rows = [], []
    for i, (n, strand) in enumerate((n, s) for n in COLUMNS for s in "+-"):
        ts = 7 + i
        piece = targets[i][ts:ts + n]
        queries.append("TT" + (piece if strand == "+" else PC.rc(piece)) + "G")
        rows.append((i, i, 2, ts, 2 + n, ts + n, ord(strand), 0, 0))
    o = np.array(rows, O.OVERLAP)
    cigars, edits = cm.align_overlaps(o, queries, targets)
    assert cigars == ["%dM" % n for n in COLUMNS for _ in "+-"] and not edits.any()
    got = cm.overlap_pileup(o, queries, targets)
    assert PC.same(got, OPi.overlap_pileup(o, queries, targets, OPi.of_cigars(cigars), "cigar"))
    for pile, target, row in zip(got, targets, rows):
        ts, te = row[3], row[5]
        want = np.zeros((6, 200), np.uint32)
        want[OPi.CHANNEL_OF[np.frombuffer(target.encode(), np.uint8)[ts:te]], np.arange(ts, te)] = 1
        assert np.array_equal(pile, want)  # depth 1 on [ts, te), 0 elsewhere, the channel the target's own base
    # as pairs of one set: the query's bases are supported as they are, too
    reads = targets + queries
    pairs = o.copy()
    pairs["query_read_id"] += len(targets)
    both = cm.pair_pileup(pairs, reads)
    assert PC.same(both[:len(targets)], got)
    for pile, query, n in zip(both[len(targets):], queries, (n for n in COLUMNS for _ in "+-")):
        want = np.zeros((6, len(query)), np.uint32)
        want[OPi.CHANNEL_OF[np.frombuffer(query.encode(), np.uint8)[2:2 + n]], np.arange(2, 2 + n)] = 1
        assert np.array_equal(pile, want)


def boundary_variants(t, x):
    """queries of a 150-base target `t` with runs of the letter `x`, which `t` does not hold, around column 64"""
    return [t[:63] + 2 * x + t[64:],                      # 0: t[63] is missing and a run of two stands in its place
            t[:64] + 2 * x + t[64:],                      # 1: a run in columns 64 and 65: its head is lane 0 of tile 1
            t[:63] + 3 * x + t[63:],                      # 2: a run over columns 63, 64, 65: head in lane 63, none in lane 0
            t[:62] + 2 * x + t[62:126] + x + t[126:]]     # 3: a run that ends in lane 63, and one in column 128


def test_insertion_runs_across_a_tile_boundary(cm):
    """A 150-base target without A and without equal neighbours and queries with A runs: a run's head in lane 0 of the
    second tile takes the state before it from the first tile, and a run that spans the boundary has its head in lane
    63 and no second head in lane 0. On '-' the target read is the reverse complement, so the aligner sees the same
    two sequences. The mirrored records, in which the target has the runs, do the same to the query role."""
    t = PC.unique_target(np.random.default_rng(150), 150)
    assert "A" not in t and "T" not in PC.rc(t)
    with_a, with_t = boundary_variants(t, "A"), boundary_variants(PC.rc(t), "T")
    reads = [t, PC.rc(t)] + with_a + [PC.rc(v) for v in with_t]
    rows = [(2 + i, 0, 0, 0, len(v), 150, ord("+"), 0, 0) for i, v in enumerate(with_a)]
    rows += [(2 + i, 1, 0, 0, len(v), 150, ord("-"), 0, 0) for i, v in enumerate(with_a)]
    # mirrored: t, or on '-' its reverse complement, is the query, and the runs are columns of state 2
    rows += [(0, 2 + i, 0, 0, 150, len(v), ord("+"), 0, 0) for i, v in enumerate(with_a)]
    rows += [(1, 6 + i, 0, 0, 150, len(v), ord("-"), 0, 0) for i, v in enumerate(with_t)]
    o = np.array(rows, O.OVERLAP)
    cigars, _ = cm.align_overlaps(o, reads)
    alignments = OPi.of_cigars(cigars)
    # the device's alignments do hold what the cases are for, on both strands and in both roles
    assert cigars[0:4] == cigars[4:8] and cigars[8:12] == cigars[12:16]
    assert cigars[1] == "64M2D86M" and cigars[2] == "63M3D87M" and cigars[3] == "62M2D64M1D24M"
    assert cigars[9] == "64M2I86M" and cigars[10] == "63M3I87M" and cigars[11] == "62M2I64M1I24M"
    print("t[63] missing, a run in its place:", cigars[0], cigars[8])
    for i in range(len(o)):
        one = o[i:i + 1]
        want = OPi.pair_pileup(one, reads, alignments[i:i + 1], "cigar")
        assert PC.same(cm.pair_pileup(one, reads), want), (i, cigars[i])
        target_role = OPi.pair_pileup(one, reads, alignments[i:i + 1], "cigar", roles=(False,))
        assert PC.same(cm.overlap_pileup(one, reads), target_role), (i, cigars[i])
    assert PC.same(cm.pair_pileup(o, reads), OPi.pair_pileup(o, reads, alignments, "cigar"))

    def insertions(record, read, role):
        piles = cm.overlap_pileup(o[record:record + 1], reads) if role == "target" else [
            a - b for a, b in zip(cm.pair_pileup(o[record:record + 1], reads), cm.overlap_pileup(o[record:record + 1], reads))]
        assert sum(int(p[INSERTION].sum()) for p in piles) == int(piles[read][INSERTION].sum())
        return piles[read][INSERTION].nonzero()[0].tolist()

    # on paper. The run in columns 64 and 65 counts once, behind target base 63; the one over 63 to 65 behind base 62;
    # on '-' (te = 150) those columns lie between target bases 149 - 63 and 149 - 62, and the smaller is 86
    assert insertions(1, 0, "target") == [63] and insertions(2, 0, "target") == [62] and insertions(3, 0, "target") == [61, 125]
    assert insertions(4 + 1, 1, "target") == [85] and insertions(4 + 2, 1, "target") == [86]
    # mirrored: the query's positions ascend on both strands
    assert insertions(8 + 1, 0, "query") == [63] and insertions(8 + 2, 0, "query") == [62]
    assert insertions(12 + 1, 1, "query") == [63] and insertions(12 + 3, 1, "query") == [61, 125]
    # the segment kernel walks the same columns: the records of both roles of the same 16 alignments, against the
    # CIGAR formulations of the two oracles on the device's own CIGARs, with a window cut at every lane (1), at odd
    # lanes (7) and at the tile boundary itself (64)
    for W in (1, 7, 64):
        (target_role, target_offsets, _), (query_role, query_offsets) = cm.pair_segments(o, reads, W)
        for got, offsets, from_cigar in ((target_role, target_offsets, OPo.segments_from_cigar),
                                         (query_role, query_offsets, OC.query_role_from_cigar)):
            rows = [from_cigar(i, o[i], cigars[i], W) for i in range(len(o))]
            want = np.array([r for per_record in rows for r in per_record], OC.SEGMENT).reshape(-1)
            assert got.dtype == cm.SEGMENT and got.tolist() == want.tolist(), (W, from_cigar.__name__)
            assert offsets.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist()
            assert len(got) >= len(o) * (140 // W)  # every window of a read holds an aligned column, a few of W = 1 aside


def test_every_cell_of_the_polishing_case(cm, polishing):
    reads, drafts, o, alignments = polishing
    want = OPi.overlap_pileup(o, reads, drafts, alignments, "cigar")
    timings = {}
    got = cm.overlap_pileup(o, reads, drafts, timings=timings)
    assert PC.same(got, want)
    assert [p.shape for p in got] == [(6, len(d)) for d in drafts] and all(p[c].sum() > 0 for p in got for c in range(6))
    assert got[0].base is not None and got[0].base is got[1].base  # views of the one copied buffer
    assert timings["bytes_to_host"] == o.nbytes + 24 * sum(len(d) for d in drafts)
    for pile, covered in zip(got, OPi.covering(o, drafts, False, alignments)):
        assert np.array_equal(OPi.depth(pile), covered)
    # read ids that count from 5 and from 3
    shifted = o.copy()
    shifted["query_read_id"] += 5
    shifted["target_read_id"] += 3
    assert PC.same(cm.overlap_pileup(shifted, reads, drafts, first_query_read_id=5, first_target_read_id=3), want)
    with pytest.raises(cm.MapperError):
        cm.overlap_pileup(shifted, reads, drafts, first_query_read_id=5, first_target_read_id=2)


def test_counts_do_not_depend_on_the_chunking(cm, polishing, correction):
    reads, drafts, o, _ = polishing
    for records, call in ((o, lambda r, **kw: cm.overlap_pileup(r, reads, drafts, **kw)),
                          (correction[2], lambda r, **kw: cm.pair_pileup(r, reads, **kw))):
        ql = records["query_end_position_in_read"].astype(np.int64) - records["query_start_position_in_read"]
        tl = records["target_end_position_in_read"].astype(np.int64) - records["target_start_position_in_read"]
        alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
        # a chunk counts its slices' bases four times and more (gathered, state slots, two bytes per column), so
        # within `alone` bytes so many copies of the records take more than two chunks
        copies = 2 * alone // (4 * int((ql + tl).sum())) + 1
        many = np.tile(records, copies)
        assert 4 * copies * int((ql + tl).sum()) > 2 * alone and copies <= 40
        whole = call(many, max_device_bytes=0)
        assert PC.same(call(many, max_device_bytes=alone), whole)
        assert PC.same(whole, [copies * p for p in call(records)])
        with pytest.raises(cm.MapperError, match="max_device_bytes"):
            call(many, max_device_bytes=alone - 1)


def test_every_cell_of_the_correction_case(cm, correction):
    reads, o, pairs, alignments = correction
    both = cm.pair_pileup(pairs, reads)
    assert PC.same(both, OPi.pair_pileup(pairs, reads, alignments, "cigar"))
    target_role = cm.overlap_pileup(pairs, reads, reads)
    assert PC.same(target_role, OPi.pair_pileup(pairs, reads, alignments, "cigar", roles=(False,)))
    query_role = [a - b for a, b in zip(both, target_role)]
    assert PC.same(query_role, OPi.pair_pileup(pairs, reads, alignments, "cigar", roles=(True,)))
    assert all(p[c].sum() > 0 for p in (np.concatenate(target_role, 1), np.concatenate(query_role, 1)) for c in range(6))
    for role, piles in ((False, target_role), (True, query_role)):
        for pile, covered in zip(piles, OPi.covering(pairs, reads, role, alignments)):
            assert np.array_equal(OPi.depth(pile), covered)
    shifted = pairs.copy()
    shifted["query_read_id"] += 9
    shifted["target_read_id"] += 9
    assert PC.same(cm.pair_pileup(shifted, reads, first_read_id=9), both)


def test_the_polisher_entry_points_equal_the_oracle_pipeline(cm, polishing, correction):
    from genomeworks_amd import polisher
    reads, drafts, o, _ = polishing
    kept = o[OPi.one_overlap_per_read(o)]
    assert polisher.one_overlap_per_read(o) == OPi.one_overlap_per_read(o) and len(kept) < len(o)
    want = OPi.overlap_pileup(kept, reads, drafts, by_cigar(cm, kept, reads, drafts), "cigar")
    timings = {}
    got = polisher.pileup(reads, drafts, overlaps=o, timings=timings)
    assert PC.same(got, want) and timings["pileup"] > 0
    assert PC.same(got, OPi.pileup(reads, drafts, o))  # the pinned aligner oracle gives the same alignments
    assert max(int(polisher.depth(p).max()) for p in got) <= len(reads)
    assert np.array_equal(polisher.depth(got[0]), got[0][:5].sum(0))
    # mapping first, with polish()'s defaults
    mapped = cm.map_reads_batched(reads, drafts[:1], post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0)
    assert PC.same(polisher.pileup(reads, drafts[:1]), OPi.pileup(reads, drafts[:1], mapped))
    reads, o, pairs, alignments = correction
    want = OPi.pair_pileup(pairs, reads, alignments, "cigar")
    assert PC.same(polisher.read_pileup(reads, overlaps=o), want)
    assert PC.same(want, OPi.read_pileup(reads, o))
    mapped = cm.map_reads_batched(reads, None, post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0)
    assert PC.same(polisher.read_pileup(reads), OPi.read_pileup(reads, mapped))
    # self overlaps alone: no pair, nothing counted
    same = o[o["query_read_id"] == o["target_read_id"]]
    assert len(same) == len(reads)
    got = polisher.read_pileup(reads, overlaps=same)
    assert [p.shape for p in got] == [(6, len(r)) for r in reads] and not any(p.any() for p in got)


class Pileup(C.Structure):
    """gwm_pileup of include/gwhip_mapper.h"""
    _fields_ = [("n_bases", C.c_int64), ("counts", C.c_void_p), ("stage_ms", C.c_float * 3)]


class DeviceCopies:
    """device copies of host arrays for the entry points that take device arrays, through the HIP runtime the mapper
    library itself is linked to: a symbol looked up in a library is looked up in its dependencies too"""

    def __init__(self, library):
        self.hip = library
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.held = []

    def of(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 1)) == 0
        self.held.append(p)
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0  # host to device
        return p

    def to_host(self, p, a):
        assert self.hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2) == 0  # device to host
        return a

    def free(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


def test_refusals_leave_a_zeroed_result_and_the_device_usable(cm, correction):
    from genomeworks_amd import _native
    reads, o, pairs, _ = correction
    want = cm.pair_pileup(pairs[:4], reads)
    calls = []
    for field, value in (("query_read_id", len(reads)), ("target_read_id", len(reads)),
                         ("target_end_position_in_read", 100000), ("query_end_position_in_read", 100000)):
        bad = pairs.copy()
        bad[2][field] = value
        calls.append(lambda bad=bad: cm.pair_pileup(bad, reads))
        calls.append(lambda bad=bad: cm.overlap_pileup(bad, reads, reads))
    calls.append(lambda: cm.pair_pileup(pairs, reads, max_device_bytes=-1))
    for call in calls:
        with pytest.raises(cm.MapperError):
            call()
        assert PC.same(cm.pair_pileup(pairs[:4], reads), want)
    # the kernel-level entry points over device arrays: -1, the error text, and the struct as gwm_pileup{} leaves it
    L = _native.mapper()
    L.gwm_last_error.restype = C.c_char_p
    vp, i64, i32, u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
    L.gwm_overlap_pileup.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i64, vp, C.POINTER(Pileup)]
    L.gwm_pair_pileup.argtypes = [vp, i64, vp, vp, i32, u32, i64, vp, C.POINTER(Pileup)]
    L.gwm_pileup_free.argtypes = [C.POINTER(Pileup)]
    L.gwm_pileup_free.restype = None
    device = DeviceCopies(L)
    try:
        bases, offsets = cm.pack_reads(reads)
        read_set = (device.of(bases), device.of(offsets), len(reads), 0)
        for field, value, text in (("target_read_id", len(reads), "outside the read set"),
                                   ("query_end_position_in_read", 100000, "beyond the end of its read")):
            bad = pairs[:8].copy()
            bad[5][field] = value
            d_bad = device.of(bad)
            for call in (lambda out: L.gwm_overlap_pileup(d_bad, len(bad), *read_set, *read_set, 0, None, out),
                         lambda out: L.gwm_pair_pileup(d_bad, len(bad), *read_set, 0, None, out)):
                out = Pileup(77, 0x1000, (1.0, 2.0, 3.0))
                assert call(C.byref(out)) == -1
                assert (out.n_bases, out.counts, list(out.stage_ms)) == (0, None, [0.0, 0.0, 0.0])
                assert text in L.gwm_last_error().decode()
        # and a good call through the same door: the counts of the Python interface, in channel-major planes
        out = Pileup()
        assert L.gwm_pair_pileup(device.of(pairs[:4]), 4, *read_set, 0, None, C.byref(out)) == 0
        assert out.n_bases == int(offsets[-1]) and out.counts and all(ms > 0 for ms in out.stage_ms)
        planes = device.to_host(out.counts, np.zeros((6, out.n_bases), np.uint32))
        assert np.array_equal(planes, np.concatenate(want, 1))
        L.gwm_pileup_free(C.byref(out))
        assert (out.n_bases, out.counts) == (0, None)
    finally:
        device.free()

