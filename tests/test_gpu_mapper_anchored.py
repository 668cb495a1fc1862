"""Anchored overlap alignment on the GPU, byte for byte against the oracles: the chains
of chain_overlaps(return_anchors=True) against tests/oracle_mapper_chain.py, and align_overlaps(anchors=) against
tests/oracle_mapper_anchored.py on the hand-made lists, the 16 chained records and the capacity case, under the three
aligners, at several spacings, independent of the chunking."""
import functools

import numpy as np
import pytest

import cigar_replay as R
import mapper_anchored_cases as GC
import mapper_cases as MC
import mapper_chain_cases as CC
import oracle_affine as OA
import oracle_mapper_anchored as OG
import oracle_mapper_chain as OC
import oracle_mapper_extend as OE

pytestmark = pytest.mark.gpu

K = GC.K


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


def same(a, b):
    return MC.overlap_bytes(a) == MC.overlap_bytes(b)


def check_chains(cm, anchors, kw, where):
    """chain_overlaps(return_anchors=True) on the host array: records and scores of the call without the flag, and
    the oracle's chains"""
    o, s, offsets, positions = cm.chain_overlaps(anchors, return_scores=True, return_anchors=True, **kw)
    plain, plain_scores = cm.chain_overlaps(anchors, return_scores=True, **kw)
    assert same(o, plain) and s.tobytes() == plain_scores.tobytes(), where
    ref_o, ref_s, chains = OC.chain_overlaps(anchors, with_chains=True, **kw)
    assert same(o, ref_o) and s.tobytes() == ref_s.tobytes(), where
    want_offsets, want_positions = OG.lists_of(chains, anchors)
    assert offsets.dtype == np.int64 and positions.dtype == np.uint32 and positions.shape == (int(offsets[-1]), 2), where
    assert offsets.tolist() == want_offsets.tolist(), where
    assert positions.tobytes() == want_positions.tobytes(), where
    assert np.diff(offsets).tolist() == o["num_residues"].tolist(), where
    return o, offsets, positions


@pytest.mark.parametrize("family", ["group_size_cases", "look_back_cases", "tie_cases", "extraction_cases",
                                    "orientation_cases"])
def test_chains_of_hand_built_cases(cm, family):
    kept = 0
    for name, anchors, kw in getattr(CC, family)():
        kept += len(check_chains(cm, anchors, kw, name)[0])
    assert kept > 0


def test_chains_of_interleaved_diagonals(cm):
    a = CC.interleaved_diagonals()
    o, offsets, positions = check_chains(cm, a, dict(max_chains=2), "M = 2")
    # the two chains alternate in anchor order, and each comes out whole and in order
    assert offsets.tolist() == [0, 6, 12]
    assert positions[:6, 1].tolist() == [1000 + 200 * i for i in range(6)]
    assert positions[6:, 1].tolist() == [9000 + 200 * i for i in range(6)]
    check_chains(cm, a, dict(max_chains=1), "M = 1")


def test_chains_of_many_groups(cm):
    a = CC.many_groups()
    for kw in ({}, dict(CC.KEEP_ALL, min_chain_score=0, max_chains=64)):
        o, offsets, _ = check_chains(cm, a, kw, "many groups %s" % kw)
        assert len(o) > 50
    none = cm.chain_overlaps(a[:2], return_anchors=True)
    assert len(none[0]) == 0 and none[1].tolist() == [0] and none[2].shape == (0, 2)


def test_chains_on_the_matcher_path(cm):
    reads, _, _, _ = GC.synthetic()
    with cm.Index(reads, 15, 10, True, 1.0) as index, cm.Matcher(index, index) as m:
        o, s, offsets, positions = cm.chain_overlaps(m, return_scores=True, return_anchors=True)
        plain, plain_scores = cm.chain_overlaps(m, return_scores=True)
        a = m.anchors()
    assert same(o, plain) and s.tobytes() == plain_scores.tobytes()
    o2, offsets2, positions2 = check_chains(cm, a, {}, "synthetic reads")
    assert same(o, o2) and offsets.tolist() == offsets2.tolist() and positions.tobytes() == positions2.tobytes()
    assert len(o) > 300


@functools.lru_cache(maxsize=None)
def hand_made_want(S, scoring):
    queries, targets, overlaps, anchors, _ = GC.hand_made()
    offsets, positions = GC.lists(anchors)
    return OG.cigars(OG.alignments(overlaps, queries, targets, offsets, positions, K, S, scoring))


def check_alignment(cm, overlaps, queries, targets, per_record, S, scoring, where, **kw):
    offsets, positions = GC.lists(per_record) if isinstance(per_record, list) else per_record
    want = OG.cigars(OG.alignments(overlaps, queries, targets, offsets, positions, K, S, scoring))
    cigars, edits = cm.align_overlaps(overlaps, queries, targets, scoring=scoring, anchors=(offsets, positions),
                                      anchor_kmer_size=K, anchor_spacing=S, **kw)
    assert cigars == want[0], where
    assert edits.tolist() == want[1], where
    return cigars, edits


@pytest.mark.parametrize("scoring", GC.SCORINGS)
@pytest.mark.parametrize("S", (1, 64, 256))
def test_hand_made_lists(cm, S, scoring):
    queries, targets, overlaps, anchors, what = GC.hand_made()
    want = hand_made_want(S, scoring)
    offsets, positions = GC.lists(anchors)
    timings = {}
    cigars, edits = cm.align_overlaps(overlaps, queries, targets, scoring=scoring, anchors=(offsets, positions),
                                      anchor_kmer_size=K, anchor_spacing=S, timings=timings)
    for k, name in enumerate(what):
        assert cigars[k] == want[0][k] and edits[k] == want[1][k], (name, S, scoring)
    assert {chr(s) for s in overlaps["relative_strand"]} == {"+", "-"} and timings["align"] > 0
    assert all(c for c, name in zip(cigars, what) if name != "both empty")
    # a record without valid anchors is the alignment of the call without anchors, byte for byte
    plain, plain_edits = cm.align_overlaps(overlaps, queries, targets, scoring=scoring)
    for k, name in enumerate(what):
        if name in ("no anchors", "n = 0", "m = 0", "both empty") and scoring is not None:
            assert cigars[k] == plain[k] and edits[k] == plain_edits[k], name
    if S == 1:
        assert len(OG.plan(overlaps, offsets, positions, K, 1)[-1]) > 128  # the stitch crosses two blocks of 64 pieces


@pytest.mark.parametrize("scoring", GC.SCORINGS)
def test_sixteen_records(cm, scoring):
    reads, overlaps, offsets, positions = GC.sixteen_records()
    for S in (64, 256):
        check_alignment(cm, overlaps, reads, None, (offsets, positions), S, scoring, (S, scoring))


def test_piece_counts_at_the_edges_of_the_scan(cm):
    queries, targets, overlaps, per_record = GC.piece_count_records((1, 63, 64, 65, 129))
    offsets, positions = GC.lists(per_record)
    assert [len(p) for p in OG.plan(overlaps, offsets, positions, K, 1)] == [1, 63, 64, 65, 129]
    for scoring in (None, (4, 6, 2, 16)):
        check_alignment(cm, overlaps, queries, targets, per_record, 1, scoring, scoring)


def test_slots_of_a_few_bytes(cm):
    queries, targets, overlaps, per_record = GC.small_slot_records()
    offsets, positions = GC.lists(per_record)
    slots = {dn + dm for record in OG.plan(overlaps, offsets, positions, K, 1) for _, _, dn, dm in record}
    assert {1, 2, 3, 4, 5} <= slots
    for scoring in GC.SCORINGS:
        check_alignment(cm, overlaps, queries, targets, per_record, 1, scoring, scoring)


def capacity_call():
    """three records: the five deletions, one deletion of 2 100 bases, the five deletions again"""
    q5, target, rec5, rows5 = GC.capacity_case(5)
    q1, target1, rec1, rows1 = GC.capacity_case(1, 2100)
    assert target1 == target
    rec1 = rec1.copy()
    rec1["query_read_id"] = 1
    return [q5, q1], [target], np.array([rec5, rec1, rec5], GC.OVERLAP), [rows5, rows1, rows5]


def test_capacity_case_end_to_end(cm):
    query, target, rec, rows = GC.capacity_case(5)
    overlaps = np.array([rec], cm.OVERLAP)
    scoring = (4, 6, 2, 16)
    cigars, edits = cm.align_overlaps(overlaps, [query], [target], scoring=scoring)
    assert cigars == [""] and edits.tolist() == [-1]  # W = 2283 diagonals: out of the aligner's reach
    cigars, edits = check_alignment(cm, overlaps, [query], [target], [rows], 256, scoring, "five deletions")
    assert cigars[0].count("450I") == 5 and edits.tolist() == [5 * 450]
    R.replay_paf(["q", str(len(query)), "0", str(len(query)), "+", "t", str(len(target)), "0", str(len(target)), "0", "0",
                  "255", "cg:Z:" + cigars[0]], {"q": query}, {"t": target})
    # two pieces: three deletions are beyond 1024 diagonals, two are not
    two = (6, 4, 3, 24, 2, 16)
    for deletions, whole in ((2, True), (3, False)):
        query, target, rec, rows = GC.capacity_case(deletions)
        overlaps = np.array([rec], cm.OVERLAP)
        assert (cm.align_overlaps(overlaps, [query], [target], scoring=two)[0] != [""]) == whole
        cigars, _ = check_alignment(cm, overlaps, [query], [target], [rows], 256, two, deletions)
        assert cigars[0].count("450I") == deletions


def test_a_piece_without_a_result_leaves_its_record_without_one(cm):
    queries, targets, overlaps, per_record = capacity_call()
    cigars, edits = check_alignment(cm, overlaps, queries, targets, per_record, 256, (4, 6, 2, 16), "middle record")
    assert cigars[1] == "" and edits.tolist()[1] == -1 and cigars[0] == cigars[2] != ""
    # the default aligner has no band: it aligns the long deletion too
    cigars, edits = check_alignment(cm, overlaps, queries, targets, per_record, 256, None, "default aligner")
    assert all(cigars)


@pytest.mark.parametrize("scoring", (None, (4, 6, 2, 16)))
def test_chunking_does_not_change_the_result(cm, scoring):
    reads, overlaps, offsets, positions = GC.sixteen_records()
    plans = OG.plan(overlaps, offsets, positions, K, 256)
    longest = max(dn for record in plans for _, _, dn, _ in record)
    needs = [cm.align_bytes_needed_anchored([(dn, dm) for _, _, dn, dm in record], scoring, longest) for record in plans]
    anchors = (offsets, positions)
    whole, whole_edits = cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=anchors)
    # one record per chunk: the largest single need admits no two records
    lone, lone_edits = cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=anchors, max_device_bytes=max(needs))
    assert lone == whole and lone_edits.tobytes() == whole_edits.tobytes()
    # several chunks of several records
    some, some_edits = cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=anchors, max_device_bytes=sum(needs) // 4)
    assert some == whole and some_edits.tobytes() == whole_edits.tobytes()
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=anchors, max_device_bytes=max(needs) - 1)
    # and the next call is whole
    again, _ = cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=anchors)
    assert again == whole


def test_no_anchors_is_the_call_without_the_argument(cm):
    reads, overlaps, _, _ = GC.sixteen_records()
    for scoring in GC.SCORINGS:
        plain, plain_edits = cm.align_overlaps(overlaps, reads, scoring=scoring)
        none, none_edits = cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=None)
        assert none == plain and none_edits.tobytes() == plain_edits.tobytes()
        # empty lists: every record is one piece
        empty = (np.zeros(len(overlaps) + 1, np.int64), np.zeros((0, 2), np.uint32))
        got, got_edits = cm.align_overlaps(overlaps, reads, scoring=scoring, anchors=empty)
        assert got == plain and got_edits.tobytes() == plain_edits.tobytes()


def test_a_list_that_is_not_monotone_names_its_record(cm):
    queries, targets, overlaps, anchors = GC.not_monotone()
    with pytest.raises(cm.MapperError, match="overlap 2 "):
        cm.align_overlaps(overlaps, queries, targets, anchors=GC.lists(anchors), anchor_spacing=64)
    good = GC.hand_made()[3]
    cigars, _ = cm.align_overlaps(overlaps, queries, targets, anchors=GC.lists(good), anchor_spacing=64)
    assert cigars == hand_made_want(64, None)[0]
    assert cm.align_overlaps(overlaps[:0], queries, targets, anchors=(np.zeros(1, np.int64), np.zeros((0, 2), np.uint32)))[0] == []


def test_extended_overlaps_keep_their_anchors(cm):
    reads, overlaps, offsets, positions = GC.sixteen_records()
    moved, extensions, _ = cm.extend_overlaps(overlaps, reads)
    assert same(moved, OE.extend_overlaps(overlaps, reads, reads)[0]) and int((extensions > 0).sum()) > 8
    check_alignment(cm, moved, reads, None, (offsets, positions), 256, (4, 6, 2, 16), "extended")
    # the ends moved away from the chains' first and last anchors, which now count
    before = sum(len(p) for p in OG.plan(overlaps, offsets, positions, K, 1))
    assert sum(len(p) for p in OG.plan(moved, offsets, positions, K, 1)) > before


def test_map_reads_hands_the_anchors_to_align_overlaps(cm):
    reads, _, _, _ = GC.synthetic()
    o, offsets, positions = cm.map_reads(reads, filtering_parameter=1.0, overlapper="chained", return_anchors=True)
    assert same(o, cm.map_reads(reads, filtering_parameter=1.0, overlapper="chained")) and len(o) > 300
    assert np.diff(offsets).tolist() == o["num_residues"].tolist()
    cigars, edits = cm.align_overlaps(o, reads, scoring=(4, 6, 2, 16), anchors=(offsets, positions))
    names, lengths = ["read_%d" % i for i in range(len(reads))], [len(r) for r in reads]
    by_name = dict(zip(names, reads))
    lines = cm.format_paf(o, names, lengths, names, lengths, 15, cigars=cigars).splitlines()
    assert len(lines) == len(o)
    for line, e in zip(lines, edits):
        assert R.replay_paf(line, by_name, by_name).edits == e, line
    with pytest.raises(ValueError):
        cm.map_reads(reads, return_anchors=True)
