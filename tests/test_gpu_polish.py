"""Polishing on the device (tests/oracle_polish.py is the oracle): the segments of aligned overlaps against records
worked out on paper and against the oracle for every record of a mapped case, their independence of the chunking, the
window sequences byte for byte, polish() against the oracle pipeline, and the refusals."""
import numpy as np
import pytest

import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_polish as OPo

pytestmark = pytest.mark.gpu

WINDOW_LENGTHS = (7, 64, 200, 4096)


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def small(cm):
    """the small case against a 3 % draft: reads, genome, draft, the device's overlaps (fused records and rescued ends
    included) and the oracle's alignment of each, computed once"""
    reads, genome = OPo.small_case()
    draft = OPo.draft_of(genome, 0.03, OPo.SMALL["seed"])
    o = cm.map_reads_batched(reads, [draft], rescue_overlap_ends=True, **OPo.MAPPING)
    assert len(o) >= 20 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    alignments = OA.alignments(o, reads, [draft])
    assert all(384 < len(a["states"]) < 1280 for a in alignments)  # 7 to 20 tiles of 64 columns each
    return reads, genome, draft, o, alignments


def rc(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def paper_cases():
    """(queries, targets, [(W, query, target, qs, qe, ts, te, strand, [(window, target_first, target_last,
    query_begin, query_end), ...]), ...])"""
    rng = np.random.default_rng(2024)
    t0, t2 = ("".join(rng.choice(list("ACGT"), n)) for n in (100, 200))
    # a target whose bases 32..47 are missing from the query. They are the only A's of the pair, so no column can
    # align them without a mismatch: the 16 gap columns of the optimal alignment are exactly these
    t1 = "".join(rng.choice(list("CGT"), 96))
    t1 = t1[:32] + "A" * 16 + t1[48:]
    q2 = t1[:32] + t1[48:]
    targets = [t0, t1, t2, "ACGTACGTAC"]
    queries = [t0[10:90], rc(t0[10:90]), q2, rc(q2), t2[64:128], t2[0:128], rc(t2[64:192]), "TTTTTGCCCC"]
    cases = [
        # an exact copy of T[10:90], W = 16
        (16, 0, 0, 0, 80, 10, 90, "+", [(0, 10, 15, 0, 6), (1, 16, 31, 6, 22), (2, 32, 47, 22, 38), (3, 48, 63, 38, 54),
                                       (4, 64, 79, 54, 70), (5, 80, 89, 70, 80)]),
        (16, 1, 0, 0, 80, 10, 90, "-", [(0, 10, 15, 74, 80), (1, 16, 31, 58, 74), (2, 32, 47, 42, 58),
                                       (3, 48, 63, 26, 42), (4, 64, 79, 10, 26), (5, 80, 89, 0, 10)]),
        # window 2 of the target is missing from the query: no record for it
        (16, 2, 1, 0, 80, 0, 96, "+", [(0, 0, 15, 0, 16), (1, 16, 31, 16, 32), (3, 48, 63, 32, 48), (4, 64, 79, 48, 64),
                                      (5, 80, 95, 64, 80)]),
        (16, 3, 1, 0, 80, 0, 96, "-", [(0, 0, 15, 64, 80), (1, 16, 31, 48, 64), (3, 48, 63, 32, 48), (4, 64, 79, 16, 32),
                                      (5, 80, 95, 0, 16)]),
        # exactly one tile, and exactly two with the window boundary between lane 63 of the first and lane 0 of the second
        (64, 4, 2, 0, 64, 64, 128, "+", [(1, 64, 127, 0, 64)]),
        (32, 4, 2, 0, 64, 64, 128, "+", [(2, 64, 95, 0, 32), (3, 96, 127, 32, 64)]),
        (64, 5, 2, 0, 128, 0, 128, "+", [(0, 0, 63, 0, 64), (1, 64, 127, 64, 128)]),
        (64, 6, 2, 0, 128, 64, 192, "-", [(1, 64, 127, 64, 128), (2, 128, 191, 0, 64)]),
        # one column: a match, and a mismatch, which is an aligned column as well
        (4, 7, 3, 5, 6, 2, 3, "+", [(0, 2, 2, 5, 6)]),
        (4, 7, 3, 5, 6, 2, 3, "-", [(0, 2, 2, 5, 6)]),
        (4, 7, 3, 0, 1, 9, 10, "+", [(2, 9, 9, 0, 1)]),
        # two empty slices: nothing
        (4, 7, 3, 3, 3, 4, 4, "+", []),
        (16, 0, 0, 80, 80, 0, 0, "-", []),
    ]
    return queries, targets, cases


def paper_call(W):
    """(queries, targets, overlaps, expected SEGMENT array, expected offsets) of the paper cases with window length W"""
    queries, targets, cases = paper_cases()
    rows, want, offsets = [], [], [0]
    for w, q, t, qs, qe, ts, te, strand, records in cases:
        if w != W:
            continue
        want += [(len(rows),) + r for r in records]
        rows.append((q, t, qs, ts, qe, te, ord(strand), 0, 0))
        offsets.append(len(want))
    return queries, targets, np.array(rows, O.OVERLAP), np.array(want, OPo.SEGMENT).reshape(-1), offsets


@pytest.mark.parametrize("W", [4, 16, 32, 64])
def test_segments_on_paper(cm, W):
    queries, targets, o, want, offsets = paper_call(W)
    assert len(o) >= 1
    timings = {}
    segments, segment_offsets, edits = cm.window_segments(o, queries, targets, W, timings=timings)
    assert segments.dtype == cm.SEGMENT and segments.tolist() == want.tolist()
    assert segment_offsets.dtype == np.int64 and segment_offsets.tolist() == offsets
    ref = OPo.segments(o, queries, targets, W)
    assert ref[0].tolist() == want.tolist() and edits.tolist() == ref[2].tolist()  # the paper and the oracle agree
    if W == 16:
        assert edits.tolist() == [0, 0, 16, 16, 0]
    if W == 4:
        assert edits.tolist() == [0, 1, 1, 0]  # G on G; G on the complement of G; T on C
    assert all(timings[k] > 0 for k in ("gather", "align", "segments"))


@pytest.mark.parametrize("W", WINDOW_LENGTHS)
def test_every_record_of_the_small_case_equals_the_oracle(cm, small, W):
    reads, _, draft, o, alignments = small
    want = OPo.segments(o, reads, [draft], W, alignments)
    got = cm.window_segments(o, reads, [draft], W)
    assert got[0].tolist() == want[0].tolist() and len(got[0]) >= len(o)
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    if W == 4096:
        assert got[0]["overlap"].tolist() == list(range(len(o)))  # one window per overlap
    if W == 7:  # a window boundary at every lane position
        cuts = {(int(s["target_first"]) - int(o[s["overlap"]]["target_start_position_in_read"])) % 64 for s in got[0]}
        assert len(cuts) >= 60


def test_records_do_not_depend_on_the_chunking(cm, small):
    reads, _, draft, o, _ = small
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
    whole = cm.window_segments(o, reads, [draft], 64, max_device_bytes=0)
    small_chunks = cm.window_segments(o, reads, [draft], 64, max_device_bytes=alone)
    for a, b in zip(whole, small_chunks):
        assert a.tolist() == b.tolist()
    assert whole[2].tolist() == cm.align_overlaps(o, reads, [draft])[1].tolist()
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.window_segments(o, reads, [draft], 64, max_device_bytes=alone - 1)


def test_window_sequences_equal_the_oracle(cm, small):
    reads, _, draft, o, _ = small
    # N and lower-case bytes in the middle of every read: inside layers of both strands
    marked = []
    for r in reads:
        at = len(r) // 2
        marked.append(r[:at] + "NN" + r[at + 2:at + 10] + r[at + 10:at + 40].lower() + r[at + 40:])
    assert all(len(a) == len(b) for a, b in zip(marked, reads))
    alignments = OA.alignments(o, marked, [draft])
    for W, depth in ((200, 30), (200, 3), (64, 3), (7, 30), (4096, 30)):
        want = OPo.windows(o, marked, [draft], W, depth, alignments)
        timings = {}
        got = cm.overlap_windows(o, marked, [draft], W, depth, timings=timings)
        assert got == want, (W, depth)
        assert [(t, k) for t, k, _ in got] == [(0, k) for k in range((len(draft) + W - 1) // W)]
        assert b"".join(seqs[0] for _, _, seqs in got) == draft.encode()
        layers = [len(seqs) - 1 for _, _, seqs in got]
        if (W, depth) == (200, 30):
            assert max(layers) > 3
            spanning = [s for _, _, seqs in got for s in seqs[1:]]
            assert any(b"N" in s for s in spanning) and any(s != s.upper() for s in spanning)
            assert timings["window_gather"] > 0 and timings["window_bases"] == sum(len(s) for _, _, q in got for s in q)
        if depth == 3:
            assert max(layers) == 3
    # '-' layers really are among them: the plan marks them reversed
    segs = OPo.segments(o, marked, [draft], 200, alignments)[0]
    plan, _ = OPo.select_layers(segs, o, [len(draft)], 200, 30)
    assert any(p[0] == 0 and p[4] == 1 for p in plan) and any(p[0] == 0 and p[4] == 0 for p in plan)


def as_rows(report):
    return [(r["target_read"], r["window"], r["layers"], r["status"], r["backbone_kept"]) for r in report]


def test_polish_equals_the_oracle_pipeline_and_improves_the_draft(cm, small):
    from genomeworks_amd import polisher
    reads, genome, draft, o, alignments = small
    want, want_report = OPo.polish(reads, [draft], o, 200, 15, 64, alignments=alignments)
    before, after = OPo.edit_distance(draft, genome), OPo.edit_distance(want[0], genome)
    timings = {}
    got, report = polisher.polish(reads, [draft], overlaps=o, window_length=200, max_depth=15, band_width=64,
                                  timings=timings, poa_memory_per_device=1 << 30)
    assert got == want and as_rows(report) == want_report
    assert after < before and OPo.edit_distance(got[0], genome) < before
    assert sum(1 for r in report if not r["backbone_kept"]) >= 3 and report[0]["backbone_kept"]
    assert all(timings[k] > 0 for k in ("gather", "align", "segments", "window_gather", "poa_seconds", "bytes_to_host"))
    # mapping first: the same overlaps, so the same answer
    mapped, mapped_report = polisher.polish(reads, [draft], window_length=200, max_depth=15, band_width=64,
                                            poa_memory_per_device=1 << 30, **OPo.MAPPING)
    assert mapped == want and as_rows(mapped_report) == want_report
    # polish()'s own mapping defaults find these overlaps too (the frequency filter is off), and may be overridden
    default, _ = polisher.polish(reads, [draft], window_length=200, max_depth=15, band_width=64,
                                 poa_memory_per_device=1 << 30, rescue_overlap_ends=True)
    assert default == want


def test_polish_with_the_fused_records_of_post_processing(cm, small):
    """every overlap cut into two neighbours 10 bases apart: post-processing appends their fusion, which speaks for
    the read in place of its halves"""
    from genomeworks_amd import polisher
    reads, genome, draft, o, _ = small
    halves = np.repeat(o, 2)
    for i, x in enumerate(o):
        qs, qe = int(x["query_start_position_in_read"]), int(x["query_end_position_in_read"])
        ts, te = int(x["target_start_position_in_read"]), int(x["target_end_position_in_read"])
        qm, half = qs + (qe - qs) // 2, (te - ts) // 2
        a, b = halves[2 * i], halves[2 * i + 1]
        a["query_end_position_in_read"], b["query_start_position_in_read"] = qm, qm + 10
        if x["relative_strand"] == ord("+"):
            a["target_end_position_in_read"], b["target_start_position_in_read"] = ts + half, ts + half + 10
        else:
            a["target_start_position_in_read"], b["target_end_position_in_read"] = te - half, te - half - 10
    given = cm.post_process_overlaps(halves)
    assert len(given) == 3 * len(o)
    fused = given[2 * len(o):]
    for name in ("query_start_position_in_read", "query_end_position_in_read", "target_start_position_in_read",
                 "target_end_position_in_read", "relative_strand", "query_read_id"):
        assert fused[name].tolist() == o[name].tolist(), name
    want, want_report = OPo.polish(reads, [draft], given, 200, 15, 64)
    got, report = polisher.polish(reads, [draft], overlaps=given, window_length=200, max_depth=15, band_width=64,
                                  poa_memory_per_device=1 << 30)
    assert got == want and as_rows(report) == want_report
    assert OPo.edit_distance(got[0], genome) < OPo.edit_distance(draft, genome)
    # the halves alone span fewer windows: the fused records made the difference
    assert sum(r[2] for r in want_report) > sum(r[2] for r in OPo.polish(reads, [draft], halves, 200, 15, 64)[1])


def test_refusals_leave_the_device_usable(cm, small):
    reads, _, draft, o, _ = small
    # the capacity of a call is its longest query slice, so the first four overlaps are aligned as a call of their own
    want = OPo.segments(o[:4], reads, [draft], 64)[0].tolist()
    calls = []
    calls.append(lambda: cm.window_segments(o, reads, [draft], 0))
    calls.append(lambda: cm.overlap_windows(o, reads, [draft], 0))
    calls.append(lambda: cm.overlap_windows(o, reads, [draft], 64, -1))
    for field, value in (("query_read_id", len(reads)), ("target_read_id", 1),
                         ("target_end_position_in_read", len(draft) + 1),
                         ("query_end_position_in_read", 100000)):
        bad = o.copy()
        bad[2][field] = value
        calls.append(lambda bad=bad: cm.window_segments(bad, reads, [draft], 64))
        calls.append(lambda bad=bad: cm.overlap_windows(bad, reads, [draft], 64))
    for call in calls:
        with pytest.raises(cm.MapperError):
            call()
        assert cm.window_segments(o[:4], reads, [draft], 64)[0].tolist() == want
    # no overlaps: every window is its backbone
    empty = cm.overlap_windows(np.zeros(0, O.OVERLAP), reads, [draft], 500)
    assert [(t, k, len(s)) for t, k, s in empty] == [(0, k, 1) for k in range(3)]
    assert b"".join(s[0] for _, _, s in empty) == draft.encode()
