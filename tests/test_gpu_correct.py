"""Read correction on the device (tests/oracle_correct.py is the oracle): the query-role records of aligned pairs
against records worked out on paper and against the oracle for every record of a set mapped against itself, the
target-role records against window_segments byte for byte, independence of the chunking, the window sequences byte for
byte, correct_reads() against the oracle pipeline, and the refusals."""
import numpy as np
import pytest

import oracle_correct as OC
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
    """the small case mapped against itself as two sets on the device -- self overlaps and both directions of a pair
    are among the records --: reads, the records, their pairs and the oracle's alignment of each pair, computed once"""
    reads, _ = OPo.small_case()
    o = cm.map_reads_batched(reads, reads, rescue_overlap_ends=True, **OPo.MAPPING)
    ids = list(zip(o["query_read_id"].tolist(), o["target_read_id"].tolist()))
    assert any(a == b for a, b in ids) and any((b, a) in set(ids) for a, b in ids if a < b)
    pairs = o[cm.select_pairs(o)]
    assert len(pairs) >= 100 and {chr(s) for s in pairs["relative_strand"]} == {"+", "-"}
    alignments = OA.alignments(pairs, reads)
    assert all(256 < len(a["states"]) <= 1280 for a in alignments)  # 5 to 20 tiles of 64 columns each
    return reads, o, pairs, alignments


def rc(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def paper_cases():
    """(reads, [(W, query, target, qs, qe, ts, te, strand, [(window, target_first, target_last, query_begin,
    query_end), ...]), ...]): the query-role records, so target_* are query positions and query_* target positions"""
    rng = np.random.default_rng(2025)
    t0, t2 = ("".join(rng.choice(list("ACGT"), n)) for n in (100, 200))
    # a query whose bases 32..47 are missing from the target. They are the only A's of the pair, so no column can align
    # them without a mismatch: the 16 query-only columns of the optimal alignment are exactly these, and they are the
    # whole of the query's window 2
    x = "".join(rng.choice(list("CGT"), 80))
    q1 = x[:32] + "A" * 16 + x[32:]
    reads = [t0, t0[10:90], rc(t0[10:90]), q1, x, rc(x), t2, t2[64:192], rc(t2[64:192]), t2[64:128], "ACGTACGTAC",
             "TTTTTGCCCC"]
    cases = [
        # an exact copy of T[10:90], W = 16
        (16, 1, 0, 0, 80, 10, 90, "+", [(0, 0, 15, 10, 26), (1, 16, 31, 26, 42), (2, 32, 47, 42, 58), (3, 48, 63, 58, 74),
                                       (4, 64, 79, 74, 90)]),
        (16, 2, 0, 0, 80, 10, 90, "-", [(0, 0, 15, 74, 90), (1, 16, 31, 58, 74), (2, 32, 47, 42, 58), (3, 48, 63, 26, 42),
                                       (4, 64, 79, 10, 26)]),
        # a query-only run swallows window 2 of the query: no record for it
        (16, 3, 4, 0, 96, 0, 80, "+", [(0, 0, 15, 0, 16), (1, 16, 31, 16, 32), (3, 48, 63, 32, 48), (4, 64, 79, 48, 64),
                                      (5, 80, 95, 64, 80)]),
        (16, 3, 5, 0, 96, 0, 80, "-", [(0, 0, 15, 64, 80), (1, 16, 31, 48, 64), (3, 48, 63, 32, 48), (4, 64, 79, 16, 32),
                                      (5, 80, 95, 0, 16)]),
        # exactly one tile, and exactly two with the query's window boundary between lane 63 of the first and lane 0 of
        # the second
        (64, 9, 6, 0, 64, 64, 128, "+", [(0, 0, 63, 64, 128)]),
        (32, 9, 6, 0, 64, 64, 128, "+", [(0, 0, 31, 64, 96), (1, 32, 63, 96, 128)]),
        (64, 7, 6, 0, 128, 64, 192, "+", [(0, 0, 63, 64, 128), (1, 64, 127, 128, 192)]),
        (64, 8, 6, 0, 128, 64, 192, "-", [(0, 0, 63, 128, 192), (1, 64, 127, 64, 128)]),
        # ... and with the query slice starting in the middle of a window: tiles and windows out of step
        (64, 7, 6, 32, 128, 96, 192, "+", [(0, 32, 63, 96, 128), (1, 64, 127, 128, 192)]),
        # one column: a match, and a mismatch, which is an aligned column as well
        (4, 11, 10, 5, 6, 2, 3, "+", [(1, 5, 5, 2, 3)]),
        (4, 11, 10, 5, 6, 2, 3, "-", [(1, 5, 5, 2, 3)]),
        (4, 11, 10, 0, 1, 9, 10, "+", [(0, 0, 0, 9, 10)]),
        # two empty slices: nothing
        (4, 11, 10, 3, 3, 4, 4, "+", []),
        (16, 1, 0, 80, 80, 0, 0, "-", []),
    ]
    return reads, cases


def paper_call(W):
    """(reads, pairs, expected query-role SEGMENT array, expected offsets) of the paper cases with window length W"""
    reads, cases = paper_cases()
    rows, want, offsets = [], [], [0]
    for w, q, t, qs, qe, ts, te, strand, records in cases:
        if w != W:
            continue
        want += [(len(rows),) + r for r in records]
        rows.append((q, t, qs, ts, qe, te, ord(strand), 0, 0))
        offsets.append(len(want))
    return reads, np.array(rows, O.OVERLAP), np.array(want, OC.SEGMENT).reshape(-1), offsets


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("W", [4, 16, 32, 64])
def test_query_role_records_on_paper(cm, W):
    reads, pairs, want, offsets = paper_call(W)
    assert len(pairs) >= 1
    timings = {}
    target_role, (query_role, query_role_offsets) = cm.pair_segments(pairs, reads, W, timings=timings)
    assert query_role.dtype == cm.SEGMENT and query_role.tolist() == want.tolist()
    assert query_role_offsets.dtype == np.int64 and query_role_offsets.tolist() == offsets
    ref_target, (ref_query, ref_offsets) = OC.pair_segments(pairs, reads, W)
    assert ref_query.tolist() == want.tolist() and ref_offsets.tolist() == offsets  # the paper and the oracle agree
    # the target role is what window_segments gives, the edit distances included
    for got, alone in zip(target_role, cm.window_segments(pairs, reads, None, W)):
        assert same_bytes(got, alone)
    assert target_role[2].tolist() == ref_target[2].tolist()
    if W == 16:
        assert target_role[2].tolist() == [0, 0, 16, 16, 0]
    assert all(timings[k] > 0 for k in ("gather", "align", "segments", "query_role_segments"))
    assert timings["pairs"] == timings["overlaps_in"] == len(pairs)


@pytest.mark.parametrize("W", WINDOW_LENGTHS)
def test_every_record_of_the_small_case_equals_the_oracle(cm, small, W):
    reads, _, pairs, alignments = small
    want_target, (want, want_offsets) = OC.pair_segments(pairs, reads, W, alignments)
    got_target, (got, got_offsets) = cm.pair_segments(pairs, reads, W)
    assert got.tolist() == want.tolist() and len(got) >= len(pairs)
    assert got_offsets.tolist() == want_offsets.tolist()
    for a, b, c in zip(got_target, cm.window_segments(pairs, reads, None, W), want_target):
        assert same_bytes(a, b) and a.tolist() == c.tolist()
    if W == 4096:
        assert got["overlap"].tolist() == list(range(len(pairs)))  # one window per pair
    if W == 7:  # a window boundary at every lane position
        cuts = {(int(s["target_first"]) - int(pairs[s["overlap"]]["query_start_position_in_read"])) % 64 for s in got}
        assert len(cuts) >= 60


def test_records_do_not_depend_on_the_chunking(cm, small):
    reads, _, pairs, _ = small
    many = np.tile(pairs, 6)
    ql = many["query_end_position_in_read"].astype(np.int64) - many["query_start_position_in_read"]
    tl = many["target_end_position_in_read"].astype(np.int64) - many["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
    # a chunk counts its slices' bases four times and more (gathered, state slots, two bytes per column), so within
    # `alone` bytes the pairs take more than two chunks
    assert 4 * int((ql + tl).sum()) > 2 * alone
    whole = cm.pair_segments(many, reads, 64, max_device_bytes=0)
    small_chunks = cm.pair_segments(many, reads, 64, max_device_bytes=alone)
    for a, b in zip(whole[0] + whole[1], small_chunks[0] + small_chunks[1]):
        assert same_bytes(a, b)
    once = cm.pair_segments(pairs, reads, 64)
    n = len(once[1][0])
    assert n > 0 and same_bytes(whole[1][0][:n], once[1][0]) and len(whole[1][0]) == 6 * n
    assert whole[0][2][:len(pairs)].tolist() == cm.align_overlaps(pairs, reads)[1].tolist()
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.pair_segments(many, reads, 64, max_device_bytes=alone - 1)


def test_window_sequences_equal_the_oracle(cm, small):
    reads, o, pairs, _ = small
    # N and lower-case bytes in the middle of every read: inside layers of both strands and both roles
    marked = []
    for r in reads:
        at = len(r) // 2
        marked.append(r[:at] + "NN" + r[at + 2:at + 10] + r[at + 10:at + 40].lower() + r[at + 40:])
    assert all(len(a) == len(b) for a, b in zip(marked, reads))
    alignments = OA.alignments(pairs, marked)
    for W, depth in ((200, 30), (200, 3), (64, 3), (7, 30), (4096, 30)):
        want = OC.windows(o, marked, W, depth, alignments)
        timings = {}
        got = cm.correction_windows(o, marked, W, depth, timings=timings)
        assert got == want, (W, depth)
        assert [(r, k) for r, k, _ in got] == [(i, k) for i, r in enumerate(reads) for k in range((len(r) + W - 1) // W)]
        assert b"".join(seqs[0] for _, _, seqs in got) == "".join(marked).encode()
        layers = [len(seqs) - 1 for _, _, seqs in got]
        assert (timings["overlaps_in"], timings["pairs"]) == (len(o), len(pairs))
        if (W, depth) == (200, 30):
            assert max(layers) > 3
            spanning = [s for _, _, seqs in got for s in seqs[1:]]
            assert any(b"N" in s for s in spanning) and any(s != s.upper() for s in spanning)
            assert timings["window_gather"] > 0 and timings["window_bases"] == sum(len(s) for _, _, q in got for s in q)
        if depth == 3:
            assert max(layers) == 3
    # layers of both roles and both strands really are among them
    (t, _, _), (q, _) = OC.pair_segments(pairs, marked, 200, alignments)
    lengths = [len(r) for r in marked]
    for role, (a, b) in enumerate(((t, q[:0]), (t[:0], q))):
        plan, table = OC.select_correction_layers(a, b, pairs, lengths, 200, 30)
        layers = [p for _, _, first, n in table for p in plan[first + 1:first + n]]
        assert any(p[4] == 1 for p in layers) and any(p[4] == 0 for p in layers), role


def as_rows(report):
    return [(r["target_read"], r["window"], r["layers"], r["status"], r["backbone_kept"]) for r in report]


def test_correct_reads_equals_the_oracle_pipeline(cm, small):
    from genomeworks_amd import polisher
    reads, o, pairs, alignments = small
    want, want_report = OC.correct(reads, o, 200, 15, 64, alignments=alignments)
    timings = {}
    got, report = polisher.correct_reads(reads, overlaps=o, window_length=200, max_depth=15, band_width=64,
                                         timings=timings, poa_memory_per_device=1 << 30)
    assert got == want and as_rows(report) == want_report
    assert sum(1 for r in report if not r["backbone_kept"]) >= len(reads) and got != reads
    assert all(timings[k] > 0 for k in ("gather", "align", "segments", "query_role_segments", "window_gather",
                                        "poa_seconds", "bytes_to_host"))
    assert (timings["overlaps_in"], timings["pairs"]) == (len(o), len(pairs))
    # mapping first: the set against itself as one set, with polish()'s defaults
    mapped = cm.map_reads_batched(reads, None, post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0)
    want, want_report = OC.correct(reads, mapped, 200, 15, 64)
    got, report = polisher.correct_reads(reads, window_length=200, max_depth=15, band_width=64,
                                         poa_memory_per_device=1 << 30)
    assert got == want and as_rows(report) == want_report


def test_self_overlaps_alone_return_the_reads(cm, small):
    from genomeworks_amd import polisher
    reads, o, _, _ = small
    same = o[o["query_read_id"] == o["target_read_id"]]
    assert len(same) == len(reads) and len(cm.select_pairs(same)) == 0
    timings = {}
    got, report = polisher.correct_reads(reads, overlaps=same, window_length=200, max_depth=15, band_width=64,
                                         timings=timings, poa_memory_per_device=1 << 30)
    assert got == reads and all(r["backbone_kept"] and r["layers"] == 0 and r["status"] is None for r in report)
    assert (timings["overlaps_in"], timings["pairs"]) == (len(same), 0)


def test_refusals_leave_the_device_usable(cm, small):
    reads, o, pairs, _ = small
    want = OC.pair_segments(pairs[:4], reads, 64)[1][0].tolist()
    calls = []
    calls.append(lambda: cm.pair_segments(pairs, reads, 0))
    calls.append(lambda: cm.correction_windows(o, reads, 0))
    calls.append(lambda: cm.correction_windows(o, reads, 64, -1))
    for field, value in (("query_read_id", len(reads)), ("target_read_id", len(reads)),
                         ("target_end_position_in_read", 100000), ("query_end_position_in_read", 100000)):
        bad = pairs.copy()
        bad[2][field] = value
        calls.append(lambda bad=bad: cm.pair_segments(bad, reads, 64))
        calls.append(lambda bad=bad: cm.correction_windows(bad, reads, 64))
    for call in calls:
        with pytest.raises(cm.MapperError):
            call()
        assert cm.pair_segments(pairs[:4], reads, 64)[1][0].tolist() == want
    # no overlaps: every window is its backbone
    empty = cm.correction_windows(np.zeros(0, O.OVERLAP), reads, 500)
    assert [(r, k, len(s)) for r, k, s in empty] == [(i, k, 1) for i, r in enumerate(reads)
                                                     for k in range((len(r) + 499) // 500)]
    assert b"".join(s[0] for _, _, s in empty) == "".join(reads).encode()
