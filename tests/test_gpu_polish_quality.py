"""Base-quality weights on the device (tests/oracle_polish_quality.py is the oracle): the
quality sums of segment records against numpy, the weights of the window sequences byte for byte, weights through
cudapoa's multi-device runner against the POA oracle, polish() and correct_reads() with qualities against the oracle
pipelines, and the refusals."""
import numpy as np
import pytest

import oracle_mapper as O
import oracle_poa as OP
import oracle_polish as OPo
import oracle_polish_quality as OQ

pytestmark = pytest.mark.gpu

POA = dict(band_mode="static_band", memory_per_device=1 << 30)


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def small(cm):
    """the small case with qualities: reads, qualities, genome, a 3 % draft, the device's overlaps of the reads against
    the draft and of the reads against themselves, computed once"""
    reads, genome = OPo.small_case()
    draft = OPo.draft_of(genome, 0.03, OPo.SMALL["seed"])
    o = cm.map_reads_batched(reads, [draft], rescue_overlap_ends=True, **OPo.MAPPING)
    assert len(o) >= 20 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    among = cm.map_reads_batched(reads, reads, rescue_overlap_ends=True, **OPo.MAPPING)
    return dict(reads=reads, qualities=OQ.qualities_for(reads), genome=genome, draft=draft, overlaps=o, among=among,
                pairs=among[cm.select_pairs(among)])


@pytest.fixture(scope="module")
def records(cm, small):
    """the device's segment records at W = 200, which tests/test_gpu_polish.py and tests/test_gpu_correct.py hold
    against the alignment oracle: (of the overlaps against the draft, (target role, query role) of the pairs)"""
    s = small
    target_role, query_role = cm.pair_segments(s["pairs"], s["reads"], 200)
    return cm.window_segments(s["overlaps"], s["reads"], [s["draft"]], 200)[0], (target_role[0], query_role[0])


@pytest.mark.parametrize("W", [7, 64, 4096])
def test_quality_sums_of_every_record_equal_numpy(cm, small, W):
    s = small
    reads, q = s["reads"], s["qualities"]
    segs = cm.window_segments(s["overlaps"], reads, [s["draft"]], W)[0]
    (target_role, _, _), (query_role, _) = cm.pair_segments(s["pairs"], reads, W)
    timings = {}
    for records, overlaps, role in ((segs, s["overlaps"], False), (target_role, s["pairs"], False),
                                    (query_role, s["pairs"], True)):
        got = cm.segment_quality_sums(records, overlaps, q, query_role=role, timings=timings)
        assert got.dtype == np.uint32 and len(got) == len(records) >= len(overlaps)
        assert got.tolist() == OQ.quality_sums(records, overlaps, q, query_role=role).tolist()
        assert timings["quality_sums"] > 0
    lengths = set((segs["query_end"].astype(np.int64) - segs["query_begin"]).tolist())
    if W == 7:
        assert min(lengths) <= 7 and len(lengths) >= 5
    if W == 4096:
        assert min(lengths) > 64 and any(n % 64 for n in lengths)


def test_quality_sums_of_hand_records(cm):
    """records of 1 byte, around one pass of the wave, of many passes, of no bytes and of a whole read; read ids that
    count from 7; both roles; a read of 50 M bytes of '~' saturates"""
    rng = np.random.default_rng(99)
    q = [(rng.integers(0, 94, n).astype(np.uint8) + 33).tobytes() for n in (1, 300, 5000)]
    o = np.array([(7, 8, 0, 0, 1, 300, ord("+"), 0, 0), (9, 8, 0, 0, 5000, 300, ord("-"), 0, 0)], O.OVERLAP)
    spans = [(0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 10, 73), (1, 10, 74), (1, 10, 75), (1, 4999, 5000), (1, 1, 4998),
             (1, 0, 5000), (1, 63, 128), (1, 64, 128), (1, 2500, 2500)]
    records = np.array([(i, 0, 0, 0, b, e) for i, b, e in spans], OPo.SEGMENT)
    got = cm.segment_quality_sums(records, o, q, first_read_id=7)
    assert got.tolist() == OQ.quality_sums(records, o, q, first_read_id=7).tolist()
    assert got[1] == 0 and got[11] == 0 and got[8] == sum(q[2]) - 33 * 5000
    # the query role reads the target read's bytes: read 8 for both overlaps
    inside = records[[1, 2, 3, 4, 5]].copy()
    inside["query_end"] = np.minimum(inside["query_end"], 300)
    got = cm.segment_quality_sums(inside, o, q, first_read_id=7, query_role=True)
    assert got.tolist() == OQ.quality_sums(inside, o, q, first_read_id=7, query_role=True).tolist()
    assert got[2] == sum(q[1][10:73]) - 33 * 63
    # 50 M bytes of Phred 93 are more than 2^32 - 1
    big = [b"~" * 50_000_000]
    whole = np.array([(0, 0, 0, 0, 0, 50_000_000), (0, 0, 0, 0, 1, 2)], OPo.SEGMENT)
    one = np.array([(0, 0, 0, 0, 50_000_000, 50_000_000, ord("+"), 0, 0)], O.OVERLAP)
    assert cm.segment_quality_sums(whole, one, big).tolist() == [2 ** 32 - 1, 93]


def test_quality_sums_refusals_leave_the_device_usable(cm):
    q = ["I" * 10, "5" * 20]
    o = np.array([(0, 1, 0, 0, 10, 20, ord("+"), 0, 0)], O.OVERLAP)
    good = np.array([(0, 0, 0, 0, 2, 9)], OPo.SEGMENT)
    for bad in ((1, 0, 0, 0, 2, 9), (0, 0, 0, 0, 2, 11), (0, 0, 0, 0, 9, 2)):
        with pytest.raises(cm.MapperError):
            cm.segment_quality_sums(np.array([good[0], bad], OPo.SEGMENT), o, q)
        assert cm.segment_quality_sums(good, o, q).tolist() == [7 * 40]
    with pytest.raises(cm.MapperError):  # a read outside the set
        cm.segment_quality_sums(good, o, q, first_read_id=1)
    assert cm.segment_quality_sums(good, o, q, query_role=True).tolist() == [7 * 20]
    with pytest.raises(ValueError):
        cm.segment_quality_sums(good, o, ["I" * 9 + " ", "5" * 20])
    assert cm.segment_quality_sums(good[:0], o, q).tolist() == []


def test_quality_sums_do_not_depend_on_the_chunking(cm, small):
    s = small
    o, reads = s["overlaps"], s["reads"]
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
    got = []
    for budget in (0, alone):
        weighted = dict(query_qualities=cm.pack_qualities(s["qualities"], reads), target_qualities=None,
                        min_mean_quality=10)
        (segs, _, _), _ = cm._window_overlaps(o, reads, [s["draft"]], 64, 15, 0, 0, budget, None, None, weighted)
        assert weighted["quality_sums"].tolist() == OQ.quality_sums(segs, o, s["qualities"]).tolist()
        got.append((segs.tolist(), weighted["quality_sums"].tolist(), weighted["weights"].tolist()))
    assert got[0] == got[1] and len(got[0][1]) == len(got[0][0]) > len(o)


def same_windows(got, want):
    assert [(t, k, seqs) for t, k, seqs, _ in got] == [(t, k, seqs) for t, k, seqs, _ in want]
    for (_, _, _, a), (_, _, _, b) in zip(got, want):
        assert all(x.dtype == np.int8 for x in a) and [x.tolist() for x in a] == [x.tolist() for x in b]


def test_weighted_polish_windows_equal_the_oracle(cm, small):
    s = small
    reads, q, draft, o = s["reads"], s["qualities"], s["draft"], s["overlaps"]
    draft_q = OQ.qualities_for([draft], seed=8, zero_read=-1)
    for W, depth, threshold, tq in ((200, 30, 10, None), (200, 3, 0, draft_q), (64, 15, 25, None), (4096, 30, 10, draft_q)):
        segs = cm.window_segments(o, reads, [draft], W)[0]
        want = OQ.polish_windows(o, reads, [draft], W, depth, q, tq, threshold, segs=segs)
        timings = {}
        got = cm.overlap_windows_weighted(o, reads, [draft], q, tq, W, depth, threshold, timings=timings)
        same_windows(got, want)
        backbones = np.concatenate([w[0] for _, _, _, w in got])
        assert backbones.tolist() == ([1] * len(draft) if tq is None else [c - 33 for c in draft_q[0].encode()])
        if (W, depth) == (200, 30):
            assert timings["quality_sums"] > 0 and timings["weight_gather"] > 0
            plain_timings = {}
            plain = cm.overlap_windows(o, reads, [draft], W, depth, timings=plain_timings)
            assert sum(len(x[2]) for x in got) < sum(len(x[2]) for x in plain)
            # beyond the unweighted call: 4 B per record and one weight byte per window base
            assert timings["bytes_to_host"] - 2 * timings["window_bases"] - 4 * len(segs) == \
                plain_timings["bytes_to_host"] - plain_timings["window_bases"]
    # '-' layers are reversed and not complemented: the weights of a layer are its read's, back to front
    segs = cm.window_segments(o, reads, [draft], 200)[0]
    plan, table = OQ.select_layers(segs, o, [len(draft)], 200, 30, OQ.quality_sums(segs, o, q), 10)
    got = cm.overlap_windows_weighted(o, reads, [draft], q, None, 200, 30, 10)
    flat = [w for _, _, _, ws in got for w in ws]
    reversed_layers = [(p, w) for p, w in zip(plan, flat) if p[0] == 0 and p[4] == 1]
    assert reversed_layers and any(p[0] == 0 and p[4] == 0 for p in plan)
    for (_, read, begin, end, _), w in reversed_layers:
        assert w.tolist() == [ord(c) - 33 for c in q[read][begin:end]][::-1]
    # no qualities at all: unit weights and the layers of overlap_windows
    unit = cm.overlap_windows_weighted(o, reads, [draft], None, None, 200, 30, 10)
    assert [x[:3] for x in unit] == cm.overlap_windows(o, reads, [draft], 200, 30)
    assert all(set(w.tolist()) == {1} for _, _, _, ws in unit for w in ws)
    # threshold 0 and no zero-sum layer: the bases of overlap_windows, byte for byte
    kept = o[o["query_read_id"] != 3]
    assert [x[:3] for x in cm.overlap_windows_weighted(kept, reads, [draft], q, None, 200, 30, 0)] == \
        cm.overlap_windows(kept, reads, [draft], 200, 30)


def test_weighted_correction_windows_equal_the_oracle(cm, small, records):
    s = small
    reads, q, among = s["reads"], s["qualities"], s["among"]
    for depth, threshold in ((30, 10), (3, 0)):
        want = OQ.correction_windows(among, reads, q, 200, depth, threshold, records=records[1])
        timings = {}
        got = cm.correction_windows_weighted(among, reads, q, 200, depth, threshold, timings=timings)
        same_windows(got, want)
        assert timings["quality_sums"] > 0 and timings["weight_gather"] > 0
    # every backbone carries its read's own weights; read 3's are all zero
    for r, k, seqs, weights in got:
        assert weights[0].tolist() == [ord(c) - 33 for c in q[r][200 * k:200 * k + 200]]
    plain = cm.correction_windows(among, reads, 200, 30)
    got = cm.correction_windows_weighted(among, reads, q, 200, 30, 10)
    assert sum(len(x[2]) for x in got) < sum(len(x[2]) for x in plain)
    unit = cm.correction_windows_weighted(among, reads, None, 200, 30, 10)
    assert [x[:3] for x in unit] == plain and all(set(w.tolist()) == {1} for _, _, _, ws in unit for w in ws)


def oracle_rows(windows, cfg):
    with OP.Workspace(cfg) as ws:
        return [ws.process(seqs, weights) for seqs, weights in windows]


def test_multi_device_runner_with_weights_equals_the_poa_oracle(cm, small, records):
    from genomeworks_amd import cudapoa
    s = small
    wins = OQ.polish_windows(s["overlaps"], s["reads"], [s["draft"]], 200, 15, s["qualities"], None, 10,
                             segs=records[0])
    deep = [(seqs, weights) for _, _, seqs, weights in wins if len(seqs) - 1 >= 2]
    wins = OQ.correction_windows(s["among"], s["reads"], s["qualities"], 200, 15, 10, records=records[1])
    deep += [(seqs, weights) for r, _, seqs, weights in wins if len(seqs) - 1 >= 2 and r != 3]
    deep = deep[:4] + deep[-4:]
    assert len(deep) == 8
    size, depth, band = OPo.poa_shape(200, 15, 64)
    want = oracle_rows(deep, OP.make_cfg(size, depth, band, 1))
    got = cudapoa.process_windows_multi_device([seqs for seqs, _ in deep], depth, size, alignment_band_width=band,
                                               weights=[weights for _, weights in deep], **POA)
    assert got["status"] == [int(r["status"]) for r in want] == [0] * 8
    assert got["consensus"] == [r["consensus"] for r in want]
    assert got["coverage"] == [list(r["coverage"]) for r in want]
    plain = cudapoa.process_windows_multi_device([seqs for seqs, _ in deep], depth, size, alignment_band_width=band, **POA)
    # weights=None is the existing call, and so are unit weights, given as None or as ones
    again = cudapoa.process_windows_multi_device([seqs for seqs, _ in deep], depth, size, alignment_band_width=band,
                                                 weights=None, **POA)
    ones = [[None if i % 2 else np.ones(len(x), np.int8) for i, x in enumerate(seqs)] for seqs, _ in deep]
    unit = cudapoa.process_windows_multi_device([seqs for seqs, _ in deep], depth, size, alignment_band_width=band,
                                                weights=ones, **POA)
    for key in ("status", "consensus", "coverage"):
        assert plain[key] == again[key] == unit[key]


def test_weights_flip_the_paper_window_on_the_device():
    from genomeworks_amd import cudapoa
    truth, reads, weights = OQ.paper_case()
    want = oracle_rows([(reads, None), (reads, weights)], OP.make_cfg(512, 8, 128, 1))
    assert want[0]["consensus"] == reads[0] != truth == want[1]["consensus"]
    plain = cudapoa.process_windows_multi_device([reads], 8, 512, alignment_band_width=128, **POA)
    weighted = cudapoa.process_windows_multi_device([reads], 8, 512, alignment_band_width=128, weights=[weights], **POA)
    assert plain["status"] == weighted["status"] == [0]
    assert plain["consensus"] == [reads[0]] and weighted["consensus"] == [truth]
    assert weighted["coverage"] == [list(want[1]["coverage"])]


def test_a_zero_weighted_read_refuses_its_window_alone():
    from genomeworks_amd import cudapoa
    truth, reads, weights = OQ.paper_case()
    other = [r[:300] for r in reads]
    zero = [None, np.zeros(333, np.int8), weights[2], weights[3]]
    windows = [reads, reads, other]
    given = [weights, zero, [None if w is None else w[:300] for w in weights]]
    got = cudapoa.process_windows_multi_device(windows, 8, 512, alignment_band_width=128, weights=given, **POA)
    assert got["status"] == [0, cudapoa.zero_weighted_poa_sequence, 0]
    assert got["consensus"][1] == "" and got["coverage"][1] == []
    alone = cudapoa.process_windows_multi_device([reads, other], 8, 512, alignment_band_width=128,
                                                 weights=[given[0], given[2]], **POA)
    want = oracle_rows([(reads, given[0]), (other, given[2])], OP.make_cfg(512, 8, 128, 1))
    assert [got["consensus"][i] for i in (0, 2)] == alone["consensus"] == [r["consensus"] for r in want]
    assert [got["coverage"][i] for i in (0, 2)] == alone["coverage"] == [list(r["coverage"]) for r in want]
    assert want[0]["consensus"] == truth
    for bad in ([weights], [weights, zero, given[2][:3]], [weights, [None, None, None, np.ones(3, np.int8)], given[2]]):
        with pytest.raises(ValueError):
            cudapoa.process_windows_multi_device(windows, 8, 512, alignment_band_width=128, weights=bad, **POA)
    negative = [weights, [None, None, None, np.full(333, -1, np.int8)], given[2]]
    with pytest.raises(RuntimeError):
        cudapoa.process_windows_multi_device(windows, 8, 512, alignment_band_width=128, weights=negative, **POA)
    assert cudapoa.process_windows_multi_device([reads], 8, 512, alignment_band_width=128, weights=[weights],
                                                **POA)["consensus"] == [truth]


def as_rows(report):
    return [(r["target_read"], r["window"], r["layers"], r["status"], r["backbone_kept"]) for r in report]


def test_polish_with_qualities_equals_the_oracle_pipeline(cm, small, records):
    from genomeworks_amd import polisher
    s = small
    reads, q, draft, o = s["reads"], s["qualities"], s["draft"], s["overlaps"]
    want, want_report = OQ.polish(reads, [draft], o, 200, 15, 64, read_qualities=q, segs=records[0])
    timings = {}
    got, report = polisher.polish(reads, [draft], overlaps=o, window_length=200, max_depth=15, band_width=64,
                                  timings=timings, poa_memory_per_device=1 << 30, read_qualities=q)
    assert got == want and as_rows(report) == want_report
    assert all(timings[k] > 0 for k in ("align", "segments", "quality_sums", "weight_gather", "window_gather"))
    assert sum(1 for r in report if r["status"] == 0) >= 3
    # the Phred 2..8 reads and the all-'!' read contribute no layer: fewer layers than without qualities
    _, unfiltered = polisher.polish(reads, [draft], overlaps=o, window_length=200, max_depth=15, band_width=64,
                                    poa_memory_per_device=1 << 30)
    assert [r["layers"] for r in report] == [r[2] for r in want_report] != [r["layers"] for r in unfiltered]
    assert all(a["layers"] <= b["layers"] for a, b in zip(report, unfiltered))
    low = {i for i in range(len(reads)) if i % 5 == 0 or i == 3}
    segs = records[0]
    plan, _ = OQ.select_layers(segs, o, [len(draft)], 200, 15, OQ.quality_sums(segs, o, q), 10)
    assert not any(p[0] == 0 and p[1] in low for p in plan)
    assert any(p[0] == 0 and p[1] in low for p in OPo.select_layers(segs, o, [len(draft)], 200, 15)[0])
    # target qualities alone: every layer of the unfiltered run, the backbone weighted
    tq = OQ.qualities_for([draft], seed=8, zero_read=-1)
    want, want_report = OQ.polish(reads, [draft], o, 200, 15, 64, target_qualities=tq, segs=segs)
    got, report = polisher.polish(reads, [draft], overlaps=o, window_length=200, max_depth=15, band_width=64,
                                  poa_memory_per_device=1 << 30, target_qualities=tq)
    assert got == want and as_rows(report) == want_report
    assert [r["layers"] for r in report] == [r["layers"] for r in unfiltered]


def test_correct_reads_with_qualities_equals_the_oracle_pipeline(cm, small, records):
    from genomeworks_amd import polisher
    s = small
    reads, q, among = s["reads"], s["qualities"], s["among"]
    want, want_report = OQ.correct(reads, among, q, 200, 15, 64, records=records[1])
    timings = {}
    got, report = polisher.correct_reads(reads, overlaps=among, window_length=200, max_depth=15, band_width=64,
                                         timings=timings, poa_memory_per_device=1 << 30, qualities=q)
    assert got == want and as_rows(report) == want_report
    assert all(timings[k] > 0 for k in ("quality_sums", "weight_gather", "query_role_segments"))
    _, unfiltered = polisher.correct_reads(reads, overlaps=among, window_length=200, max_depth=15, band_width=64,
                                           poa_memory_per_device=1 << 30)
    assert [r["layers"] for r in report] == [r[2] for r in want_report] != [r["layers"] for r in unfiltered]
    assert all(a["layers"] <= b["layers"] for a, b in zip(report, unfiltered))
    # read 3's backbone weights sum to 0: its windows keep the backbone and their POA is not run, whatever spans them
    of_read_3 = [r for r in report if r["target_read"] == 3]
    assert of_read_3 and all(r["status"] is None and r["backbone_kept"] for r in of_read_3)
    assert any(r["layers"] >= 2 for r in of_read_3) and got[3] == reads[3]
    assert sum(1 for r in report if r["status"] == 0) >= 10


def test_refusals_leave_the_device_usable(cm, small):
    from genomeworks_amd import polisher
    s = small
    reads, q, draft, o, among = s["reads"], s["qualities"], s["draft"], s["overlaps"], s["among"]
    want = cm.window_segments(o[:4], reads, [draft], 64)[0].tolist()
    short = q[:1] + [q[1][:-1]] + q[2:]
    byte_32 = q[:2] + [" " + q[2][1:]] + q[3:]
    calls = []
    for bad in (short, byte_32):
        calls.append(lambda bad=bad: cm.overlap_windows_weighted(o, reads, [draft], bad, None, 64))
        calls.append(lambda bad=bad: cm.correction_windows_weighted(among, reads, bad, 64))
        calls.append(lambda bad=bad: polisher.polish(reads, [draft], overlaps=o, read_qualities=bad))
        calls.append(lambda bad=bad: polisher.correct_reads(reads, overlaps=among, qualities=bad))
    calls.append(lambda: cm.overlap_windows_weighted(o, reads, [draft], q, ["I" * (len(draft) + 1)], 64))
    calls.append(lambda: cm.overlap_windows_weighted(o, reads, [draft], q, None, 64, min_mean_quality=-1))
    calls.append(lambda: cm.correction_windows_weighted(among, reads, q, 64, min_mean_quality=-1))
    calls.append(lambda: polisher.polish(reads, [draft], overlaps=o, read_qualities=q, min_mean_quality=-1))
    for call in calls:
        with pytest.raises(ValueError):
            call()
        assert cm.window_segments(o[:4], reads, [draft], 64)[0].tolist() == want
    # what the library itself refuses, past the Python checks: a byte of 32 and a negative threshold
    L = cm._native.mapper()
    (qb, qo, nq), (tb, to, nt) = cm._read_set_args(reads, [draft])
    for flat, threshold in ((cm.pack_reads(byte_32)[0], 10), (cm.pack_qualities(q, reads), -1)):
        assert not L.gw_mapper_window_overlaps_weighted(cm._p(o), len(o), qb, qo, nq, 0, tb, to, nt, 0, cm._p(flat), None,
                                                        threshold, 64, 15, 0, None)
        assert b"gw_mapper_window_overlaps_weighted" in L.gw_mapper_last_error()
        assert cm.window_segments(o[:4], reads, [draft], 64)[0].tolist() == want
    with pytest.raises(cm.MapperError):  # the device-side checks of the unweighted call still hold
        cm.overlap_windows_weighted(o, reads, [draft], q, None, 0)
    assert cm.window_segments(o[:4], reads, [draft], 64)[0].tolist() == want
    empty = cm.overlap_windows_weighted(np.zeros(0, O.OVERLAP), reads, [draft], q, None, 500)
    assert [(t, k, len(x), [len(v) for v in w]) for t, k, x, w in empty] == \
        [(0, k, 1, [len(draft[500 * k:500 * k + 500])]) for k in range(3)]
