"""The consumers of the 64-column tile walk (mapper/gwm_column_walk.hpp) on gap runs of a tile and longer
(tests/gap_run_cases.py; tests/test_gap_run_cases.py pins what the cases guarantee): tiles without a single aligned
column, tiles that are one run of state 2 or 3, alignments that begin or end with whole tiles of gap, windows an
alignment skips while it covers their neighbours, records whose query range swallows a run, and a deletion channel fed
by every lane of several tiles. Everything is byte for byte. The expected values are the CIGAR formulations of the
oracles applied to the device's own CIGARs, which are first asserted to be the stated strings, so no tie-break of an
aligner decides a test; all 336 records are checked in every test, each time in one call.

Every call is made as it is and once more with max_device_bytes at the largest single record's need, which cuts the
call into many chunks. align_overlaps and overlap_variants, the two entry points that take a scoring, also run under
the affine costs (4, 6, 2) and the two-piece costs (6, 4, 3, 24, 2) at band 16; the segment and pileup entry points
align with the default aligner alone."""
import numpy as np
import pytest

import gap_run_cases as GC
import oracle_correct as OC
import oracle_mapper_align as OA
import oracle_pileup as OPi
import oracle_polish as OPo
import oracle_polish_quality as OQ
import oracle_variants as OV
import pileup_cases as PC
import variant_cases as VC

pytestmark = pytest.mark.gpu

INSERTION = PC.CHANNELS.index("insertion")
HOW = ("whole", "chunked")
SCORINGS = (None, GC.AFFINE, GC.TWO_PIECE)


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def grid(cm):
    """the grid, the device's CIGARs of it under the default aligner -- the stated ones --, and the budgets that give
    the largest record a chunk of its own, sized as tests/test_gpu_polish.py sizes them"""
    reads, o, stated = GC.grid()
    cigars, edits = cm.align_overlaps(o, reads)
    assert cigars == stated and edits.tolist() == [case[1] for case in GC.GRID]
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
    scored = max(cm.align_bytes_needed_scored(int(a), int(b), GC.AFFINE[-1]) for a, b in zip(ql, tl))
    # a chunk counts its slices' bases four times and more (gathered, state slots, two bytes per column), so within
    # the scored budget the records take five chunks and more. The default aligner's workspace is counted per wave of
    # 64 records and is most of `alone`: how many chunks that budget makes is the chunk loop's business, the budget is
    # the smallest the call can have (test_the_cigars_are_the_stated_ones shows that one byte less is refused)
    assert 4 * int((ql + tl).sum()) > 5 * scored
    return dict(reads=reads, o=o, cigars=cigars, alignments=OPi.of_cigars(cigars), alone=alone, scored=scored)


def budget(grid, how, scoring=None):
    if how == "whole":
        return dict()
    return dict(max_device_bytes=grid["scored" if scoring else "alone"])


def from_cigars(o, cigars, W, from_cigar):
    """(records, offsets) of one role by a CIGAR formulation"""
    rows = [from_cigar(i, o[i], cigars[i], W) for i in range(len(o))]
    return (np.array([r for per_record in rows for r in per_record], OC.SEGMENT).reshape(-1),
            np.cumsum([0] + [len(r) for r in rows]))


@pytest.fixture(scope="module")
def expected(grid):
    """what the CIGAR formulations make of the device's CIGARs, computed once: the records of both roles per window
    length, the pileups of both roles together and of the target role alone, and the variants at min_count = 1"""
    o, reads, cigars, alignments = grid["o"], grid["reads"], grid["cigars"], grid["alignments"]
    return dict(target_role={W: from_cigars(o, cigars, W, OPo.segments_from_cigar) for W in GC.WINDOW_LENGTHS},
                query_role={W: from_cigars(o, cigars, W, OC.query_role_from_cigar) for W in GC.WINDOW_LENGTHS},
                both=OPi.pair_pileup(o, reads, alignments, "cigar"),
                of_targets=OPi.pair_pileup(o, reads, alignments, "cigar", roles=(False,)),
                variants=OV.overlap_variants(o, reads, None, alignments, "cigar", 1, 0))


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("scoring", SCORINGS, ids=("default", "affine", "two_piece"))
def test_the_cigars_are_the_stated_ones(cm, grid, scoring, how):
    cigars, edits = cm.align_overlaps(grid["o"], grid["reads"], scoring=scoring, **budget(grid, how, scoring))
    for i, case in enumerate(GC.GRID):
        assert cigars[i] == grid["cigars"][i] == GC.cigar_of(case[0], case[1], case[2], case[4]), (case, cigars[i])
    assert edits.dtype == np.int32 and edits.tolist() == [case[1] for case in GC.GRID]
    if how == "chunked":  # the budget is the smallest the call can have
        with pytest.raises(cm.MapperError, match="max_device_bytes"):
            cm.align_overlaps(grid["o"], grid["reads"], scoring=scoring,
                              max_device_bytes=budget(grid, how, scoring)["max_device_bytes"] - 1)


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("W", GC.WINDOW_LENGTHS)
def test_the_records_of_both_roles(cm, grid, expected, W, how):
    o, reads = grid["o"], grid["reads"]
    (target_role, target_offsets, edits), (query_role, query_offsets) = cm.pair_segments(o, reads, W, **budget(grid, how))
    for role, got, offsets in (("target_role", target_role, target_offsets), ("query_role", query_role, query_offsets)):
        want, want_offsets = expected[role][W]
        assert got.dtype == cm.SEGMENT and offsets.tolist() == want_offsets.tolist(), (role, W)
        for i, case in enumerate(GC.GRID):  # the smallest failing case is a single record
            a, b = int(want_offsets[i]), int(want_offsets[i + 1])
            assert got[a:b].tolist() == want[a:b].tolist(), (role, W, case)
    assert edits.tolist() == [case[1] for case in GC.GRID]
    if W == 64:  # windows are skipped, and ranges swallow runs, on the device's own records too
        skipped = [GC.skipped_windows(target_role[int(a):int(b)].tolist()) for a, b in zip(target_offsets[:-1], target_offsets[1:])]
        assert 1 in skipped and max(skipped) >= 2
        assert int((target_role["query_end"].astype(np.int64) - target_role["query_begin"]).max()) >= 192
    # the targets as a second read set: the same target-role records out of gwm_window_segments
    apart = o.copy()
    apart["query_read_id"] //= 2
    apart["target_read_id"] //= 2
    segments, offsets, apart_edits = cm.window_segments(apart, reads[0::2], reads[1::2], W, **budget(grid, how))
    assert segments.tolist() == target_role.tolist() and offsets.tolist() == target_offsets.tolist()
    assert apart_edits.tolist() == edits.tolist()


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("order", ("as_given", "reversed"))
def test_the_pileups_of_both_roles(cm, grid, expected, order, how):
    o, reads = grid["o"], grid["reads"]
    records = o if order == "as_given" else np.ascontiguousarray(o[::-1])
    both = cm.pair_pileup(records, reads, **budget(grid, how))
    of_targets = cm.overlap_pileup(records, reads, **budget(grid, how))
    for i, case in enumerate(GC.GRID):
        for r in (2 * i, 2 * i + 1):
            assert np.array_equal(both[r], expected["both"][r]), (case, r)
            assert np.array_equal(of_targets[r], expected["of_targets"][r]), (case, r)
        # a deletion channel fed by every lane of the run's tiles, an insertion counted once or nowhere
        holder, at = GC.run_positions(case)
        assert both[2 * i + holder][OPi.DELETION].nonzero()[0].tolist() == at
        assert int(both[2 * i + 1 - holder][INSERTION].sum()) == int(GC.has_both_neighbours(case)), case
        assert not both[2 * i + holder][INSERTION].any() and (OPi.depth(both[2 * i + holder]) == 1).all()
    assert PC.same(both, expected["both"]) and PC.same(of_targets, expected["of_targets"])


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("scoring", SCORINGS, ids=("default", "affine", "two_piece"))
def test_the_variants(cm, grid, expected, scoring, how):
    o, reads = grid["o"], grid["reads"]
    got, piles = cm.overlap_variants(o, reads, None, 1, 0, return_pileup=True, scoring=scoring, **budget(grid, how, scoring))
    assert VC.same_records(got, expected["variants"])
    # no insertion record: every run exceeds the longest allele; the deletions are the A's of the runs in the target
    assert set(got["kind"].tolist()) == {OV.DELETION} and got["count"].tolist() == got["depth"].tolist() == [1] * len(got)
    want = [(2 * i + 1, p) for i, case in enumerate(GC.GRID) if not case[4] for p in GC.run_positions(case)[1]]
    assert list(zip(got["target_read"].tolist(), got["position"].tolist())) == want
    assert PC.same(piles, expected["of_targets"])
    if scoring is None and how == "whole":
        assert PC.same(piles, cm.overlap_pileup(o, reads))


def test_the_quality_sums_of_both_roles(cm, grid, expected):
    o, reads = grid["o"], grid["reads"]
    qualities = OQ.qualities_for(reads)
    (target_role, _, _), (query_role, _) = cm.pair_segments(o, reads, 64)
    assert target_role.tolist() == expected["target_role"][64][0].tolist()
    assert query_role.tolist() == expected["query_role"][64][0].tolist()
    for records, role in ((target_role, False), (query_role, True)):
        spans = records["query_end"].astype(np.int64) - records["query_begin"]
        assert (spans >= 192).sum() >= 8 and spans.max() >= 264  # several passes of the kernel's loop
        got = cm.segment_quality_sums(records, o, qualities, query_role=role)
        want = OQ.quality_sums(records, o, qualities, query_role=role)
        assert got.dtype == np.uint32 and got.tolist() == want.tolist(), role
        assert got[spans >= 192].min() > 0


def test_the_window_call(cm):
    from genomeworks_amd import polisher
    reads, targets, o, stated = GC.window_call()
    cigars, _ = cm.align_overlaps(o, reads, targets)
    assert cigars == stated
    alignments = OA.alignments(o, reads, targets)
    assert [a["cigar"] for a in alignments] == cigars  # the oracle's alignments are the device's
    lengths = [len(t) for t in targets]
    for W, depth in ((64, 30), (64, 3), (128, 30)):
        want_segments, want_offsets = from_cigars(o, cigars, W, OPo.segments_from_cigar)
        segments, offsets, _ = cm.window_segments(o, reads, targets, W)
        assert segments.tolist() == want_segments.tolist() and offsets.tolist() == want_offsets.tolist()
        want_plan, want_table = OPo.select_layers(want_segments, o, lengths, W, depth)
        plan, table = cm.select_layers(segments, o, len(reads), lengths, W, depth)
        assert (plan, table) == (want_plan, want_table), (W, depth)
        want = OPo.windows(o, reads, targets, W, depth, alignments)
        got = cm.overlap_windows(o, reads, targets, W, depth)
        assert got == want, (W, depth)
        assert b"".join(seqs[0] for _, _, seqs in got) == targets[0].encode()
        layers = lambda k: [plan[j][1] for j in range(table[k][2] + 1, table[k][2] + table[k][3])]
        if (W, depth) == (64, 30):
            # windows 1 and 2 from four reads only; window 0 of the reads that carry the run is refused: 192 > 2 W bases
            assert [len(seqs) - 1 for _, _, seqs in got] == [4, 4, 4, 6, 6, 6, 6]
            assert sorted(layers(0)) == [0, 1, 4, 5] and sorted(layers(1)) == sorted(layers(2)) == [2, 3, 4, 5]
            refused = [s for s in segments if s["overlap"] in (2, 3) and s["window"] == 0]
            assert [(int(s["query_begin"]), int(s["query_end"])) for s in refused] == [(0, 192), (336, 528)]
        if W == 128:
            # 256 = 2 W bases are a layer: window 0 holds the whole run of both reads that carry it (the '-' read has
            # T's, which its layer, cut out reversed and complemented, shows as A's)
            assert sorted(layers(0)) == [2, 3, 4, 5]
            assert sorted(len(s) for s in got[0][2][1:]) == [128, 128, 256, 256]
            assert sum(s.count(b"A" * 128) for s in got[0][2][1:]) == 2
    want, want_report = OPo.polish(reads, targets, o, 64, 15, 64, alignments=alignments)
    got, report = polisher.polish(reads, targets, overlaps=o, window_length=64, max_depth=15, band_width=64,
                                  poa_memory_per_device=1 << 30)
    assert got == want
    assert [(r["target_read"], r["window"], r["layers"], r["status"], r["backbone_kept"]) for r in report] == want_report


def test_the_literals(cm, grid):
    o, reads = grid["o"], grid["reads"]
    (records, offsets, _), _ = cm.pair_segments(o, reads, 64)
    piles = cm.overlap_pileup(o, reads)
    variants = cm.overlap_variants(o, reads, None, 1, 0)
    GC.check_literals(lambda i: records[int(offsets[i]):int(offsets[i + 1])].tolist(), lambda i: piles[2 * i + 1],
                      lambda i: variants[variants["target_read"] == 2 * i + 1])
