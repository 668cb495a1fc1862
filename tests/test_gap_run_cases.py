"""What the gap-run cases of tests/gap_run_cases.py guarantee, without a GPU, so that a later edit of the generator
cannot hollow out tests/test_gpu_gap_runs.py: the pinned aligner oracle finds the stated CIGAR of every case, the state
and CIGAR formulations of the segment, pileup and variant oracles agree on all of them, the grid does hold record lists
that skip windows and alignments with whole tiles of gap at their beginning and end, the three literals worked out on
paper hold against both formulations, and the window call gives the layer selection what it is for."""
import numpy as np
import pytest

import gap_run_cases as GC
import oracle_correct as OC
import oracle_mapper_align as OA
import oracle_pileup as OPi
import oracle_polish as OPo
import oracle_variants as OV
import pileup_cases as PC

INSERTION = PC.CHANNELS.index("insertion")


@pytest.fixture(scope="module")
def aligned():
    """the grid and the oracle's alignments of its records, computed once"""
    reads, o, cigars = GC.grid()
    return reads, o, cigars, OA.alignments(o, reads)


def test_the_grid_is_the_stated_one(aligned):
    reads, o, cigars, _ = aligned
    assert len(GC.GRID) == len(set(GC.GRID)) == len(o) == 336 and len(reads) == 672
    assert max(len(r) for r in reads) == 335 and min(len(r) for r in reads) == 1
    assert all((head, tail) != (0, 0) for head, _, tail, _, _ in GC.GRID)
    for i, (case, x) in enumerate(zip(GC.GRID, o)):
        head, run, tail, strand, run_in_query = case
        query, target = reads[2 * i], reads[2 * i + 1] if strand == "+" else PC.rc(reads[2 * i + 1])
        long, short = (query, target) if run_in_query else (target, query)
        # A nowhere but in the run, and the short read is the long one without it
        assert long.count("A") == run and long[head:head + run] == "A" * run and short == long[:head] + long[head + run:]
        assert (x["query_read_id"], x["target_read_id"]) == (2 * i, 2 * i + 1) and chr(x["relative_strand"]) == strand
        assert (x["query_end_position_in_read"], x["target_end_position_in_read"]) == (len(query), len(target))
        holder, at = GC.run_positions(case)
        assert {reads[2 * i + holder][p] for p in at} == {"T" if holder and strand == "-" else "A"} and len(at) == run
    assert cigars[GC.position(*GC.LITERAL_1[0])] == "64M128I70M" and cigars[GC.position(*GC.LITERAL_2[0])] == "63M128D70M"
    assert GC.cigar_of(0, 64, 1, True) == "64D1M" and GC.cigar_of(65, 200, 0, False) == "65M200I"


def test_the_oracle_finds_the_stated_cigars(aligned):
    _, _, cigars, alignments = aligned
    assert [a["cigar"] for a in alignments] == cigars
    assert [a["edit_distance"] for a in alignments] == [case[1] for case in GC.GRID]


def test_the_two_formulations_agree(aligned):
    reads, o, _, alignments = aligned
    for W in GC.WINDOW_LENGTHS:
        by_states = OC.pair_segments(o, reads, W, alignments)
        by_cigar = OC.pair_segments(o, reads, W, alignments, "cigar")
        for a, b in zip(by_states[0] + by_states[1], by_cigar[0] + by_cigar[1]):
            assert a.tolist() == b.tolist() and len(a) >= len(o), W
    for roles in ((False, True), (False,), (True,)):
        assert PC.same(OPi.pair_pileup(o, reads, alignments, roles=roles),
                       OPi.pair_pileup(o, reads, alignments, "cigar", roles=roles))
    by_states = OV.overlap_variants(o, reads, None, alignments, "states", 1, 0)
    by_cigar = OV.overlap_variants(o, reads, None, alignments, "cigar", 1, 0)
    assert by_states.tolist() == by_cigar.tolist()
    # every run exceeds 32 bases: none is called, and what is called is the deleted A's of the runs in the target
    assert set(by_cigar["kind"].tolist()) == {OV.DELETION} and by_cigar["count"].tolist() == [1] * len(by_cigar)
    want = [(2 * i + 1, p) for i, case in enumerate(GC.GRID) if not case[4] for p in GC.run_positions(case)[1]]
    assert list(zip(by_cigar["target_read"].tolist(), by_cigar["position"].tolist())) == want
    # the insertion channel: 1 in the read without the run where the run has a base of it on both sides
    piles = OPi.pair_pileup(o, reads, alignments, "cigar")
    for i, case in enumerate(GC.GRID):
        holder, _ = GC.run_positions(case)
        assert int(piles[2 * i + holder][INSERTION].sum()) == 0
        assert int(piles[2 * i + 1 - holder][INSERTION].sum()) == int(GC.has_both_neighbours(case)), case


def test_the_grid_holds_what_it_is_for(aligned):
    reads, o, _, alignments = aligned
    (target_role, target_offsets, _), (query_role, query_offsets) = OC.pair_segments(o, reads, 64, alignments)
    skipped = [GC.skipped_windows(records[int(a):int(b)].tolist())
               for records, offsets in ((target_role, target_offsets), (query_role, query_offsets))
               for a, b in zip(offsets[:-1], offsets[1:])]
    assert 1 in skipped and max(skipped) >= 2 and 0 in skipped
    # a record whose query range swallows a run of 128 bases and more
    for records in (target_role, query_role):
        assert int((records["query_end"].astype(np.int64) - records["query_begin"]).max()) >= 192
    empty = [GC.tiles_without_aligned_column(a["states"]) for a in alignments]
    assert any(e[0] for e in empty) and any(e[-1] for e in empty) and any(len(e) > 2 and e[0] and e[1] for e in empty)
    assert any(len(e) > 2 and e[-1] and e[-2] for e in empty)         # the last two as well
    assert any(not e[0] and not e[-1] and any(e) for e in empty)      # and a tile of gap in the middle
    assert any(e[0] and 3 in a["states"][:64] for e, a in zip(empty, alignments))  # of either state
    assert any(e[0] and 2 in a["states"][:64] for e, a in zip(empty, alignments))


@pytest.mark.parametrize("formulation", ["states", "cigar"])
def test_the_literals(aligned, formulation):
    reads, o, _, alignments = aligned
    (records, offsets, _), _ = OC.pair_segments(o, reads, 64, alignments, formulation)
    piles = OPi.pair_pileup(o, reads, alignments, formulation, roles=(False,))

    def variants_of(i):
        return OV.overlap_variants(o[i:i + 1], reads, None, alignments[i:i + 1], formulation, 1, 0)
    GC.check_literals(lambda i: records[int(offsets[i]):int(offsets[i + 1])].tolist(), lambda i: piles[2 * i + 1],
                      variants_of)


def test_the_window_call(aligned):
    reads, targets, o, cigars = GC.window_call()
    alignments = OA.alignments(o, reads, targets)
    assert [a["cigar"] for a in alignments] == cigars
    assert "A" not in targets[0] and len(targets[0]) == GC.WINDOW_TARGET_LENGTH
    for formulation in ("states", "cigar"):
        segs, offsets, _ = OPo.segments(o, reads, targets, 64, alignments, formulation)
        plan, table = OPo.select_layers(segs, o, [len(targets[0])], 64, 30)
        assert [n - 1 for _, _, _, n in table] == [4, 4, 4, 6, 6, 6, 6]
        # windows 1 and 2 have no layer of the two reads that miss them, window 0 none of the two that carry the run
        layers = lambda k: [plan[j][1] for j in range(table[k][2] + 1, table[k][2] + table[k][3])]
        assert sorted(layers(0)) == [0, 1, 4, 5] and sorted(layers(1)) == sorted(layers(2)) == [2, 3, 4, 5]
        refused = [s for s in segs if s["overlap"] in (2, 3) and s["window"] == 0]
        assert [(int(s["query_begin"]), int(s["query_end"])) for s in refused] == [(0, 192), (336, 528)]
    # at W = 128 the same two records hold 256 = 2 W bases, which a layer may
    segs, _, _ = OPo.segments(o, reads, targets, 128, alignments)
    plan, table = OPo.select_layers(segs, o, [len(targets[0])], 128, 30)
    first = plan[table[0][2] + 1:table[0][2] + table[0][3]]
    assert sorted(p[1] for p in first) == [2, 3, 4, 5] and {p[3] - p[2] for p in first if p[1] in (2, 3)} == {256}


def test_the_host_selection_equals_the_oracle_on_the_window_call():
    from genomeworks_amd import build, cudamapper as cm
    build.build_mapper()
    reads, targets, o, _ = GC.window_call()
    alignments = OA.alignments(o, reads, targets)
    for W, depth in ((64, 30), (64, 3), (128, 30), (200, 30), (7, 30)):
        segs, _, _ = OPo.segments(o, reads, targets, W, alignments)
        want = OPo.select_layers(segs, o, [len(targets[0])], W, depth)
        assert cm.select_layers(segs, o, len(reads), [len(targets[0])], W, depth) == want, (W, depth)
