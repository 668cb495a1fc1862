"""cudamapper under affine gap costs: align_overlaps(..., scoring=...) against
tests/oracle_affine.py on the slices of the polishing small case, both strands, independent of the chunking;
overlap_variants and polisher.call_variants over those alignments; the band's capacity; the refusals."""
import numpy as np
import pytest

import oracle_affine as OA
import oracle_pileup as OPi
import oracle_polish as OPo
import oracle_variants as OV
import pileup_cases as PC
import variant_cases as VC

pytestmark = pytest.mark.gpu

SCORING = (4, 6, 2, 64)


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


def aligner_rc(s):
    """the reverse complement as cudaaligner takes it: "TGAC"[(c >> 1) & 3] for every byte, back to front"""
    return "".join("TGAC"[(ord(c) >> 1) & 3] for c in reversed(s))


def slices(o, reads, drafts):
    out = []
    for x in o:
        q = reads[int(x["query_read_id"])][int(x["query_start_position_in_read"]):int(x["query_end_position_in_read"])]
        t = drafts[int(x["target_read_id"])][int(x["target_start_position_in_read"]):int(x["target_end_position_in_read"])]
        out.append((q, aligner_rc(t) if chr(x["relative_strand"]) == "-" else t))
    return out


@pytest.fixture(scope="module")
def polishing(cm):
    """the small case against two 3 % drafts of its genome, mapped on the device (the fixture of test_gpu_variants.py):
    reads, drafts, overlaps, and the oracle's alignment of every overlap's slices under SCORING, computed once"""
    reads, genome = OPo.small_case()
    drafts = [OPo.draft_of(genome, 0.03, OPo.SMALL["seed"]), PC.rc(OPo.draft_of(genome, 0.03, 5))]
    o = cm.map_reads_batched(reads, drafts, rescue_overlap_ends=True, **OPo.MAPPING)
    assert len(o) >= 30 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    assert set(o["target_read_id"].tolist()) == {0, 1}
    x, g, e, B = SCORING
    want = [OA.align(q, t, x, g, e, B) for q, t in slices(o, reads, drafts)]
    return reads, drafts, o, want


def test_cigars_and_edit_distances_equal_the_oracle(cm, polishing):
    reads, drafts, o, want = polishing
    timings = {}
    cigars, edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING, timings=timings)
    assert len(cigars) == len(o) and all(w["states"] is not None for w in want)
    for k, (c, d, w) in enumerate(zip(cigars, edits, want)):
        assert c == OA.cigar(w["states"]), (k, chr(o[k]["relative_strand"]))
        assert d == sum(1 for s in w["states"] if s != 0), k
    assert timings["align"] > 0
    # a dict is the same scoring
    again, again_edits = cm.align_overlaps(o, reads, drafts, scoring=dict(mismatch=4, gap_open=6, gap_extend=2, band=64))
    assert again == cigars and again_edits.tobytes() == edits.tobytes()


def test_chunking_does_not_change_the_result(cm, polishing):
    reads, drafts, o, _ = polishing
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed_scored(int(a), int(b), SCORING[3]) for a, b in zip(ql, tl))
    total = sum(cm.align_bytes_needed_scored(int(a), int(b), SCORING[3]) for a, b in zip(ql, tl))
    # a chunk's cost is at least the sum of its overlaps' bit matrices, which are most of `alone`: a budget of a fifth of
    # the call's sum forces four chunks and more
    budget = max(alone, total // 5)
    assert total > 4 * budget * 1.1
    whole, whole_edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING)
    chunked, chunked_edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING, max_device_bytes=budget)
    assert chunked == whole and chunked_edits.tobytes() == whole_edits.tobytes()
    lone, lone_edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING, max_device_bytes=alone)
    assert lone == whole and lone_edits.tobytes() == whole_edits.tobytes()
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.align_overlaps(o, reads, drafts, scoring=SCORING, max_device_bytes=alone - 1)


def test_no_scoring_is_the_call_without_the_argument(cm, polishing):
    reads, drafts, o, _ = polishing
    plain, plain_edits = cm.align_overlaps(o, reads, drafts)
    none, none_edits = cm.align_overlaps(o, reads, drafts, scoring=None)
    assert none == plain and none_edits.tobytes() == plain_edits.tobytes()
    assert cm.overlap_variants(o, reads, drafts, scoring=None).tobytes() == cm.overlap_variants(o, reads, drafts).tobytes()


def test_variants_are_the_oracle_on_the_calls_own_cigars(cm, polishing):
    reads, drafts, o, _ = polishing
    cigars, _ = cm.align_overlaps(o, reads, drafts, scoring=SCORING)
    alignments = OPi.of_cigars(cigars)
    for min_count, min_percent in ((1, 0), (3, 30)):
        got, piles = cm.overlap_variants(o, reads, drafts, min_count, min_percent, scoring=SCORING, return_pileup=True)
        assert VC.same_records(got, OV.overlap_variants(o, reads, drafts, alignments, "cigar", min_count, min_percent))
        assert len(got) > 0
    assert all((got["kind"] == k).any() for k in range(3))
    # independent of the chunking as well
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed_scored(int(a), int(b), SCORING[3]) for a, b in zip(ql, tl))
    assert cm.overlap_variants(o, reads, drafts, 3, 30, scoring=SCORING, max_device_bytes=alone).tobytes() == got.tobytes()


def test_call_variants_passes_the_scoring_through(cm, polishing):
    from genomeworks_amd import polisher
    reads, drafts, o, _ = polishing

    def by_cigar(kept):
        return OPi.of_cigars(cm.align_overlaps(kept, reads, drafts, scoring=SCORING)[0])

    got = polisher.call_variants(reads, drafts, overlaps=o, scoring=SCORING)
    assert got == OV.call_variants(reads, drafts, o, by_cigar) and len(got) > 10
    assert polisher.call_variants(reads, drafts, overlaps=o, scoring=None) == polisher.call_variants(reads, drafts, overlaps=o)


def test_a_band_over_the_capacity_gives_no_cigar(cm, polishing):
    reads, drafts, o, _ = polishing
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    few = o[(np.abs(ql - tl) <= 20) & (ql > 300)][:4].copy()
    assert len(few) == 4
    few[1]["query_end_position_in_read"] -= 100  # |m - n| of 80 and more: W > 2048 at B = 1000; the others stay below
    wide = (4, 6, 2, 1000)
    want = [OA.align(q, t, *wide) for q, t in slices(few, reads, drafts)]
    assert [w["states"] is None for w in want] == [False, True, False, False]
    cigars, edits = cm.align_overlaps(few, reads, drafts, scoring=wide)
    assert cigars == [OA.cigar(w["states"]) if w["states"] is not None else "" for w in want]
    assert edits.tolist() == [sum(1 for s in w["states"] if s != 0) if w["states"] is not None else -1 for w in want]
    # every overlap over the capacity: no CIGAR anywhere, no records, no fault
    cigars, edits = cm.align_overlaps(o, reads, drafts, scoring=(4, 6, 2, 1024))
    assert cigars == [""] * len(o) and edits.tolist() == [-1] * len(o)
    assert len(cm.overlap_variants(o, reads, drafts, 1, 0, scoring=(4, 6, 2, 1024))) == 0


def test_refusals(cm, polishing):
    from genomeworks_amd import _native, polisher
    reads, drafts, o, want = polishing
    for bad in ((0, 6, 2, 64), (256, 6, 2, 64), (4, -1, 2, 64), (4, 256, 2, 64), (4, 6, 0, 64), (4, 6, 256, 64), (4, 6, 2, -1),
                (4, 6, 2), dict(open=3)):
        with pytest.raises(ValueError):
            cm.align_overlaps(o, reads, drafts, scoring=bad)
        with pytest.raises(ValueError):
            cm.overlap_variants(o, reads, drafts, scoring=bad)
        with pytest.raises(ValueError):
            polisher.call_variants(reads, drafts, overlaps=o, scoring=bad)
    # the C API refuses the same before it uploads anything
    L = _native.mapper()
    q, t = cm._read_set_args(reads, drafts)
    records = np.ascontiguousarray(o, cm.OVERLAP)
    for bad in ((0, 6, 2, 64), (4, 256, 2, 64), (4, 6, 0, 64), (4, 6, 2, -1)):
        sc = np.array(bad, np.int32)
        assert not L.gw_mapper_align_overlaps_scored(cm._p(records), len(records), *q, 0, *t, 0, cm._p(sc), 0, None)
        assert "scoring" in L.gw_mapper_last_error().decode()
        assert not L.gw_mapper_overlap_variants_scored(cm._p(records), len(records), *q, 0, *t, 0, 3, 30, cm._p(sc), 0, None)
        assert "scoring" in L.gw_mapper_last_error().decode()
    bad = o.copy()
    bad[2]["target_end_position_in_read"] = 10 ** 7
    with pytest.raises(cm.MapperError):
        cm.align_overlaps(bad, reads, drafts, scoring=SCORING)
    # and the next call is whole
    cigars, _ = cm.align_overlaps(o[:6], reads, drafts, scoring=SCORING)
    assert cigars == [OA.cigar(w["states"]) for w in want[:6]]
