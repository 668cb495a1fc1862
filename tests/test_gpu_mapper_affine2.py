"""cudamapper under two-piece gap costs: align_overlaps(..., scoring=<6-tuple>) against
tests/oracle_affine2.py on the slices of a small case whose reads carry one 40-base deletion or one 40-base insertion
against the draft, both strands, independent of the chunking; overlap_variants and polisher.call_variants over those
alignments; the band's capacity; the refusals."""
import random

import numpy as np
import pytest

import affine2_cases as cases
import oracle_affine as O1
import oracle_affine2 as O
import oracle_pileup as OPi
import oracle_variants as OV
import pileup_cases as PC
import variant_cases as VC

pytestmark = pytest.mark.gpu

SCORING = cases.DEFAULT + (64,)
ONE_PIECE = cases.ONE_PIECE + (64,)
SEED = 6                      # chosen so that test_the_case_is_not_vacuous holds
DRAFT, DELETED, INSERTED_AFTER, EVENT = 2000, 900, 1300, 40


def aligner_rc(s):
    """the reverse complement as cudaaligner takes it: "TGAC"[(c >> 1) & 3] for every byte, back to front"""
    return "".join("TGAC"[(ord(c) >> 1) & 3] for c in reversed(s))


def build_case(seed):
    """(reads, [draft], overlap records as tuples): 12 reads of 500-700 draft bases at 4-8 % errors, read k on
    strand "+-"[k % 2]; reads 0-3 lack draft[DELETED : DELETED + 40], reads 4-7 carry 40 bases behind draft[INSERTED_AFTER]"""
    r = random.Random(seed)
    draft = cases.random_sequence(r, DRAFT)
    extra = cases.random_sequence(r, EVENT)
    reads, records = [], []
    for k in range(12):
        around = DELETED if k < 4 else INSERTED_AFTER if k < 8 else r.randrange(600, 1400)
        begin = around - r.randrange(200, 350)
        end = begin + r.randrange(500, 700)
        if k < 4:
            parts = [draft[begin:DELETED], draft[DELETED + EVENT:end]]
        elif k < 8:
            parts = [draft[begin:INSERTED_AFTER + 1], extra, draft[INSERTED_AFTER + 1:end]]
        else:
            parts = [draft[begin:end]]
        if k < 4:  # no errors in the 20 bases on either side of the deletion: every carrier shows the same 40 bases
            parts = [parts[0][:-20], parts[0][-20:] + parts[1][:20], parts[1][20:]]
            read = cases.mutate(r, parts[0], 0.04) + parts[1] + cases.mutate(r, parts[2], 0.04)
        else:      # errors anywhere, at twice the rate next to an insertion: they compete with the long run for its columns
            read = "".join(cases.mutate(r, p, 0.08 if k < 8 else 0.04) for p in parts)
        strand = "+-"[k % 2]
        reads.append(PC.rc(read) if strand == "-" else read)
        records.append((k, 0, 0, begin, len(read), end, ord(strand), 0, 0))
    return reads, [draft], records


def slices(o, reads, drafts):
    out = []
    for x in o:
        q = reads[int(x["query_read_id"])][int(x["query_start_position_in_read"]):int(x["query_end_position_in_read"])]
        t = drafts[int(x["target_read_id"])][int(x["target_start_position_in_read"]):int(x["target_end_position_in_read"])]
        out.append((q, aligner_rc(t) if chr(x["relative_strand"]) == "-" else t))
    return out


def differing(pairs, want):
    """the overlaps whose two-piece CIGAR holds a run of 40 or more and is not the one-piece CIGAR"""
    out = []
    for k, ((q, t), w) in enumerate(zip(pairs, want)):
        if any(L >= EVENT for _, L in O.runs(w["states"])) and O1.align(q, t, *ONE_PIECE)["states"] != w["states"]:
            out.append(k)
    return out


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def case(cm):
    """reads, drafts, overlaps, and the oracle's alignment of every overlap's slices under SCORING, computed once"""
    reads, drafts, records = build_case(SEED)
    o = np.array(records, cm.OVERLAP)
    want = [O.align(q, t, *SCORING) for q, t in slices(o, reads, drafts)]
    return reads, drafts, o, want


def _budgets(cm, o):
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    each = [cm.align_bytes_needed_scored(int(a), int(b), SCORING[5]) for a, b in zip(ql, tl)]
    return max(each), sum(each)


def test_the_case_is_not_vacuous(cm, case):
    # on the CPU, with the oracles alone: the second piece changes at least one CIGAR, and that one holds the whole event
    reads, drafts, o, want = case
    assert {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    assert all(w["states"] is not None and w["optimal"] for w in want)
    assert len(differing(slices(o, reads, drafts), want)) >= 1
    for k in range(8):  # every read that carries an event shows it as one run under the two-piece costs
        assert max(L for _, L in O.runs(want[k]["states"])) >= EVENT


def test_cigars_and_edit_distances_equal_the_oracle(cm, case):
    reads, drafts, o, want = case
    timings = {}
    cigars, edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING, timings=timings)
    assert len(cigars) == len(o)
    for k, (c, d, w) in enumerate(zip(cigars, edits, want)):
        assert c == O.cigar(w["states"]), (k, chr(o[k]["relative_strand"]))
        assert d == sum(1 for s in w["states"] if s != 0), k
    assert timings["align"] > 0
    # a dict is the same scoring
    x, o1, e1, o2, e2, B = SCORING
    again, again_edits = cm.align_overlaps(o, reads, drafts, scoring=dict(mismatch=x, gap_open=o1, gap_extend=e1, gap_open2=o2,
                                                                         gap_extend2=e2, band=B))
    assert again == cigars and again_edits.tobytes() == edits.tobytes()
    defaults, _ = cm.align_overlaps(o, reads, drafts, scoring=dict(gap_open2=o2, gap_extend2=e2, band=B))
    assert defaults == cigars


def test_chunking_does_not_change_the_result(cm, case):
    reads, drafts, o, _ = case
    alone, total = _budgets(cm, o)
    budget = max(alone, total // 5)
    assert total > 4 * budget * 1.1  # more than four chunks
    whole, whole_edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING)
    chunked, chunked_edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING, max_device_bytes=budget)
    assert chunked == whole and chunked_edits.tobytes() == whole_edits.tobytes()
    lone, lone_edits = cm.align_overlaps(o, reads, drafts, scoring=SCORING, max_device_bytes=alone)
    assert lone == whole and lone_edits.tobytes() == whole_edits.tobytes()
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.align_overlaps(o, reads, drafts, scoring=SCORING, max_device_bytes=alone - 1)


def test_the_old_forms_mean_what_they_meant(cm, case):
    reads, drafts, o, _ = case
    plain, plain_edits = cm.align_overlaps(o, reads, drafts)
    none, none_edits = cm.align_overlaps(o, reads, drafts, scoring=None)
    assert none == plain and none_edits.tobytes() == plain_edits.tobytes()
    four, four_edits = cm.align_overlaps(o, reads, drafts, scoring=ONE_PIECE)
    want = [O1.align(q, t, *ONE_PIECE) for q, t in slices(o, reads, drafts)]
    assert four == [O1.cigar(w["states"]) for w in want]
    assert four_edits.tolist() == [sum(1 for s in w["states"] if s != 0) for w in want]
    assert cm.overlap_variants(o, reads, drafts, scoring=None).tobytes() == cm.overlap_variants(o, reads, drafts).tobytes()


def test_variants_are_the_oracle_on_the_calls_own_cigars(cm, case):
    reads, drafts, o, _ = case
    cigars, _ = cm.align_overlaps(o, reads, drafts, scoring=SCORING)
    alignments = OPi.of_cigars(cigars)
    for min_count, min_percent in ((1, 0), (3, 30)):
        got = cm.overlap_variants(o, reads, drafts, min_count, min_percent, scoring=SCORING)
        assert VC.same_records(got, OV.overlap_variants(o, reads, drafts, alignments, "cigar", min_count, min_percent))
        assert len(got) > 0
    alone, _ = _budgets(cm, o)
    assert cm.overlap_variants(o, reads, drafts, 3, 30, scoring=SCORING, max_device_bytes=alone).tobytes() == got.tobytes()


def test_call_variants_reports_the_deletion_as_one_record(cm, case):
    from genomeworks_amd import polisher
    reads, drafts, o, _ = case
    got = polisher.call_variants(reads, drafts, overlaps=o, scoring=SCORING)
    long_ones = [v for v in got if v["kind"] == "deletion" and len(v["ref"]) >= 20]
    assert len(long_ones) == 1
    (v,) = long_ones
    # the run may sit a few bases to either side where the draft repeats itself; it is 40 bases, and what is left joins
    assert len(v["ref"]) == EVENT and abs(v["position"] - DELETED) <= 3 and v["count"] == 4
    assert drafts[0][:v["position"]] + drafts[0][v["position"] + EVENT:] == drafts[0][:DELETED] + drafts[0][DELETED + EVENT:]

    def by_cigar(kept):
        return OPi.of_cigars(cm.align_overlaps(kept, reads, drafts, scoring=SCORING)[0])

    assert got == OV.call_variants(reads, drafts, o, by_cigar)


def test_a_band_over_the_capacity_gives_no_cigar(cm, case):
    reads, drafts, o, _ = case
    few = o[8:12].copy()  # the reads without an event: |m - n| of a few bases
    few[1]["query_end_position_in_read"] -= 100  # |m - n| of about 100: W > 1024 at B = 480; the others stay below
    wide = cases.DEFAULT + (480,)
    want = [O.align(q, t, *wide) for q, t in slices(few, reads, drafts)]
    assert [w["states"] is None for w in want] == [False, True, False, False]
    cigars, edits = cm.align_overlaps(few, reads, drafts, scoring=wide)
    assert cigars == [O.cigar(w["states"]) if w["states"] is not None else "" for w in want]
    assert edits.tolist() == [sum(1 for s in w["states"] if s != 0) if w["states"] is not None else -1 for w in want]
    # every overlap over the capacity: no CIGAR anywhere, no records, no fault; the one-piece aligner still takes the band
    cigars, edits = cm.align_overlaps(o, reads, drafts, scoring=cases.DEFAULT + (512,))
    assert cigars == [""] * len(o) and edits.tolist() == [-1] * len(o)
    assert len(cm.overlap_variants(o, reads, drafts, 1, 0, scoring=cases.DEFAULT + (512,))) == 0
    assert all(cm.align_overlaps(o, reads, drafts, scoring=cases.ONE_PIECE + (512,))[0])


def test_refusals(cm, case):
    from genomeworks_amd import _native, polisher
    reads, drafts, o, want = case
    for bad in ((0, 4, 3, 24, 2, 64), (6, 4, 3, -1, 2, 64), (6, 4, 3, 256, 2, 64), (6, 4, 3, 24, 0, 64), (6, 4, 3, 24, 256, 64),
                (6, 4, 3, 24, 2, -1), (6, 4, 3, 24, 2), dict(gap_open2=24), dict(gap_extend2=2)):
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
    for bad in ((0, 4, 3, 24, 2, 64), (6, 256, 3, 24, 2, 64), (6, 4, 3, 256, 2, 64), (6, 4, 3, 24, 0, 64), (6, 4, 3, 24, 2, -1)):
        sc = np.array(bad, np.int32)
        assert not L.gw_mapper_align_overlaps_scored2(cm._p(records), len(records), *q, 0, *t, 0, cm._p(sc), 0, None)
        assert "scoring" in L.gw_mapper_last_error().decode()
        assert not L.gw_mapper_overlap_variants_scored2(cm._p(records), len(records), *q, 0, *t, 0, 3, 30, cm._p(sc), 0, None)
        assert "scoring" in L.gw_mapper_last_error().decode()
    bad = o.copy()
    bad[2]["target_end_position_in_read"] = 10 ** 7
    with pytest.raises(cm.MapperError):
        cm.align_overlaps(bad, reads, drafts, scoring=SCORING)
    # and the next call is whole
    cigars, _ = cm.align_overlaps(o[:6], reads, drafts, scoring=SCORING)
    assert cigars == [O.cigar(w["states"]) for w in want[:6]]
