"""The CPU oracle of cudamapper's overlap post-processing (tests/oracle_mapper_postprocess.py) against the reference's
own answers: the hand-transcribed cases of its tests (cudamapper_postprocess_vectors.json) and what its
post_process_overlaps / rescue_overlap_ends returned on seeded inputs (cudamapper_postprocess_reference.npz), record
for record. The branch counts make sure the recorded inputs keep reaching every rule."""
import numpy as np
import pytest

import mapper_postprocess_cases as PC
import oracle_mapper as O
import oracle_mapper_postprocess as P


@pytest.fixture(scope="module")
def vectors():
    return PC.load_vectors()


@pytest.fixture(scope="module")
def golden():
    return PC.load_reference()


# ---- the reference's tests -----------------------------------------------------------------------------------------

def test_post_process_vectors(vectors):
    for case in vectors["post_process"]:
        out = P.post_process_overlaps(PC.overlaps_from_dicts(case["overlaps"]))
        assert len(out) == case["expected_count"], case["source"]


def test_extension_vector(vectors):
    for case in vectors["extension"]:
        o = case["overlap"]
        s = dict(qs=o["query_start_position_in_read"], qe=o["query_end_position_in_read"],
                 ts=o["target_start_position_in_read"], te=o["target_end_position_in_read"])
        P.extend_overlap_by_sequence_similarity(s, case["query"].encode(), case["target"].encode(), case["extension"],
                                                case["required_similarity"])
        e = case["expected"]
        assert (s["qs"], s["ts"], s["qe"], s["te"]) == (
            e["query_start_position_in_read"], e["target_start_position_in_read"], e["query_end_position_in_read"],
            e["target_end_position_in_read"]), case["source"]


def test_drop_by_mask_vectors(vectors):
    for case in vectors["drop_by_mask"]:
        o = np.zeros(len(case["query_read_ids"]), O.OVERLAP)
        o["query_read_id"] = case["query_read_ids"]
        out = P.drop_overlaps_by_mask(o, case["mask"])
        assert out["query_read_id"].tolist() == case["expected_query_read_ids"], case["source"]


def test_kmer_vectors(vectors):
    for case in vectors["kmers"]:
        k = P.split_into_kmers(case["sequence"], case["kmer_size"], case["stride"])
        assert (len(k), k[0], k[-1]) == (case["expected_count"], case["expected_first"], case["expected_last"])
    for case in vectors["shared"]:
        assert P.count_shared_elements(sorted(case["a"]), sorted(case["b"])) == case["expected"], case["source"]
    for case in vectors["similarity"]:
        s = P.sequence_jaccard_similarity(case["a"], case["b"], case["kmer_size"], case["stride"])
        assert {"== 1": s == 1.0, "== 0": s == 0.0, "between 0 and 1": 0.0 < s < 1.0}[case["expected"]], case["source"]


def test_grouping_vectors(vectors):
    for case in vectors["grouping"]:
        lengths = [len(s) for s in PC.fasta_reads(case["fasta"])]
        got = P.group_reads_into_indices(lengths, case["max_basepairs_per_index"])
        assert [list(d) for d in got] == case["expected"], case["source"]


def test_grouping_corner_cases():
    assert P.group_reads_into_indices([], 10) == [(0, 0)]
    assert P.group_reads_into_indices([11, 3], 10) == [(0, 0), (0, 1), (1, 1)]
    assert P.group_reads_into_indices([10, 1], 10) == [(0, 1), (1, 1)]
    assert P.group_reads_into_indices([4, 6, 20, 1], 10) == [(0, 2), (2, 1), (3, 1)]


# ---- what the reference's functions returned -----------------------------------------------------------------------

@pytest.mark.parametrize("case", PC.CASES)
def test_post_process_equals_reference(golden, case):
    o = golden[case + "_overlaps"]
    assert np.array_equal(P.post_process_overlaps(o), golden[case + "_post"])
    assert np.array_equal(P.post_process_overlaps(o, True), golden[case + "_post_drop"])


@pytest.mark.parametrize("case", PC.RESCUE_CASES)
def test_rescue_equals_reference(golden, case):
    q, t = PC.reads_of(golden, case)
    assert np.array_equal(P.rescue_overlap_ends(golden[case + "_overlaps"], q, t, 50, 0.5), golden[case + "_rescue"])
    assert np.array_equal(P.rescue_overlap_ends(golden[case + "_post"], q, t, 50, 0.5), golden[case + "_post_rescue"])


def test_fixture_reaches_every_fusion_branch(golden):
    o = golden["fuse_overlaps"]
    assert len(o) + len(golden["rescue_overlaps"]) >= 200
    alone = {"+": [0, 0, 0, 0], "-": [0, 0, 0, 0]}  # short only, ratio only, relative only, none
    other_pair = other_strand = 0
    for a, b in zip(o[:-1], o[1:]):
        c = P.merge_conditions(a, b)
        if c is None:
            other_pair += a["relative_strand"] == b["relative_strand"]
            other_strand += a["relative_strand"] != b["relative_strand"]
            continue
        s = chr(int(a["relative_strand"]))
        if sum(c) == 1:
            alone[s][c.index(True)] += 1
        elif sum(c) == 0:
            alone[s][3] += 1
    for s in "+-":
        assert all(n > 0 for n in alone[s]), (s, alone[s])
    assert other_pair > 0 and other_strand > 0
    flags = P.mergable_flags(o)
    runs, n = [], 0
    for f in list(flags) + [False]:
        if f:
            n += 1
        elif n:
            runs.append(n + 1)
            n = 0
    assert 2 in runs and 3 in runs and max(runs) > 3, runs
    assert flags[-1] and flags[-2], "the array must end inside a run"
    assert not flags[0] or not all(flags), "and some run must end before it"
    # the run that ends the array takes its fields from the second to last member
    last = golden["fuse_post"][-1]
    assert (int(last["num_residues"]), int(last["overlap_complete"])) == (7 + 8 + 9, int(o[-2]["overlap_complete"]))
    assert int(o[-2]["overlap_complete"]) != int(o[-1]["overlap_complete"])
    # and the mapped set fuses too
    assert len(golden["mapped_post"]) > len(golden["mapped_overlaps"]) > len(golden["mapped_post_drop"]) > 0
    assert set(np.unique(golden["mapped_overlaps"]["relative_strand"]).tolist()) == {ord("+"), ord("-")}


def test_fixture_reaches_every_rescue_branch(golden):
    q, t = PC.reads_of(golden, "rescue")
    o = golden["rescue_overlaps"]
    trace = []
    out = P.rescue_overlap_ends(o, q, t, 50, 0.5, trace=trace)
    bins = lambda w: 0 if w == 0 else 1 if w < 15 else 2 if w < 50 else 3
    for strand in (ord("+"), ord("-")):
        head, tail = set(), set()
        moved_rounds = {"round 1 only": 0, "all three": 0, "never": 0}
        for rec, rounds in zip(o, trace):
            if rec["relative_strand"] != strand:
                continue
            assert len(rounds) == 3  # the early exit never fires on these
            head.update(bins(r[2]) for r in rounds)
            tail.update(bins(r[3]) for r in rounds)
            for end, size in ((0, 2), (1, 3)):
                real = [r[end] and r[size] > 0 for r in rounds]
                if real == [True, False, False]:
                    moved_rounds["round 1 only"] += 1
                elif all(real):
                    moved_rounds["all three"] += 1
                elif not any(real):
                    moved_rounds["never"] += 1
        assert head == {0, 1, 2, 3} and tail == {0, 1, 2, 3}, (head, tail)
        assert all(n > 0 for n in moved_rounds.values()), moved_rounds
    # similarity exactly 0.5 on a full window: 24 shared of 36 + 36 - 24
    exact = 0
    for rec in o:
        qr, tr = q[int(rec["query_read_id"])], t[int(rec["target_read_id"])]
        if rec["relative_strand"] == ord("-"):
            continue
        a, b = int(rec["query_start_position_in_read"]), int(rec["target_start_position_in_read"])
        if min(a, b) >= 50:
            exact += P.sequence_jaccard_similarity(qr[a - 50:a], tr[b - 50:b], 15) == 0.5
    assert exact > 0
    assert any(b"N" in r for r in q)
    assert any(rec["query_start_position_in_read"] == rec["query_end_position_in_read"] for rec in o)
    # the uncomplemented middle base of an odd-length '-' target matters to some record
    plain = P.reverse_complement
    try:
        P.reverse_complement = lambda s: s.translate(P._COMP)[::-1]
        assert not np.array_equal(P.rescue_overlap_ends(o, q, t, 50, 0.5), out)
    finally:
        P.reverse_complement = plain


def test_rescue_rejects_what_the_reference_leaves_undefined():
    reads = [b"ACGT" * 30, b"ACGT" * 20]
    ok = PC.overlaps_from_dicts([dict(query_read_id=0, target_read_id=1, query_start_position_in_read=10,
                                      query_end_position_in_read=60, target_start_position_in_read=10,
                                      target_end_position_in_read=60, relative_strand="+")])
    P.rescue_overlap_ends(ok, reads, reads)
    for field, value in (("target_end_position_in_read", 81), ("query_end_position_in_read", 121),
                         ("target_read_id", 2), ("query_read_id", 7), ("query_start_position_in_read", 200)):
        bad = ok.copy()
        bad[field] = value
        with pytest.raises(ValueError):
            P.rescue_overlap_ends(bad, reads, reads)


def test_format_paf_line():
    o = PC.overlaps_from_dicts([dict(query_read_id=1, target_read_id=0, query_start_position_in_read=5,
                                     query_end_position_in_read=405, target_start_position_in_read=100,
                                     target_end_position_in_read=520, relative_strand="-", num_residues=12)])
    text = P.format_paf(o, ["a", "b"], [1000, 900], ["a", "b"], [1000, 900], 15)
    assert text == "b\t900\t5\t405\t-\ta\t1000\t100\t520\t180\t420\t255\n"
