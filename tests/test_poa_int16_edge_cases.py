"""The windows of poa_int16_edge_cases.py on the CPU: for every one of them the reference's answer is well defined -- the
configuration selects int16 scores, the oracle ends with status 0 and no overflow event -- so the GPU test
(test_gpu_poa_int16_edges.py) may demand bit-exact equality at the edges of the packed passes' admission bounds. Also pins
the placement of the inputs (the computed edges), the flip of the consensus at the uint16 wrap of the edge weights, and the
reference's own answer for the heavy-weight windows (tests/golden/reference_simt_heavy_weights.json)."""
import json
import os

import pytest

import poa_int16_edge_cases as E

SCORE_CASES, WEIGHT_CASES = E.all_cases()
HERE = os.path.dirname(os.path.abspath(__file__))


def ids(cases):
    return [c["id"] for c in cases]


def test_case_ids_are_unique_and_the_windows_stay_small():
    all_ids = ids(SCORE_CASES + WEIGHT_CASES)
    assert len(set(all_ids)) == len(all_ids)
    assert all(len(c["reads"]) <= 6 for c in SCORE_CASES)
    assert all(len(r) <= c["config"]["max_seq"] for c in SCORE_CASES + WEIGHT_CASES for r in c["reads"])
    assert all(len(c["reads"]) <= c["config"]["max_seqs"] for c in SCORE_CASES + WEIGHT_CASES)


@pytest.mark.parametrize("mode,width,max_seq,match,last_admitted", [
    ("static_band", 256, 1024, 31, 1022), ("adaptive_band", 256, 1024, 31, 1022), ("static_band_traceback", 256, 1024, 31, 1022),
    ("static_band", 512, 1024, 31, 989), ("full_band", 256, 1024, 31, 923), ("static_band", 128, 512, 63, 502),
    ("static_band", 256, 328, 99, 319)])
def test_computed_edges_of_the_upper_bound(mode, width, max_seq, match, last_admitted):
    """Guards the input placement, not the kernel: the restatement of (A) puts the edges where the bounds in the device code,
    worked out by hand, put them; and the sweep has windows on both sides of each."""
    cfg = E.make_config(mode, width, max_seq, -4, -6, match)
    assert E.last_admitted_identical(cfg) == last_admitted
    assert E.lhs_a(cfg, last_admitted, last_admitted) <= 32767 < E.lhs_a(cfg, last_admitted + 1, last_admitted + 1)
    swept = sorted(c["read_length"] for c in SCORE_CASES if c["config"] == cfg and c["identical"])
    assert swept[:5] == list(range(last_admitted - 2, last_admitted + 3))


def test_computed_edges_of_the_lower_bound():
    cases = [c for c in SCORE_CASES if c["kind"] == "B"]
    assert len(cases) == 5 * 5
    for c in cases:
        assert c["graph_count"] > 512  # the five reads really are unrelated: the graph has outgrown the longest read
    for mode in E.BAND_MODES:
        sweep = [c for c in cases if c["config"]["band_mode"] == mode]
        G = sweep[0]["graph_count"]
        assert [c["graph_count"] + c["read_length"] for c in sweep] == [1546, 1547, 1548, 1549, 1550], (mode, G)
        assert [E.lhs_b(c["config"], c["read_length"], G) >= -32768 + 256 for c in sweep] == [True, True, True, False, False]


@pytest.mark.parametrize("case", SCORE_CASES + WEIGHT_CASES, ids=ids(SCORE_CASES + WEIGHT_CASES))
def test_the_oracle_answer_is_well_defined(case):
    ref = E.oracle_result(case)
    assert ref["score32"] == 0
    assert ref["status"] == 0
    assert ref["overflow"] == 0
    if case["identical"]:
        assert ref["consensus"] == case["reads"][0]
        assert list(ref["coverage"]) == [len(case["reads"])] * len(case["reads"][0])


def test_lower_bound_windows_reach_the_edge_with_the_graph_the_placement_assumed():
    """The sixth read of a (B) window meets the graph of the first five: the window's final node count is at least that G."""
    for c in SCORE_CASES:
        if c["kind"] == "B":
            assert E.oracle_result(c)["node_count"] >= c["graph_count"]


def by_id(cid):
    return next(c for c in WEIGHT_CASES if c["id"] == cid)


@pytest.mark.parametrize("mode,width", E.WEIGHT_MODES)
@pytest.mark.parametrize("suffix", ["", "_two_branches"])
def test_consensus_flips_where_the_heaviest_edge_wraps(mode, width, suffix):
    """258 reads of r: edge weight 65 532, the consensus is r. 259: 65 786 wraps to 250 as the reference's uint16 does, below the
    25 400 of the 100 reads of v, and the consensus is v."""
    name = E.label(dict(band_mode=mode, band_width=width))
    below = by_id("W_%s_r258_v100_sum65532%s" % (name, suffix))
    above = by_id("W_%s_r259_v100_sum65786%s" % (name, suffix))
    assert E.oracle_result(below)["consensus"] == below["r"] != below["v"]
    assert E.oracle_result(above)["consensus"] == above["v"]


@pytest.mark.parametrize("mode,width", E.WEIGHT_MODES)
def test_edge_weights_above_int16_keep_their_sign(mode, width):
    name = E.label(dict(band_mode=mode, band_width=width))
    c = by_id("W_%s_r140_v120_sum35560" % name)
    assert E.oracle_result(c)["consensus"] == c["r"]
    c = by_id("W_%s_r110_v90_phred60to93" % name)
    assert E.oracle_result(c)["consensus"] == c["r"]


def reference_fixture():
    with open(os.path.join(HERE, "golden", "reference_simt_heavy_weights.json")) as f:
        return json.load(f)["windows"]


@pytest.mark.parametrize("case", WEIGHT_CASES, ids=ids(WEIGHT_CASES))
def test_heavy_weight_windows_equal_the_reference_itself(case):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_reference_simt_heavy_weights as M
    fixture = reference_fixture()
    assert set(fixture) == set(ids(WEIGHT_CASES))
    want, ref = fixture[case["id"]], E.oracle_result(case)
    assert want["reads_sha256"] == M.digest(case)  # the fixture belongs to these reads
    assert (want["status"], want["consensus"], want["coverage"]) == (ref["status"], ref["consensus"], [int(x) for x in ref["coverage"]])
