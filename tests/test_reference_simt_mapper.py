"""The cudamapper oracle (tests/oracle_mapper.c) against the REFERENCE's own kernels run on the CPU emulator of
oracle/simt: the committed fixtures tests/golden/cudamapper_reference_simt.npz / .json (written by
tests/golden/make_mapper_reference_simt_goldens.py) stage by stage, the record of the one-off check of the covid
goldens, and -- where oracle/_ref/libref_cudamapper_simt.so exists -- a small fresh-seed sample, reference against oracle.

Directions: for a read of more than one central step the reference's direction of some elements is a byte of a window
position (its direction array is overrun: oracle_mapper.c, oracle/simt/README.md). The fixtures hold what the reference
gives and the oracle reproduces it in REFERENCE_DIRECTIONS mode; in TRUE_DIRECTIONS mode, which the GPU path is held to,
it differs from that in exactly the elements it marks in ALIASED_DIRECTIONS mode."""
import hashlib
import json

import numpy as np
import pytest

import mapper_cases as MC
import oracle_mapper as O
import ref_cudamapper as R


@pytest.fixture(scope="module")
def fx():
    return MC.Fixture()


@pytest.fixture(scope="module")
def described():
    with open(MC.REFERENCE_SIMT_JSON) as f:
        return json.load(f)["cases"]


def strip(case):
    return {k: v for k, v in case.items() if k != "fill_dependent"}


def test_fixture_describes_every_case(fx, described):
    cases = MC.reference_simt_cases()
    assert [strip(c) for c in described] == cases  # class, k, w, hash and seed per case, as the generators give them today
    assert not any(c["fill_dependent"] for c in described)
    classes = {(c["stage"], c["cls"]) for c in cases}
    for cls in ("multi_step", "step_boundary", "stale_carry", "w1", "end_steps", "exact_length", "short_among_long", "ties",
                "non_acgt", "k16", "filter", "all_filtered"):
        assert ("index", cls) in classes
        assert {c["hash"] for c in cases if c["cls"] == cls} == {True, False}, cls
    assert {cls for stage, cls in classes if stage == "matcher"} == set(MC.MATCHER_CLASSES)
    assert all(c["k"] <= 16 for c in cases if "k" in c)  # the emulator does not judge k >= 17
    assert all((c["k"] + c["w"]) % 64 == 2 for c in cases if c["cls"] == "stale_carry")
    for c in cases:
        if c["cls"] == "step_boundary":
            s, one = MC.central_step(c["k"], c["w"]), c["k"] + c["w"] - 1
            assert fx.meta[c["name"] + "/lengths"] == [one - 1 + n for n in (1, s - 1, s, s + 1, 2 * s + 1)]


def index_cases():
    return [c for c in MC.reference_simt_cases() if c["stage"] == "index"]


@pytest.mark.parametrize("case", index_cases(), ids=lambda c: c["name"])
def test_oracle_reproduces_reference_index(fx, case):
    reads = MC.index_case_reads(case["cls"], case["k"], case["w"], case["seed"])
    p = case["name"] + "/"
    MC.fixture_check(fx, p + "bases", np.frombuffer(b"".join(reads), np.uint8), "inputs")
    args = (reads, case["k"], case["w"], case["hash"], case["F"], case["first_read_id"])
    ref_mode = O.index(*args, direction_mode=O.REFERENCE_DIRECTIONS)
    MC.fixture_check_index(fx, p, ref_mode, case["name"])
    true_mode, aliased = O.index(*args), O.index(*args, direction_mode=O.ALIASED_DIRECTIONS)["directions"]
    assert set(np.unique(true_mode["directions"]).tolist()) <= {0, 1}
    keep = aliased == 0
    np.testing.assert_array_equal(true_mode["directions"][keep], ref_mode["directions"][keep])
    for name in MC.INDEX_ARRAY_NAMES:
        if name != "directions":
            np.testing.assert_array_equal(true_mode[name], ref_mode[name])


def test_fixtures_reach_the_rules_they_are_there_for(fx):
    """the stale carry re-emits, the filter cases sit on their threshold, short reads shift the ids, directions alias"""
    cases = index_cases()
    aliased = 0
    for c in cases:
        reads = MC.index_case_reads(c["cls"], c["k"], c["w"], c["seed"])
        if c["cls"] == "stale_carry":
            s = O.sketch(reads, c["k"], c["w"], c["hash"])
            key = s["read_ids"].astype(np.int64) << 32 | s["positions_in_reads"]
            assert len(np.unique(key)) < len(key), c["name"]  # an element emitted again at a step boundary
        if c["cls"] == "filter":
            full = O.index(reads, c["k"], c["w"], c["hash"], 1.0)
            counts = np.diff(full["first_occurrence_of_representations"].astype(np.int64))
            threshold = int(len(full["representations"]) * c["F"] + 0.001)
            assert threshold in counts and threshold - 1 in counts, c["name"]
        if c["cls"] == "all_filtered":
            assert fx.meta[c["name"] + "/representations"][0] == 0 and fx.meta[c["name"] + "/scalars"][0] > 0
        if c["cls"] == "short_among_long":
            long_enough = sum(len(r) >= c["k"] + c["w"] - 1 for r in reads)
            assert 0 < long_enough < len(reads)
            assert fx.meta[c["name"] + "/scalars"][:3] == [len(reads), c["first_read_id"], c["first_read_id"] + len(reads) - 1]
        aliased += bool(O.index(reads, c["k"], c["w"], c["hash"], direction_mode=O.ALIASED_DIRECTIONS)["directions"].any())
    assert aliased >= 10  # cases with elements whose reference direction is a byte of a window position


def matcher_cases():
    return [c for c in MC.reference_simt_cases() if c["stage"] == "matcher"]


@pytest.mark.parametrize("case", matcher_cases(), ids=lambda c: c["name"])
def test_oracle_reproduces_reference_anchors(fx, case):
    p = case["name"] + "/"
    q, t = MC.fixture_index(fx, p + "query/"), MC.fixture_index(fx, p + "target/")  # the reference's indices
    a = O.anchors(q, t)
    MC.fixture_check(fx, p + "anchors", a, case["name"])
    # and the indices themselves, where they come from reads
    for name, s in zip(("query", "target"), MC.matcher_case_inputs(case["cls"], case["k"], case["w"], case["hash"], case["seed"])):
        if s is not None and "reads" in s:
            idx = O.index(s["reads"], case["k"], case["w"], case["hash"], 1.0, s["first_read_id"], O.REFERENCE_DIRECTIONS)
            MC.fixture_check_index(fx, p + name + "/", idx, case["name"] + " " + name)
        elif s is not None:
            MC.fixture_check_index(fx, p + name + "/", s["index"], case["name"] + " " + name)
    if case["cls"] == "block_300x300":
        assert len(a) >= 90000
    if case["cls"] == "wide_position_key":
        assert q["number_of_basepairs_in_longest_read"] * t["number_of_basepairs_in_longest_read"] > 1 << 32 and len(a) > 0
    if case["cls"] in ("disjoint", "query_empty", "target_empty"):
        assert len(a) == 0
    if case["cls"] in ("self", "first_read_ids"):
        assert len(a) > 0


def overlapper_cases():
    return [c for c in MC.reference_simt_cases() if c["stage"] == "overlapper"]


@pytest.mark.parametrize("case", overlapper_cases(), ids=lambda c: c["name"])
def test_oracle_reproduces_reference_overlaps(fx, case):
    p = case["name"] + "/"
    anchors = MC.overlapper_case_input(case)
    MC.fixture_check(fx, p + "anchors", anchors, "inputs")
    o = O.overlaps(anchors, case["all_to_all"], **MC.OVERLAPPER_FILTERS[case["filter"]])
    assert len(o) == fx.meta[p + "n_overlaps"], case["name"]
    MC.fixture_check(fx, p + "overlaps", np.frombuffer(MC.overlap_bytes(o), np.uint8), case["name"])


@pytest.mark.parametrize("case", [c for c in MC.reference_simt_cases() if c["stage"] == "map"], ids=lambda c: c["name"])
def test_oracle_reproduces_reference_end_to_end(fx, case):
    p = case["name"] + "/"
    queries, targets = MC.map_case_reads(case)
    MC.fixture_check(fx, p + "bases", np.frombuffer("".join(queries + (targets or [])).encode(), np.uint8), "inputs")
    o = O.map_reads(queries, targets, case["k"], case["w"], case["F"], **MC.OVERLAPPER_FILTERS[case["filter"]])
    assert len(o) == fx.meta[p + "n_overlaps"] and len(o) > 0, case["name"]
    MC.fixture_check(fx, p + "overlaps", np.frombuffer(MC.overlap_bytes(o), np.uint8), case["name"])


def test_overlapper_cases_sit_on_both_sides_of_every_condition():
    """chains of 2, 3 and 4 anchors, steps of 148..151, fusion distances of 298..301, falling targets, self pairs; every
    filter keeps some overlaps and drops others by each of its conditions"""
    for seed, n in ((400, 3000), (401, 4000), (402, 2500)):
        a = MC.overlapper_case_anchors(seed, n)
        same_pair = (a["query_read_id"][1:] == a["query_read_id"][:-1]) & (a["target_read_id"][1:] == a["target_read_id"][:-1])
        dq = (a["query_position_in_read"][1:].astype(np.int64) - a["query_position_in_read"][:-1])[same_pair]
        dt = (a["target_position_in_read"][1:].astype(np.int64) - a["target_position_in_read"][:-1])[same_pair]
        assert {148, 149, 150, 151} <= set(dq.tolist()) and {148, 149, 150, 151} <= set(np.abs(dt).tolist())
        assert (dt < 0).any() and (dt > 0).any() and (a["query_read_id"] == a["target_read_id"]).any()
        unfiltered = O.overlaps(a, False, 0, 0, 1 << 40, -1.0)
        assert {3, 4} <= set(unfiltered["num_residues"].tolist()) and (unfiltered["num_residues"] > 4).any()
        assert len(O.overlaps(a, True, 0, 0, 1 << 40, -1.0)) < len(unfiltered)  # self pairs go with all_to_all only
        tl = unfiltered["target_end_position_in_read"].astype(np.int64) - unfiltered["target_start_position_in_read"]
        ql = unfiltered["query_end_position_in_read"].astype(np.int64) - unfiltered["query_start_position_in_read"]
        length, res = np.maximum(tl, ql), unfiltered["num_residues"].astype(np.int64)
        for filt in MC.OVERLAPPER_FILTERS:
            conditions = [res >= filt["min_residues"], length // res < filt["min_bases_per_residue"],
                          np.minimum(ql, tl) >= filt["min_overlap_len"],
                          np.minimum(ql, tl).astype(np.float32) / length.astype(np.float32) > np.float32(filt["min_overlap_fraction"])]
            assert np.all(conditions, axis=0).any(), filt
            assert sum((~c).any() for c in conditions) >= 2, filt
        assert any((~c).any() for c in [res >= 6]) and any((length // res >= 75).tolist())


def test_covid_goldens_were_checked_against_the_reference():
    with open(MC.REFERENCE_SIMT_CHECK) as f:
        record = json.load(f)
    golden = np.load(MC.COVID_NPZ)
    assert [(c["k"], c["w"], c["F"]) for c in record["configs"]] == [(c["k"], c["w"], c["F"]) for c in MC.COVID_CONFIGS]
    for c in record["configs"]:
        key = "w%d_F%g" % (c["w"], c["F"])
        assert c["agrees"] is True
        assert c["n_elements"] == int(golden[key + "_n_elements"])
        assert c["n_anchors"] == int(golden[key + "_n_anchors"])
        assert c["n_overlaps"] == int(golden[key + "_n_overlaps"])
        assert c["overlaps_sha256"] == str(golden[key + "_overlaps_sha256"])


# ---- live: fresh seeds, reference against oracle (skips where the library is absent) ----------------------------------

needs_library = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libref_cudamapper_simt.so is not built (no reference checkout)")


@needs_library
@pytest.mark.parametrize("seed", range(6))
def test_live_reference_against_oracle(seed):
    rng = np.random.default_rng(9000 + seed)
    k, w = [(15, 10), (15, 51), (16, 50), (11, 1), (7, 60), (13, 24)][seed]
    h = bool(seed % 2)
    reads = MC.synthetic_reads(9000 + seed, 3000, 3, 900, 0.04) + [MC._random_bases(rng, 1700, b"ACGTN"), b"AC" * 600]
    half = len(reads) // 2
    F = [1.0, 0.01][seed % 2]
    rq, rt = R.index(reads[:half], k, w, h, F), R.index(reads[half:], k, w, h, F, half)
    oq = O.index(reads[:half], k, w, h, F, 0, O.REFERENCE_DIRECTIONS)
    ot = O.index(reads[half:], k, w, h, F, half, O.REFERENCE_DIRECTIONS)
    for r, o in ((rq, oq), (rt, ot)):
        for name in MC.INDEX_ARRAY_NAMES:
            np.testing.assert_array_equal(r[name], o[name], err_msg=name)
        assert [r[n] for n in MC.INDEX_SCALAR_NAMES] == [o[n] for n in MC.INDEX_SCALAR_NAMES]
    ra = R.anchors(rq, rt)
    np.testing.assert_array_equal(ra, O.anchors(oq, ot))
    anchors = MC.overlapper_case_anchors(9100 + seed, 1500)
    for a in (ra, anchors):
        for filt in MC.OVERLAPPER_FILTERS[:3]:
            assert MC.overlap_bytes(R.overlaps(a, False, **filt)) == MC.overlap_bytes(O.overlaps(a, False, **filt))
