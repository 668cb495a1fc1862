"""cudamapper on the GPU against the REFERENCE's own kernels: the fixtures tests/golden/cudamapper_reference_simt.npz
(the reference's minimizer, index, matcher and overlapper sources run on a CPU emulator, written by
tests/golden/make_mapper_reference_simt_goldens.py) through cm.Index, cm.Matcher / cm.find_anchors, cm.find_overlaps and
cm.map_reads. Every case is also compared with the oracle array by array first, so that a fixture array stored as a
digest still gives a readable first difference. Reads only tests/golden/.

Directions: the reference's direction array of a central step is overrun, and for some elements of reads of more than
one central step it returns a byte of a window position instead (tests/oracle_mapper.c). The GPU path gives the strand
(0 / 1), which its packed host copy stores in one bit. It is held to the fixture through the oracle: equal to the
oracle's TRUE_DIRECTIONS everywhere, which equal its REFERENCE_DIRECTIONS outside the elements it marks as aliased,
which are the fixture's."""
import numpy as np
import pytest

import mapper_cases as MC
import oracle_mapper as O

pytestmark = pytest.mark.gpu

GPU_NAMES = {"directions": "directions_of_reads"}
CASES = MC.reference_simt_cases()


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def fx():
    return MC.Fixture()


def gpu_index_dict(index):
    d = {name: getattr(index, GPU_NAMES.get(name, name)) for name in MC.INDEX_ARRAY_NAMES}
    d.update((name, getattr(index, name)) for name in MC.INDEX_SCALAR_NAMES)
    return d


def check_index_against_fixture(fx, prefix, gpu, reads, k, w, h, F, first_read_id, where):
    args = (reads, k, w, h, F, first_read_id)
    true_mode = O.index(*args)
    ref_mode = O.index(*args, direction_mode=O.REFERENCE_DIRECTIONS)
    aliased = O.index(*args, direction_mode=O.ALIASED_DIRECTIONS)["directions"]
    for name in MC.INDEX_ARRAY_NAMES:  # the oracle first: a readable difference
        np.testing.assert_array_equal(gpu[name], true_mode[name], err_msg="%s %s" % (where, name))
    MC.fixture_check_index(fx, prefix, gpu, where, skip=("directions",))
    MC.fixture_check(fx, prefix + "directions", ref_mode["directions"], where)
    keep = aliased == 0
    np.testing.assert_array_equal(gpu["directions"][keep], ref_mode["directions"][keep], err_msg=where + " directions")
    if prefix + "directions" in fx.files:
        np.testing.assert_array_equal(gpu["directions"][keep], fx[prefix + "directions"][keep], err_msg=where + " directions")
    assert set(np.unique(gpu["directions"]).tolist()) <= {0, 1}, where


@pytest.mark.parametrize("case", [c for c in CASES if c["stage"] == "index"], ids=lambda c: c["name"])
def test_index_reproduces_reference(cm, fx, case):
    reads = MC.index_case_reads(case["cls"], case["k"], case["w"], case["seed"])
    index = cm.Index(reads, case["k"], case["w"], case["hash"], case["F"], case["first_read_id"])
    check_index_against_fixture(fx, case["name"] + "/", gpu_index_dict(index), reads, case["k"], case["w"], case["hash"],
                                case["F"], case["first_read_id"], case["name"])
    index.close()


def index_from_fixture(cm, idx):
    return cm.Index.from_arrays(idx["read_ids"], idx["positions_in_reads"], idx["unique_representations"],
                                idx["first_occurrence_of_representations"], idx["smallest_read_id"], idx["number_of_reads"],
                                idx["number_of_basepairs_in_longest_read"])


@pytest.mark.parametrize("case", [c for c in CASES if c["stage"] == "matcher"], ids=lambda c: c["name"])
def test_matcher_reproduces_reference(cm, fx, case):
    p = case["name"] + "/"
    q, t = MC.fixture_index(fx, p + "query/"), MC.fixture_index(fx, p + "target/")
    expected = O.anchors(q, t)
    # the reference's indices, handed over as arrays
    a = cm.find_anchors(index_from_fixture(cm, q), index_from_fixture(cm, t))
    np.testing.assert_array_equal(a, expected, err_msg=case["name"])
    MC.fixture_check(fx, p + "anchors", a, case["name"])
    # and the indices built on the GPU from the reads, through a Matcher
    sides = MC.matcher_case_inputs(case["cls"], case["k"], case["w"], case["hash"], case["seed"])
    if all(s is None or "reads" in s for s in sides):
        built = []
        for name, s in zip(("query", "target"), sides):
            if s is None:
                built.append(built[0])
                continue
            index = cm.Index(s["reads"], case["k"], case["w"], case["hash"], 1.0, s["first_read_id"])
            check_index_against_fixture(fx, p + name + "/", gpu_index_dict(index), s["reads"], case["k"], case["w"], case["hash"], 1.0,
                                        s["first_read_id"], case["name"] + " " + name)
            built.append(index)
        m = cm.Matcher(built[0], built[1])
        MC.fixture_check(fx, p + "anchors", m.anchors(), case["name"] + " from reads")
        m.close()


@pytest.mark.parametrize("case", [c for c in CASES if c["stage"] == "overlapper"], ids=lambda c: c["name"])
def test_overlapper_reproduces_reference(cm, fx, case):
    p = case["name"] + "/"
    anchors = MC.overlapper_case_input(case)
    MC.fixture_check(fx, p + "anchors", anchors, "inputs")
    filt = MC.OVERLAPPER_FILTERS[case["filter"]]
    o = cm.find_overlaps(np.ascontiguousarray(anchors, cm.ANCHOR), case["all_to_all"], **filt)
    expected = O.overlaps(anchors, case["all_to_all"], **filt)
    assert len(o) == len(expected) == fx.meta[p + "n_overlaps"], case["name"]
    for name in O.OVERLAP.names:
        np.testing.assert_array_equal(o[name], expected[name], err_msg="%s %s" % (case["name"], name))
    MC.fixture_check(fx, p + "overlaps", np.frombuffer(MC.overlap_bytes(o), np.uint8), case["name"])


@pytest.mark.parametrize("case", [c for c in CASES if c["stage"] == "map"], ids=lambda c: c["name"])
def test_map_reads_reproduces_reference(cm, fx, case):
    p = case["name"] + "/"
    queries, targets = MC.map_case_reads(case)
    MC.fixture_check(fx, p + "bases", np.frombuffer("".join(queries + (targets or [])).encode(), np.uint8), "inputs")
    filt = MC.OVERLAPPER_FILTERS[case["filter"]]
    o = cm.map_reads(queries, targets, case["k"], case["w"], case["F"], **filt)
    expected = O.map_reads(queries, targets, case["k"], case["w"], case["F"], **filt)
    assert len(o) == len(expected) == fx.meta[p + "n_overlaps"] and len(o) > 0, case["name"]
    for name in O.OVERLAP.names:
        np.testing.assert_array_equal(o[name], expected[name], err_msg="%s %s" % (case["name"], name))
    MC.fixture_check(fx, p + "overlaps", np.frombuffer(MC.overlap_bytes(o), np.uint8), case["name"])
