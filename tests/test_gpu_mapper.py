"""cudamapper on the GPU against the plain-C oracle (tests/oracle_mapper.c) and the reference's known answers: index
arrays, anchors and overlaps array for array, on the reference's vectors, a seeded random sweep and the covid
fixture; plus the object life cycle."""
import hashlib

import numpy as np
import pytest

import mapper_cases as MC
import oracle_mapper as O

pytestmark = pytest.mark.gpu

INDEX_ARRAYS = [("representations", "representations"), ("read_ids", "read_ids"),
                ("positions_in_reads", "positions_in_reads"), ("directions_of_reads", "directions"),
                ("unique_representations", "unique_representations"),
                ("first_occurrence_of_representations", "first_occurrence_of_representations")]


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


def assert_index_equal(gpu, ref, where=""):
    for g, r in INDEX_ARRAYS:
        np.testing.assert_array_equal(getattr(gpu, g), ref[r], err_msg="%s %s" % (where, g))
    for f in ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read"):
        assert getattr(gpu, f) == ref[f], (where, f, getattr(gpu, f), ref[f])


def check_pipeline(cm, queries, targets, k, w, hash_representations, F, params, where):
    qi = cm.Index(queries, k, w, hash_representations, F)
    qo = O.index(queries, k, w, hash_representations, F)
    assert_index_equal(qi, qo, where + " query")
    if targets is None:
        ti, to = qi, qo
    else:
        ti = cm.Index(targets, k, w, hash_representations, F, first_read_id=len(queries))
        to = O.index(targets, k, w, hash_representations, F, first_read_id=len(queries))
        assert_index_equal(ti, to, where + " target")
    m = cm.Matcher(qi, ti)
    a_ref = O.anchors(qo, to)
    a = m.anchors()
    assert a.dtype == cm.ANCHOR
    np.testing.assert_array_equal(a, a_ref, err_msg=where + " anchors")
    o = cm.find_overlaps(m, targets is None, **params)
    o_ref = O.overlaps(a_ref, targets is None, **params)
    assert MC.overlap_bytes(o) == MC.overlap_bytes(o_ref), where + " overlaps"
    return qi, a, o


# ---- the reference's known answers ---------------------------------------------------------------------------------

def test_minimizer_vectors(cm):
    for case in MC.load_vectors()["minimizers"]:
        idx = cm.Index(case["reads"], case["k"], case["w"], case["hash"], 1.0, case.get("first_read_id", 0))
        order = np.lexsort((idx.positions_in_reads, idx.read_ids))  # sketch order: read, then position
        assert idx.representations[order].tolist() == case["representations"], case["source"]
        assert idx.read_ids[order].tolist() == case["read_ids"], case["source"]
        assert idx.positions_in_reads[order].tolist() == case["positions_in_reads"], case["source"]
        assert idx.directions_of_reads[order].tolist() == case["directions"], case["source"]


def test_index_vectors(cm):
    for case in MC.load_vectors()["indices"]:
        idx = cm.Index(case["reads"], case["k"], case["w"], False, case["filtering_parameter"], case["first_read_id"])
        for name in ("representations", "read_ids", "positions_in_reads", "directions_of_reads",
                     "unique_representations", "first_occurrence_of_representations"):
            assert getattr(idx, name).tolist() == case[name], (case["source"], name)
        assert idx.number_of_reads == case["number_of_reads"], case["source"]
        assert idx.number_of_basepairs_in_longest_read == case["number_of_basepairs_in_longest_read"], case["source"]
        if case["number_of_reads"]:
            assert (idx.smallest_read_id, idx.largest_read_id) == (case["smallest_read_id"], case["largest_read_id"])


def test_matcher_vectors(cm):
    for case in MC.load_vectors()["matcher"]:
        side = {}
        for s in ("query", "target"):
            side[s] = cm.Index.from_arrays(case[s + "_read_ids"], case[s + "_positions_in_reads"],
                                           case[s + "_unique_representations"], case[s + "_first_occurrence"],
                                           case[s + "_first_read_id"], case[s + "_number_of_reads"], case[s + "_longest"])
        a = cm.find_anchors(side["query"], side["target"])
        assert [tuple(int(v) for v in x) for x in a] == [tuple(x) for x in case["expected_anchors"]], case["source"]
    for case in MC.load_vectors()["matcher_files"]:
        q = cm.Index(case["reads"], case["query_k"], case["w"])
        t = cm.Index(case["reads"], case["target_k"], case["w"])
        assert len(cm.find_anchors(q, t)) == case["expected_count"], case["source"]


def test_negative_thresholds_are_an_error(cm):
    a = np.array([(1, 2, 100, 1000), (1, 2, 200, 1100), (1, 2, 300, 1200)], cm.ANCHOR)
    for bad in (dict(min_residues=-1), dict(min_overlap_len=-1), dict(min_bases_per_residue=-5)):
        with pytest.raises(cm.MapperError):
            cm.find_overlaps(a, False, **dict(dict(min_residues=0, min_overlap_len=0, min_bases_per_residue=1000), **bad))


def test_c_api_map_matches_oracle(cm):
    """gw_mapper_map, the one-call C entry point, all-vs-all and query-vs-target."""
    import ctypes as C
    from genomeworks_amd import _native
    L = _native.mapper()
    reads = MC.synthetic_reads(41, 20000, 6, 2000, 0.03)
    half = len(reads) // 2
    for queries, targets in ((reads, None), (reads[:half], reads[half:])):
        qb, qo = cm.pack_reads(queries)
        tb, to = cm.pack_reads(targets) if targets is not None else (None, None)
        vp = C.c_void_p
        cap = 1 << 16
        out = np.zeros(cap, cm.OVERLAP)
        n = L.gw_mapper_map(qb.ctypes.data_as(vp), qo.ctypes.data_as(vp), len(queries),
                            tb.ctypes.data_as(vp) if tb is not None else None,
                            to.ctypes.data_as(vp) if to is not None else None, len(targets or []),
                            15, 10, 1.0, 3, 250, 1000, 0.8, out.ctypes.data_as(vp), cap, None)
        assert 0 < n <= cap, n
        ref = O.map_reads(queries, targets, 15, 10, 1.0)
        assert MC.overlap_bytes(out[:n]) == MC.overlap_bytes(ref)


def test_overlapper_vectors(cm):
    for case in MC.load_vectors()["overlapper"]:
        anchors = np.array([tuple(a) for a in case["anchors"]], cm.ANCHOR)
        o = cm.find_overlaps(anchors, case["all_to_all"], case["min_residues"], case["min_overlap_len"],
                             case["min_bases_per_residue"], case["min_overlap_fraction"])
        assert len(o) == len(case["expected"]), case["source"]
        for got, exp in zip(o, case["expected"]):
            for f, v in exp.items():
                want = ord(v) if f == "relative_strand" else v
                assert int(got[f]) == want, (case["source"], f)


# ---- seeded random sweep -------------------------------------------------------------------------------------------

SWEEP = [  # (seed, genome, coverage, mean length, error, k, w, hash, F, min_overlap_len)
    (1, 20000, 8, 2000, 0.03, 15, 10, True, 1.0, 250),
    (2, 20000, 8, 2000, 0.03, 15, 5, True, 2e-4, 250),
    (3, 5000, 6, 300, 0.02, 12, 1, True, 1.0, 100),         # w = 1
    (4, 8000, 6, 800, 0.02, 32, 4, True, 1.0, 150),         # k at its maximum, hashed
    (5, 8000, 6, 800, 0.02, 32, 4, False, 1.0, 150),        # k at its maximum, plain representations
    (6, 3000, 4, 400, 0.05, 16, 8, False, 1e-3, 100),       # k = 16: the sign-extended top code
    (7, 4000, 10, 60, 0.01, 15, 30, True, 1.0, 10),         # many reads shorter than k + w - 1
    (8, 10000, 3, 1500, 0.10, 9, 3, False, 0.01, 250),
]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "seed%d_k%d_w%d" % (c[0], c[5], c[6]))
def test_random_sweep_all_vs_all(cm, case):
    seed, g, cov, length, err, k, w, h, F, mol = case
    reads = MC.synthetic_reads(seed, g, cov, length, err)
    params = dict(MC.OVERLAP_PARAMS, min_overlap_len=mol)
    check_pipeline(cm, reads, None, k, w, h, F, params, "sweep %s" % (case,))


def test_random_query_vs_target(cm):
    reads = MC.synthetic_reads(11, 30000, 6, 3000, 0.03)
    half = len(reads) // 2
    check_pipeline(cm, reads[:half], reads[half:], 15, 10, True, 1.0, MC.OVERLAP_PARAMS, "q-vs-t")


def test_zero_sized_stages(cm):
    # no read long enough: empty index, no anchors, no overlaps
    empty = cm.Index(["ACGT", "AC"], 15, 10)
    assert empty.number_of_reads == 0 and len(empty.representations) == 0
    assert len(empty.first_occurrence_of_representations) == 0
    assert len(cm.find_anchors(empty, empty)) == 0
    # everything filtered away (threshold 0)
    reads = MC.synthetic_reads(21, 2000, 2, 300, 0.0)
    gone = cm.Index(reads, 15, 5, True, 1e-9)
    ref = O.index(reads, 15, 5, True, 1e-9)
    assert_index_equal(gone, ref, "all filtered")
    assert len(gone.representations) == 0 and gone.first_occurrence_of_representations.tolist() == [0]
    full = cm.Index(reads, 15, 5)
    assert len(cm.find_anchors(gone, full)) == 0 and len(cm.find_anchors(full, gone)) == 0
    # disjoint read sets: no shared minimizer, zero anchors
    a = cm.Index(["A" * 200], 15, 5, False)
    c = cm.Index(["C" * 200], 15, 5, False)
    m = cm.Matcher(a, c)
    assert m.n_anchors == 0 and len(cm.find_overlaps(m)) == 0
    assert len(cm.find_overlaps(np.zeros(0, cm.ANCHOR))) == 0


# ---- covid fixture -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def covid():
    return MC.covid_reads()[1]


@pytest.mark.parametrize("cfg", MC.COVID_CONFIGS, ids=lambda c: "w%d_F%g" % (c["w"], c["F"]))
def test_covid_all_vs_all(cm, covid, cfg):
    idx, a, o = check_pipeline(cm, covid, None, cfg["k"], cfg["w"], True, cfg["F"], MC.OVERLAP_PARAMS,
                               "covid %s" % cfg)
    golden = np.load(MC.COVID_NPZ)
    key = "w%d_F%g" % (cfg["w"], cfg["F"])
    assert int(golden[key + "_n_overlaps"]) == len(o)
    assert str(golden[key + "_overlaps_sha256"]) == hashlib.sha256(MC.overlap_bytes(o)).hexdigest()
    if key + "_overlaps" in golden:
        assert MC.overlap_bytes(golden[key + "_overlaps"]) == MC.overlap_bytes(o)
    assert int(golden[key + "_n_anchors"]) == len(a)
    assert int(golden[key + "_n_elements"]) == len(idx.representations)


def test_covid_map_reads_matches_oracle(cm, covid):
    o = cm.map_reads(covid, k=15, w=5, filtering_parameter=1.0)
    assert MC.overlap_bytes(o) == MC.overlap_bytes(O.map_reads(covid, k=15, w=5, filtering_parameter=1.0))


# ---- life cycle ----------------------------------------------------------------------------------------------------

def test_create_destroy_many_times(cm):
    reads = MC.synthetic_reads(31, 10000, 5, 1000, 0.02)
    ref = None
    for i in range(40):
        idx = cm.Index(reads, 15, 10)
        m = cm.Matcher(idx, idx)
        o = cm.find_overlaps(m, True, **MC.OVERLAP_PARAMS)
        if ref is None:
            ref = MC.overlap_bytes(o)
        assert MC.overlap_bytes(o) == ref, i
        m.close()
        idx.close()
