"""cudamapper without a GPU: the plain-C oracle reproduces the reference's known answers (cudamapper_vectors.json) and
the committed covid goldens; libcudamapper.so is built apart from the stamped POA / aligner kernel set."""
import hashlib
import os

import numpy as np

import mapper_cases as MC
import oracle_mapper as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_minimizer_vectors():
    for case in MC.load_vectors()["minimizers"]:
        s = O.sketch(case["reads"], case["k"], case["w"], case["hash"], case["first_read_id"])
        for name in ("representations", "read_ids", "positions_in_reads", "directions"):
            assert s[name].tolist() == case[name], (case["source"], name)


def test_oracle_index_vectors():
    for case in MC.load_vectors()["indices"]:
        # the reads come from the committed FASTA fixture the reference test names
        names, seqs = MC.read_fasta(os.path.join(MC.GOLDEN, "cudamapper_data", case["fasta"]))
        assert seqs[case["first_read_id"]:case["past_the_last_read_id"]] == case["reads"], case["source"]
        idx = O.index(case["reads"], case["k"], case["w"], False, case["filtering_parameter"], case["first_read_id"])
        idx["directions_of_reads"] = idx["directions"]
        for name in ("representations", "read_ids", "positions_in_reads", "directions_of_reads",
                     "unique_representations", "first_occurrence_of_representations", "number_of_reads",
                     "number_of_basepairs_in_longest_read"):
            got = idx[name].tolist() if hasattr(idx[name], "tolist") else idx[name]
            assert got == case[name], (case["source"], name)
        if case["number_of_reads"]:
            assert (idx["smallest_read_id"], idx["largest_read_id"]) == (case["smallest_read_id"],
                                                                          case["largest_read_id"]), case["source"]


def oracle_index_from_case(case, side):
    return dict(unique_representations=np.array(case[side + "_unique_representations"], np.uint64),
                first_occurrence_of_representations=np.array(case[side + "_first_occurrence"], np.uint32),
                read_ids=np.array(case[side + "_read_ids"], np.uint32),
                positions_in_reads=np.array(case[side + "_positions_in_reads"], np.uint32))


def test_oracle_matcher_vectors():
    for case in MC.load_vectors()["matcher"]:
        a = O.anchors(oracle_index_from_case(case, "query"), oracle_index_from_case(case, "target"))
        assert [tuple(int(v) for v in x) for x in a] == [tuple(x) for x in case["expected_anchors"]], case["source"]
    for case in MC.load_vectors()["matcher_files"]:
        q = O.index(case["reads"], case["query_k"], case["w"], True)
        t = O.index(case["reads"], case["target_k"], case["w"], True)
        assert len(O.anchors(q, t)) == case["expected_count"], case["source"]


def test_oracle_overlapper_vectors():
    for case in MC.load_vectors()["overlapper"]:
        anchors = np.array([tuple(a) for a in case["anchors"]], O.ANCHOR)
        o = O.overlaps(anchors, case["all_to_all"], case["min_residues"], case["min_overlap_len"],
                       case["min_bases_per_residue"], case["min_overlap_fraction"])
        assert len(o) == len(case["expected"]), case["source"]
        for got, exp in zip(o, case["expected"]):
            for f, v in exp.items():
                assert int(got[f]) == (ord(v) if f == "relative_strand" else v), (case["source"], f)


def test_oracle_chain_rules():
    # (prev, cur) order: a query step back is a huge unsigned difference and breaks the chain; the target step is
    # taken in absolute value
    a = np.array([(0, 1, 100, 500), (0, 1, 120, 480), (0, 1, 140, 460), (0, 1, 160, 440)], O.ANCHOR)
    o = O.overlaps(a, False, 0, 0, 1000, 0.0)
    assert len(o) == 1 and o[0]["relative_strand"] == ord("-") and o[0]["num_residues"] == 4
    # two chains of 3 whose first anchors satisfy ||dq| - |dt|| < 300 fuse (residues add up); a 2-anchor chain between
    # them is dropped before fusion
    a = np.array([(0, 1, 0, 0), (0, 1, 100, 100), (0, 1, 200, 200),
                  (0, 1, 1000, 5000), (0, 1, 1100, 5100),
                  (0, 1, 2000, 2000), (0, 1, 2100, 2100), (0, 1, 2200, 2200)], O.ANCHOR)
    o = O.overlaps(a, False, 0, 0, 1000, 0.0)
    assert len(o) == 1 and o[0]["num_residues"] == 6 and o[0]["query_end_position_in_read"] == 2200
    # self-mappings go only when all_to_all is set
    a = np.array([(3, 3, 0, 0), (3, 3, 100, 100), (3, 3, 200, 200)], O.ANCHOR)
    assert len(O.overlaps(a, True, 0, 0, 1000, 0.0)) == 0 and len(O.overlaps(a, False, 0, 0, 1000, 0.0)) == 1


def test_oracle_reproduces_covid_goldens():
    reads = MC.covid_reads()[1]
    assert len(reads) == 3000 and sum(map(len, reads)) == 1153275
    golden = np.load(MC.COVID_NPZ)
    for cfg in MC.COVID_CONFIGS[:2]:  # the filtered configs: the unfiltered ones run on the GPU test only
        key = "w%d_F%g" % (cfg["w"], cfg["F"])
        idx = O.index(reads, cfg["k"], cfg["w"], True, cfg["F"])
        a = O.anchors(idx, idx)
        o = O.overlaps(a, True, **MC.OVERLAP_PARAMS)
        assert int(golden[key + "_n_elements"]) == len(idx["representations"])
        assert int(golden[key + "_n_anchors"]) == len(a)
        assert str(golden[key + "_overlaps_sha256"]) == hashlib.sha256(MC.overlap_bytes(o)).hexdigest()


def test_mapper_library_is_built_apart_from_the_kernel_digest():
    import json
    from genomeworks_amd import build as B
    lib = os.path.join(ROOT, "genomeworks_amd", "lib", "libcudamapper.so")
    assert os.path.exists(lib), "build() did not produce libcudamapper.so"
    assert all(not s.startswith("mapper/") for s in B.KERNEL_SRCS + B.HOST_SRCS)
    # the stamped POA / aligner kernel set is the one the last PMC profile was taken on
    with open(os.path.join(ROOT, "profiles", "r06_pmc_profile.json")) as f:
        stamp = json.load(f)["kernel_source_sha256"]
    assert B.kernel_source_digest() == stamp
    with open(lib, "rb") as f:
        data = f.read()
    for sym in (b"gw_mapper_index_create", b"gw_mapper_matcher_create", b"gw_mapper_get_overlaps", b"gw_mapper_map",
                b"gwm_index_build"):
        assert sym in data, sym
