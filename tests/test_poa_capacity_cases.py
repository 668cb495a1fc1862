"""The generators of poa_capacity_cases.py reach what they were built for (CPU, oracle only): every class holds windows that
succeed and windows that end with the class's failure status, the precedence class holds both answers, the edge-slot windows
fail with 5 and not with 4 and really reach the degree they aim at, and add_poa_group's own limits refuse no window.
test_gpu_poa_capacity.py then compares the kernels with the same oracle answers."""
import collections

import poa_capacity_cases as K

CASES = K.all_cases()


def by_class(cls):
    return [c for c in CASES if c["class"] == cls]


def groups(cls):
    """The cases of a class by (merge instantiation, band mode, output): each of them has to hold both sides."""
    out = collections.defaultdict(list)
    for c in by_class(cls):
        out[c["merge"], c["config"]["band_mode"], c["output"]].append(c)
    return out


def test_every_class_and_every_merge_instantiation_is_there():
    assert {c["class"] for c in CASES} == set(K.FAILURE)
    assert {c["side"] for c in CASES} == {"below", "at", "above"}
    for cls in ("E_out", "E_in", "N", "P"):
        assert {c["merge"] for c in by_class(cls)} == {"lds", "matrix", "serial"}, cls
        assert {c["config"]["band_mode"] for c in by_class(cls)} == set(K.BAND_MODES), cls
    for cls in ("E_out", "E_in"):
        assert {c["output"] for c in by_class(cls)} == {"consensus", "msa"}


def test_no_window_is_refused_by_add_poa_group():
    """add_seq_to_poa refuses a read longer than max_sequence_size and a read beyond max_sequences_per_poa (its other refusals
    are about weights and the batch's memory); the explicit BatchConfig wants max_nodes_per_graph and max_consensus_size >=
    max_sequence_size >= band width."""
    for c in CASES:
        cfg = K.oracle_cfg(c["config"])
        assert 2 <= len(c["reads"]) <= cfg.max_sequences_per_poa, c["id"]
        assert all(1 <= len(r) <= cfg.max_sequence_size for r in c["reads"]), c["id"]
        if c["config"]["max_nodes"] is not None:
            assert cfg.max_nodes_per_graph >= cfg.max_sequence_size >= cfg.alignment_band_width, c["id"]
            assert cfg.max_consensus_size >= cfg.max_sequence_size, c["id"]


def test_each_class_reaches_success_and_its_failure_status():
    for cls, failure in K.FAILURE.items():
        for key, cases in groups(cls).items():
            statuses = [K.oracle_result(c)["status"] for c in cases]
            print(cls, key, statuses)
            assert 0 in statuses, (cls, key, statuses)
            assert set(statuses) <= {0} | set(failure), (cls, key, statuses)
            if cls != "P":
                assert failure[0] in statuses, (cls, key, statuses)


def test_precedence_class_holds_both_answers():
    for key, cases in groups("P").items():
        statuses = {c["id"]: K.oracle_result(c)["status"] for c in cases}
        assert {0, 4, 5} <= set(statuses.values()), (key, statuses)
        # the read that overflows both at one read position: the node count is checked first
        both = [s for cid, s in statuses.items() if "both_at_one_position" in cid]
        assert both == [4], (key, statuses)


def test_edge_windows_fail_with_the_edge_status_and_reach_their_degree():
    """Status 5 and never 4; the windows below the edge really hold a node with K + 1 edges on the side they were built for (so
    the edge was met by the degree, not by an accident of the alignment), read from the oracle's MSA rows: a deletion of d bases
    shows as d gap columns in one row."""
    for cls in ("E_out", "E_in"):
        for c in by_class(cls):
            ref = K.oracle_result(c)
            assert ref["status"] in (0, 5), (c["id"], ref["status"])
            assert ref["node_count"] == len(c["reads"][0]), c["id"]  # deletions only: no read adds a node
            if ref["status"] == 0 and c["output"] == "msa":
                gaps = sorted(row.count("-") for row in ref["msa"])
                assert gaps == list(range(len(c["reads"]))), c["id"]  # every deletion length 0 .. K once, nothing else
                starts = {row.index("-") for row in ref["msa"][1:]} if cls == "E_out" else {row.rindex("-") for row in ref["msa"][1:]}
                assert len(starts) == 1, (c["id"], starts)  # all gaps begin behind (end in front of) one node: K + 1 edges there
        for key, cases in groups(cls).items():
            good = [len(c["reads"]) - 1 for c in cases if K.oracle_result(c)["status"] == 0]
            bad = [len(c["reads"]) - 1 for c in cases if K.oracle_result(c)["status"] == 5]
            assert max(good) == K.MAX_EDGES - 2 and min(bad) == K.MAX_EDGES - 1, (cls, key, good, bad)


def test_persistent_windows_hold_the_failures_they_scatter():
    windows = K.persistent_windows(300)
    kinds = collections.Counter(kind for kind, _ in windows)
    assert kinds["E"] >= 3 and kinds["N"] >= 2 and kinds["ok"] >= 290
    seen = {}
    for kind, reads in windows:
        if kind not in seen or kind == "ok":
            st = K.oracle_window(K.PERSISTENT_CONFIG, reads, "consensus")["status"]
            assert st == {"E": 5, "N": 4, "ok": 0}[kind], (kind, st)
            seen[kind] = st
        assert all(len(r) <= K.PERSISTENT_CONFIG["max_seq"] for r in reads) and len(reads) <= K.PERSISTENT_CONFIG["max_seqs"]
