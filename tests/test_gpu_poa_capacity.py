"""The POA kernels at the capacity edges of a graph (windows: poa_capacity_cases.py, whose oracle answers
test_poa_capacity_cases.py shows to lie on both sides of every edge): windows that must end with
node_count_exceeded_maximum_graph_size (4), edge_count_exceeded_maximum_graph_size (5), exceeded_adaptive_banded_matrix_size (6)
or, from the output kernels, exceeded_maximum_sequence_size (2), and their neighbours that must succeed -- through the three
instantiations of the graph merge, in every band mode. Nothing here knows where an edge is: status, consensus, coverage and
MSA rows are the oracle's.

A failed window must also leave its neighbours alone: the same windows in shuffled batches, after reset(), and through the
persistent grid (more windows than resident blocks) give what they give alone."""
import ctypes as C
import random
import time

import pytest

import oracle_poa as O
import poa_capacity_cases as K

pytestmark = pytest.mark.gpu

CASES = K.all_cases()
_GPU = {}


def ids(cases):
    return [c["id"] for c in cases]


def make_batch(config, output, mem=2 << 30):
    """The batch of a case's config, by the constructor the config asks for; its BatchConfig must be the oracle's."""
    from genomeworks_amd import cudapoa
    cfg = K.oracle_cfg(config, 1 if output == "consensus" else 2)
    if config["max_nodes"] is None and config["max_consensus"] is None:
        b = cudapoa.CudaPoaBatch.from_batch_config(config["max_seq"], config["max_seqs"], config["band_width"], config["band_mode"], mem,
                                                   output_type=output, adaptive_storage_factor=config["storage_factor"],
                                                   graph_length_factor=config["graph_factor"])
    else:
        b = cudapoa.CudaPoaBatch(config["max_seqs"], config["max_seq"], mem, output_type=output, band_mode=config["band_mode"],
                                 alignment_band_width=config["band_width"], max_consensus_size=cfg.max_consensus_size,
                                 max_nodes_per_graph=cfg.max_nodes_per_graph, matrix_sequence_dimension=cfg.matrix_sequence_dimension,
                                 max_banded_pred_distance=cfg.max_banded_pred_distance)
    for field, _ in b.batch_size._fields_:
        assert getattr(b.batch_size, field) == getattr(cfg, field), (field, getattr(b.batch_size, field), getattr(cfg, field))
    return b


def run_windows(b, windows, output):
    """reset, add, generate -> per window (status, consensus, coverage) or (status, msa rows)."""
    b.reset()
    for reads in windows:
        st, seq_st = b.add_poa_group(reads)
        assert st == 0 and not any(seq_st), (st, seq_st)  # add_poa_group's own limits refuse nothing
    b.generate_poa()
    if output == "msa":
        msa, status = b.get_msa()
        assert len(status) == len(windows)
        return [(status[i], msa[i]) for i in range(len(windows))]
    cons, cov, status = b.get_consensus()
    assert len(status) == len(windows)
    return [(status[i], cons[i], cov[i]) for i in range(len(windows))]


def gpu_result(case):
    """This window's result; the batch of its (config, output) runs once per process with all its windows."""
    key = (K.config_key(case["config"]), case["output"])
    group = [c for c in CASES if (K.config_key(c["config"]), c["output"]) == key]
    if key not in _GPU:
        t = time.time()
        b = make_batch(case["config"], case["output"], (3 << 30) if case["output"] == "msa" else (2 << 30))
        _GPU[key] = run_windows(b, [c["reads"] for c in group], case["output"])
        print("batch %s %s: %d windows, %.2f s" % (group[0]["id"], case["output"], len(group), time.time() - t))
    return _GPU[key][ids(group).index(case["id"])]


def expected(ref, output):
    """What the host API returns for the oracle's answer: the output of a successful window; for a failed one its status, an
    empty consensus with an empty coverage, or no MSA rows."""
    if ref["status"] != 0:
        return (ref["status"], []) if output == "msa" else (ref["status"], "", [])
    if output == "msa":
        return (0, ref["msa"])
    return (0, ref["consensus"], [int(x) for x in ref["coverage"]])


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_status_and_output_equal_the_oracle(case):
    ref = K.oracle_result(case)
    got = gpu_result(case)
    want = expected(ref, case["output"])
    print(case["id"], "oracle status", ref["status"], "kernel status", got[0])
    assert got[0] == want[0], (got[0], want[0])
    assert got == want


# ---- isolation inside a batch ------------------------------------------------------------------------------------------------
# (band mode, max_sequence_size, output): the three merge instantiations, and the MSA instantiation of the LDS-table kernel
ISOLATION = (("static_band", 1024, "consensus"), ("adaptive_band", 1024, "msa"), ("static_band", 1025, "consensus"),
             ("adaptive_band", 1025, "consensus"), ("static_band_traceback", 1025, "consensus"), ("full_band", 1025, "consensus"))


@pytest.mark.parametrize("mode,max_seq,output", ISOLATION)
def test_failed_windows_leave_their_neighbours_alone(mode, max_seq, output):
    """The E_out and E_in sweeps of one config (12 windows, half of them fail) in one batch in two shuffled orders, the second
    after reset() on the same batch object: every succeeding window gives exactly what it gives in a batch of its own, every
    failing window keeps its status."""
    group = [c for c in CASES if c["class"] in ("E_out", "E_in") and c["output"] == output and c["config"]["band_mode"] == mode and
             c["config"]["max_seq"] == max_seq]
    assert len(group) == 12
    refs = [expected(K.oracle_result(c), output) for c in group]
    assert sorted(r[0] for r in refs) == [0] * 6 + [5] * 6
    solo = make_batch(group[0]["config"], output)
    alone = [run_windows(solo, [c["reads"]], output)[0] for c in group]
    assert alone == refs
    mixed = make_batch(group[0]["config"], output)
    for seed in (1, 2):
        order = list(range(len(group)))
        random.Random(seed).shuffle(order)
        got = run_windows(mixed, [group[i]["reads"] for i in order], output)
        for at, i in enumerate(order):
            assert got[at] == alone[i], (seed, at, group[i]["id"])


# ---- persistent grid ---------------------------------------------------------------------------------------------------------
def device_config(cfg):
    from genomeworks_amd import _native
    return _native.PoaConfig(cfg.max_sequence_size, cfg.max_consensus_size, cfg.max_nodes_per_graph, cfg.matrix_sequence_dimension,
                             cfg.alignment_band_width, cfg.max_sequences_per_poa, cfg.band_mode, cfg.max_banded_pred_distance,
                             cfg.gap_score, cfg.mismatch_score, cfg.match_score, cfg.output_mask, cfg.score32, 0, cfg.trace16, 0)


def test_failed_windows_in_the_persistent_grid():
    """One window more than there are resident blocks (gwhip_poa_resident_windows): the blocks fetch further windows from
    the work counter, and the failed E and N windows scattered among the 90-base windows must neither stop a block nor disturb
    what it takes next. Every window equals the oracle and what it gives in batches that fit the grid (one block per window);
    then again after reset() in another order on the same batch object."""
    from genomeworks_amd import _native
    cfg = K.oracle_cfg(K.PERSISTENT_CONFIG)
    L = _native.gwhip()
    L.gwhip_poa_resident_windows.argtypes = [C.POINTER(_native.PoaConfig)]
    L.gwhip_poa_resident_windows.restype = C.c_int32
    resident = L.gwhip_poa_resident_windows(C.byref(device_config(cfg)))
    assert resident >= 64, resident  # the LDS-table kernels: a persistent grid exists
    windows = K.persistent_windows(resident + 1)
    kinds = [kind for kind, _ in windows]
    assert kinds.count("E") >= 3 and kinds.count("N") >= 3
    refs, failing = [], {}
    with O.Workspace(cfg) as ws:
        for kind, reads in windows:
            if kind not in failing:
                ref = expected(ws.process(reads), "consensus")
                if kind != "ok":
                    failing[kind] = ref  # (the failing windows of a kind are copies)
            refs.append(ref if kind == "ok" else failing[kind])
    assert failing["E"][0] == 5 and failing["N"][0] == 4 and all(r[0] == 0 for r, k in zip(refs, kinds) if k == "ok")
    b = make_batch(K.PERSISTENT_CONFIG, "consensus", 1 << 30)
    assert b.max_poas >= len(windows), b.max_poas
    third = (len(windows) + 2) // 3
    assert third < resident
    in_parts = []
    for first in range(0, len(windows), third):
        in_parts += run_windows(b, [reads for _, reads in windows[first:first + third]], "consensus")
    assert in_parts == refs
    for seed in (0, 1):
        order = list(range(len(windows)))
        if seed:
            random.Random(seed).shuffle(order)
        got = run_windows(b, [windows[i][1] for i in order], "consensus")
        wrong = [(at, i, kinds[i]) for at, i in enumerate(order) if got[at] != in_parts[i]]
        assert not wrong, (seed, wrong[:10])
