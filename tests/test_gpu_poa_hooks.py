"""GPU unit tests of the individual POA device functions through the gwhip_poa_test_* hooks, fed with the
reference's own inline known-answer vectors (tests/golden/cudapoa_vectors.json), and of the merge the window kernels run
(add_alignment_parallel) through gwhip_poa_test_add_alignment_parallel (libgwhip_poa_hooks.so): the same vectors, byte-equal to
the serial routine, and hand-built graphs at the edge slots, the node budget and the precedence of the two."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_poa as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "cudapoa_vectors.json")) as f:
    V = json.load(f)
E = 50


class HookGraph(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("graph", C.c_void_p), ("node_id_to_pos", C.c_void_p), ("graph_count", C.c_int32),
                ("incoming_edge_count", C.c_void_p), ("incoming_edges", C.c_void_p), ("outgoing_edge_count", C.c_void_p),
                ("outgoing_edges", C.c_void_p)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lib():
    from genomeworks_amd import _native
    L = _native.gwhip()
    L.gwhip_poa_test_nw_scratch_bytes.restype = C.c_size_t
    L.gwhip_poa_test_nw_scratch_bytes.argtypes = [C.POINTER(_native.PoaConfig)]
    L.gwhip_poa_test_nw.argtypes = [C.POINTER(_native.PoaConfig), C.POINTER(HookGraph), C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.gwhip_poa_test_topsort.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.gwhip_poa_test_add_alignment.argtypes = [C.c_void_p] * 9 + [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_void_p]
    L.gwhip_poa_test_consensus.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 14 + [C.c_int32, C.c_void_p]
    return L


def device_cfg(ocfg):
    from genomeworks_amd import _native
    return _native.PoaConfig(ocfg.max_sequence_size, ocfg.max_consensus_size, ocfg.max_nodes_per_graph,
                             ocfg.matrix_sequence_dimension, ocfg.alignment_band_width, ocfg.max_sequences_per_poa,
                             ocfg.band_mode, ocfg.max_banded_pred_distance, ocfg.gap_score, ocfg.mismatch_score,
                             ocfg.match_score, 1, 0, 1, ocfg.trace16, 0)


def run_nw_gpu(ocfg, g, read):
    import torch
    L = lib()
    cfg = device_cfg(ocfg)
    mx = ocfg.max_nodes_per_graph
    t = {k: dev(g[k]) for k in ("nodes", "graph", "pos", "incoming_count", "incoming", "outgoing_count", "outgoing")}
    tg = HookGraph(t["nodes"].data_ptr(), t["graph"].data_ptr(), t["pos"].data_ptr(), g["count"],
                   t["incoming_count"].data_ptr(), t["incoming"].data_ptr(), t["outgoing_count"].data_ptr(),
                   t["outgoing"].data_ptr())
    rb = np.zeros(ocfg.max_sequence_size + 4096, np.uint8)
    r = np.frombuffer(read.encode(), np.uint8)
    rb[:len(r)] = r
    d_read = dev(rb)
    scratch = torch.zeros(L.gwhip_poa_test_nw_scratch_bytes(C.byref(cfg)) + 256, dtype=torch.uint8, device="cuda")
    ag = torch.zeros(2 * mx + 16, dtype=torch.int32, device="cuda")
    ar = torch.zeros(2 * mx + 16, dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = L.gwhip_poa_test_nw(C.byref(cfg), C.byref(tg), d_read.data_ptr(), len(r), scratch.data_ptr(), ag.data_ptr(),
                             ar.data_ptr(), n.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    k = int(n.item())
    return k, ag[:max(k, 0)].cpu().numpy(), ar[:max(k, 0)].cpu().numpy()


def csv(a):
    return ",".join(str(int(x)) for x in a)


@pytest.mark.parametrize("mode", ["full", "static", "adaptive", "static_tb", "adaptive_tb"])
@pytest.mark.parametrize("case", V["nw"], ids=[c["name"] for c in V["nw"]])
def test_nw_known_answers(case, mode):
    # Test_CudapoaNW.cu:100-187 (full band) and the same graphs through every banded variant
    bm = {"full": 0, "static": 1, "adaptive": 2, "static_tb": 3, "adaptive_tb": 4}[mode]
    ocfg = O.make_cfg() if mode == "full" else O.make_cfg(1024, 2, 128, bm)
    g = O.graph_buffers(case["nodes"], case["outgoing"], ocfg.max_nodes_per_graph, case["sorted"])
    n, ag, ar = run_nw_gpu(ocfg, g, case["read"])
    assert (csv(ag), csv(ar)) == (case["graph_ans"], case["read_ans"])


@pytest.mark.parametrize("mode", ["static", "adaptive", "static_tb", "adaptive_tb"])
def test_nw_banded_equals_full_493x530(mode):
    # Test_CudapoaNW.cu:446-508
    nb = V["nw_banded"]
    nodes, read = nb["nodes"], nb["read"]
    outgoing = [[i + 1] for i in range(len(nodes) - 1)] + [[]]
    bm = {"static": 1, "adaptive": 2, "static_tb": 3, "adaptive_tb": 4}[mode]
    cf = O.make_cfg()
    g = O.graph_buffers(nodes, outgoing, cf.max_nodes_per_graph, list(range(len(nodes))))
    nf, agf, arf = run_nw_gpu(cf, g, read)
    cb = O.make_cfg(1024, 2, 128, bm)
    nbn, agb, arb = run_nw_gpu(cb, g, read)
    assert nf == nbn == 550
    assert csv(agf) == csv(agb) and csv(arf) == csv(arb)
    no, ago, aro = O.run_nw(cb, g, read, mode)
    assert csv(ago) == csv(agb) and csv(aro) == csv(arb)


@pytest.mark.parametrize("case", V["topsort"], ids=[c["answer"] for c in V["topsort"]])
def test_topsort_known_answers(case):
    # Test_CudapoaTopSort.cu:48-58
    import torch
    n = len(case["outgoing"])
    g = O.graph_buffers(None, case["outgoing"], 64)
    sp = torch.zeros(64, dtype=torch.int32, device="cuda")
    pos = torch.zeros(64, dtype=torch.int32, device="cuda")
    loc = torch.zeros(64, dtype=torch.int16, device="cuda")
    ic, oe, oc = dev(g["incoming_count"]), dev(g["outgoing"]), dev(g["outgoing_count"])
    assert lib().gwhip_poa_test_topsort(sp.data_ptr(), pos.data_ptr(), n, ic.data_ptr(), oe.data_ptr(), oc.data_ptr(),
                                        loc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert "-".join(str(int(x)) for x in sp[:n].cpu()) == case["answer"]


@pytest.mark.parametrize("idx", range(len(V["add_alignment"])))
def test_add_alignment_known_answers(idx):
    # Test_CudapoaAddAlignment.cu:127-229
    import torch
    case = V["add_alignment"][idx]
    mx = 3072
    g = O.graph_buffers(case["nodes"], case["outgoing"], mx)
    t = {k: dev(g[k]) for k in ("nodes", "incoming_count", "incoming", "outgoing_count", "outgoing")}
    na = torch.zeros(mx * E, dtype=torch.int32, device="cuda")
    nac = torch.zeros(mx, dtype=torch.int16, device="cuda")
    w = torch.zeros(mx * E, dtype=torch.int16, device="cuda")
    cov = np.zeros(mx, np.uint16)
    cov[:len(case["coverage"])] = case["coverage"]
    d_cov = dev(cov)
    rd = dev(np.frombuffer(case["read"].encode(), np.uint8).copy())
    bw = dev(np.array(case["weights"], np.int8))
    ag = dev(np.array(case["alignment_graph"], np.int32))
    ar = dev(np.array(case["alignment_read"], np.int32))
    nc = dev(np.array([len(case["nodes"])], np.int32))
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib().gwhip_poa_test_add_alignment(t["nodes"].data_ptr(), nc.data_ptr(), na.data_ptr(), nac.data_ptr(),
                                            t["incoming"].data_ptr(), t["incoming_count"].data_ptr(),
                                            t["outgoing"].data_ptr(), t["outgoing_count"].data_ptr(), w.data_ptr(),
                                            len(case["alignment_graph"]), ag.data_ptr(), rd.data_ptr(), ar.data_ptr(),
                                            d_cov.data_ptr(), bw.data_ptr(), mx, st.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    n = int(nc.item())
    oc = t["outgoing_count"].cpu().numpy()
    oe = t["outgoing"].cpu().numpy()
    assert [[int(oe[i * E + j]) for j in range(oc[i])] for i in range(n)] == case["answer"]


@pytest.mark.parametrize("idx", range(len(V["consensus"])))
def test_consensus_known_answers(idx):
    # Test_CudapoaGenerateConsensus.cu:95-160 with the harness's weight placement [to*50 + from] (:62-73)
    import torch
    case = V["consensus"][idx]
    mx = 3072
    g = O.graph_buffers(case["nodes"], case["outgoing"], mx, case["sorted"])
    na = np.zeros(mx * E, np.int32)
    nac = np.zeros(mx, np.uint16)
    for i, al in enumerate(case["node_alignments"]):
        for j, a in enumerate(al):
            na[i * E + j] = a
            nac[i] += 1
    w = np.zeros(mx * E, np.uint16)
    for i, outs in enumerate(case["outgoing"]):
        for j, to in enumerate(outs):
            w[to * E + i] = case["outgoing_w"][i][j]
    cov = np.zeros(mx, np.uint16)
    cov[:len(case["coverage"])] = case["coverage"]
    t = {k: dev(g[k]) for k in ("nodes", "graph", "pos", "incoming_count", "incoming", "outgoing_count", "outgoing")}
    d_na, d_nac, d_w, d_cov = dev(na), dev(nac), dev(w), dev(cov)
    preds = torch.zeros(mx, dtype=torch.int32, device="cuda")
    scores = torch.zeros(mx + 2, dtype=torch.int32, device="cuda")
    cons = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    cvg = torch.zeros(2048, dtype=torch.int16, device="cuda")
    rc = lib().gwhip_poa_test_consensus(t["nodes"].data_ptr(), len(case["nodes"]), t["graph"].data_ptr(), t["pos"].data_ptr(),
                                        t["incoming"].data_ptr(), t["incoming_count"].data_ptr(), t["outgoing"].data_ptr(),
                                        t["outgoing_count"].data_ptr(), d_w.data_ptr(), preds.data_ptr(), scores.data_ptr(),
                                        cons.data_ptr(), cvg.data_ptr(), d_cov.data_ptr(), d_na.data_ptr(), d_nac.data_ptr(),
                                        2048, None)
    assert rc == 0
    torch.cuda.synchronize()
    c = cons.cpu().numpy()
    n = int(np.argmax(c == 0))
    assert bytes(c[:n]).decode() == case["answer"]


def test_scores_that_leave_int16_end_as_an_error_not_as_a_result():
    """The kernels equal the reference only while no int16 store wraps (with a wrap the reference's result depends on its
    relaxation order). The precondition is enforced: the 493-node case through the static band with a match score that drives
    the scores past 32767 returns the kernel's "score wrapped" code (StatusType::generic_error at the batch level), while the
    same call with the default scores still gives the known answer."""
    nb = V["nw_banded"]
    nodes, read = nb["nodes"], nb["read"]
    outgoing = [[i + 1] for i in range(len(nodes) - 1)] + [[]]
    cb = O.make_cfg(1024, 2, 128, 1)
    g = O.graph_buffers(nodes, outgoing, cb.max_nodes_per_graph, list(range(len(nodes))))
    n_ok, _, _ = run_nw_gpu(cb, g, read)
    assert n_ok == 550
    hot = O.make_cfg(1024, 2, 128, 1, match=120)  # ~490 matches x 120 > 32767; the hook keeps the int16 instantiation
    hot.score32 = 0
    n_bad, _, _ = run_nw_gpu(hot, g, read)
    assert n_bad == -5  # kNwScoreWrapped (poa_layout.h)


# ---- the merge the window kernels run (add_alignment_parallel) next to the serial addAlignmentToGraph ------------------------
GRAPH_ARRAYS = ("nodes", "node_alignments", "node_alignment_count", "incoming", "incoming_count", "outgoing", "outgoing_count",
                "weights", "coverage")


def merge_state(nodes, outgoing, coverage, mx=3072, aligned=None):
    """Host arrays of a graph in the hooks' layout; aligned: {node: [nodes aligned to it]}."""
    g = O.graph_buffers(nodes, outgoing, mx)
    s = dict(nodes=g["nodes"], node_alignments=np.zeros(mx * E, np.int32), node_alignment_count=np.zeros(mx, np.uint16),
             incoming=g["incoming"], incoming_count=g["incoming_count"], outgoing=g["outgoing"], outgoing_count=g["outgoing_count"],
             weights=np.zeros(mx * E, np.uint16), coverage=np.zeros(mx, np.uint16), count=len(nodes))
    s["coverage"][:len(coverage)] = coverage
    for n, others in (aligned or {}).items():
        s["node_alignment_count"][n] = len(others)
        s["node_alignments"][n * E:n * E + len(others)] = others
    return s


def run_merge(state, read, weights, alignment_graph, alignment_read, max_nodes, which):
    """which: "serial" (gwhip_poa_test_add_alignment), "parallel32" / "parallel16" (gwhip_poa_test_add_alignment_parallel with
    32-bit / 16-bit scratch). -> (return code: the serial hook's status, the parallel merge's value as it is; node count;
    {array: host copy})."""
    import torch
    from genomeworks_amd import _native
    t = {k: dev(state[k]) for k in GRAPH_ARRAYS}
    rd = dev(np.frombuffer(read.encode(), np.uint8).copy())
    bw = dev(np.array(weights, np.int8))
    ag = dev(np.array(alignment_graph, np.int32))
    ar = dev(np.array(alignment_read, np.int32))
    nc = dev(np.array([state["count"]], np.int32))
    rc = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    graph_args = [t[k].data_ptr() for k in ("nodes",)] + [nc.data_ptr()] + [t[k].data_ptr() for k in (
        "node_alignments", "node_alignment_count", "incoming", "incoming_count", "outgoing", "outgoing_count", "weights")]
    tail = [len(alignment_graph), ag.data_ptr(), rd.data_ptr(), ar.data_ptr(), t["coverage"].data_ptr(), bw.data_ptr()]
    if which == "serial":
        err = lib().gwhip_poa_test_add_alignment(*graph_args, *tail, max_nodes, rc.data_ptr(), None)
    else:
        H = _native.poa_hooks()
        s16 = 1 if which == "parallel16" else 0
        scratch = torch.zeros(H.gwhip_poa_test_add_alignment_parallel_scratch_bytes(len(read), max_nodes, s16) + 16, dtype=torch.uint8, device="cuda")
        err = H.gwhip_poa_test_add_alignment_parallel(*graph_args, *tail, len(read), max_nodes, s16, scratch.data_ptr(), rc.data_ptr(), None)
    assert err == 0
    torch.cuda.synchronize()
    return int(rc.item()), int(nc.item()), {k: t[k].cpu().numpy() for k in GRAPH_ARRAYS}


def outgoing_lists(arrays, n):
    oc, oe = arrays["outgoing_count"], arrays["outgoing"]
    return [[int(oe[i * E + j]) for j in range(oc[i])] for i in range(n)]


def mirrored(case):
    """The reference's vectors hand the read over back to front (alignment entry k holds read position k, and addAlignment walks
    from the last entry down), while a traceback leaves read position 0 in the LAST entry -- the order the merge of the window
    kernels is a map over. The same vector with the read, its weights and the read positions mirrored is the same sequence of
    (base, weight, graph node) steps for the serial routine, and in traceback order."""
    L = len(case["read"])
    return dict(case, read=case["read"][::-1], weights=case["weights"][::-1],
                alignment_read=[-1 if r < 0 else L - 1 - r for r in case["alignment_read"]])


PARALLEL = ("parallel32", "parallel16")


@pytest.mark.parametrize("which", PARALLEL)
@pytest.mark.parametrize("idx", range(len(V["add_alignment"])))
def test_add_alignment_known_answers_through_the_production_merge(idx, which):
    """Test_CudapoaAddAlignment.cu:127-229 through add_alignment_parallel: the reference's outgoing edges, and graph arrays
    byte-equal to the serial routine's."""
    case = V["add_alignment"][idx]
    m = mirrored(case)
    results = {}
    for name, c in (("serial_as_given", case), ("serial", m), (which, m)):
        state = merge_state(c["nodes"], c["outgoing"], c["coverage"])
        results[name] = run_merge(state, c["read"], c["weights"], c["alignment_graph"], c["alignment_read"], 3072, "serial" if name.startswith("serial") else which)
    for name, (rc, n, arrays) in results.items():
        assert rc == 0, (name, rc)
        assert outgoing_lists(arrays, n) == case["answer"], name
    assert results[which][1] == results["serial"][1]
    for k in GRAPH_ARRAYS:
        assert results[which][2][k].tobytes() == results["serial"][2][k].tobytes(), k
        assert results["serial_as_given"][2][k].tobytes() == results["serial"][2][k].tobytes(), k


def assert_untouched(state, n, arrays):
    assert n == state["count"]
    for k in GRAPH_ARRAYS:
        assert arrays[k].tobytes() == np.ascontiguousarray(state[k]).tobytes(), k


@pytest.mark.parametrize("which", PARALLEL)
@pytest.mark.parametrize("idx", range(len(V["add_alignment"])))
def test_production_merge_hands_an_incomplete_alignment_to_the_serial_routine(idx, which):
    """An alignment that misses a read position (the reference's degenerate traceback result): -1, nothing modified."""
    m = mirrored(V["add_alignment"][idx])
    ar = list(m["alignment_read"])
    ar[[k for k, r in enumerate(ar) if r >= 0][len(m["read"]) // 2]] = -1
    state = merge_state(m["nodes"], m["outgoing"], m["coverage"])
    rc, n, arrays = run_merge(state, m["read"], m["weights"], m["alignment_graph"], ar, 3072, which)
    assert rc == -1
    assert_untouched(state, n, arrays)


@pytest.mark.parametrize("which", PARALLEL)
def test_production_merge_hands_aligned_nodes_on_the_path_to_the_serial_routine(which):
    """A hand-built graph A -> C -> G -> T whose nodes 1 and 2 are aligned to each other, and the read AGGT along it: read
    position 1 (G against C) looks through node 1's aligned nodes and finds node 2, which is on the path itself -- two read
    positions would touch one node. -1, nothing modified; the serial routine takes the read (and reuses node 2 twice)."""
    def state():
        return merge_state("ACGT", [[1], [2], [3], []], [1, 1, 1, 1], aligned={1: [2], 2: [1]})
    ag, ar = [3, 2, 1, 0], [3, 2, 1, 0]
    rc, n, arrays = run_merge(state(), "AGGT", [1, 1, 1, 1], ag, ar, 3072, which)
    assert rc == -1
    assert_untouched(state(), n, arrays)
    rc, n, arrays = run_merge(state(), "AGGT", [1, 1, 1, 1], ag, ar, 3072, "serial")
    assert (rc, n) == (0, 4)
    # without the mutual alignment the same read is the parallel merge's own: a new node for the G at read position 1
    plain = merge_state("ACGT", [[1], [2], [3], []], [1, 1, 1, 1])
    got = run_merge(plain, "AGGT", [1, 1, 1, 1], ag, ar, 3072, which)
    want = run_merge(plain, "AGGT", [1, 1, 1, 1], ag, ar, 3072, "serial")
    assert got[:2] == want[:2] == (0, 5)
    for k in GRAPH_ARRAYS:
        assert got[2][k].tobytes() == want[2][k].tobytes(), k


@pytest.mark.parametrize("which", PARALLEL + ("serial",))
@pytest.mark.parametrize("edges", [48, 49])
@pytest.mark.parametrize("side", ["out", "in"])
def test_merge_edge_slots(side, edges, which):
    """A node with 48 / 49 edges on one side and a read that adds one more: 49 edges are the most a node may hold -- the 50th
    is edge_count_exceeded_maximum_graph_size (5). (out: node 0 -> nodes 1 .. edges, the read goes 0 -> node edges + 1;
    in: nodes 1 .. edges -> node 0, the read comes from node edges + 1.)"""
    far = edges + 1
    nodes = "A" + "C" * edges + "G"
    if side == "out":
        outgoing = [list(range(1, edges + 1))] + [[] for _ in range(edges + 1)]
        read, ag = "AG", [far, 0]
    else:
        outgoing = [[]] + [[0] for _ in range(edges)] + [[]]
        read, ag = "GA", [0, far]
    state = merge_state(nodes, outgoing, [1] * len(nodes))
    rc, n, arrays = run_merge(state, read, [1, 1], ag, [1, 0], 3072, which)
    assert rc == (0 if edges == 48 else 5)
    if rc == 0:
        lists = outgoing_lists(arrays, n)
        assert n == len(nodes) and (lists[0][-1] == far and len(lists[0]) == 49 if side == "out" else lists[far] == [0] and arrays["incoming_count"][0] == 49)


@pytest.mark.parametrize("which", PARALLEL + ("serial",))
@pytest.mark.parametrize("room", [2, 1])
def test_merge_node_budget(room, which):
    """max_nodes_per_graph - room nodes and a read that adds one node: the node count has to stay below max_nodes_per_graph, so
    with room 1 it is node_count_exceeded_maximum_graph_size (4)."""
    max_nodes = 64
    count = max_nodes - room
    nodes = "".join("ACGT"[i % 4] for i in range(count))
    outgoing = [[i + 1] for i in range(count - 1)] + [[]]
    state = merge_state(nodes, outgoing, [1] * count, mx=max_nodes)
    read = nodes[-2:] + "T"  # two bases along the graph's end, one new base behind it
    rc, n, arrays = run_merge(state, read, [1, 1, 1], [-1, count - 1, count - 2], [2, 1, 0], max_nodes, which)
    assert rc == (0 if room == 2 else 4)
    if rc == 0:
        assert n == count + 1 and outgoing_lists(arrays, n)[count - 1] == [count]


@pytest.mark.parametrize("which", PARALLEL + ("serial",))
def test_merge_error_precedence(which):
    """One read that overflows the edge slots (node 0 has 49 out-edges, the read adds a 50th) and the node budget (room for one
    node, the read brings two). The first failing read position wins, and inside one position the node count comes first:
    new nodes in front of the edge -> 4; the edge in front of them -> 5; the second new node is the edge's own end -> 4; the
    first new node is the edge's end, the second follows -> 5."""
    edges = 49
    nodes = "G" + "A" + "C" * edges + "T"          # 0: G (lead-in), 1: the hub A, 2 .. 50: its children, 51: T
    hub, far = 1, edges + 2
    outgoing = [[hub], list(range(2, edges + 2))] + [[] for _ in range(edges + 1)]
    count = len(nodes)
    max_nodes = count + 2                            # count + 1 nodes are the most: room for one

    def run(read, graph_nodes):
        L = len(read)
        state = merge_state(nodes, outgoing, [1] * count, mx=max_nodes)
        return run_merge(state, read, [1] * L, graph_nodes[::-1], list(range(L))[::-1], max_nodes, which)[0]

    assert run("GA" + "T", [0, hub, far]) == 5                        # the edge alone
    assert run("GTTA" + "T", [0, -1, -1, hub, far]) == 4              # two new nodes, then the edge
    assert run("GA" + "T" + "GG", [0, hub, far, -1, -1]) == 5         # the edge, then two new nodes
    assert run("GGA" + "G", [0, -1, hub, -1]) == 4                    # one new node; the second is the end of the hub's 50th edge
    assert run("GA" + "GG", [0, hub, -1, -1]) == 5                    # the first new node is the end of the 50th edge; the second follows
