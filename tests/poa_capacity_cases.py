"""TEST INFRASTRUCTURE: POA windows at the capacity edges of a graph, where a window ends with a failure status instead of a
result -- shared by test_poa_capacity_cases.py (CPU: the generators reach both sides of every edge in the oracle) and
test_gpu_poa_capacity.py (GPU: the kernels give the oracle's status and, where that is 0, its output).

    class    edge                                                                     failure status
    E_out    50 edge slots of a node, out-degree (reads that delete 1 .. K bases behind one node)         5
    E_in     the same, in-degree (deletions of 1 .. K bases in front of one node)                        5
    N        max_nodes_per_graph, reached inside a read (insertions, or substitutions: aligned nodes)    4
    N_pre    max_nodes_per_graph, the check in front of a read (`node_count >= max_nodes_per_graph`)     4
    P        precedence: one read that overflows the edge slots AND the node budget                 4 or 5
    S6       adaptive band, adaptive_storage_factor 1.0: the widened band leaves the score matrix        6
    X_cons   max_consensus_size around the consensus length (output kernel)                              2
    X_msa    max_consensus_size around the MSA row length (output kernel)                                2

NO expected status is written here: the oracle supplies it, and test_poa_capacity_cases.py asserts that every class holds
status 0 and its failure status (P: both 4 and 5), that the failing E windows fail with 5 and not with 4, and that
add_poa_group's own limits refuse nothing. Every edge is swept (side = "below" / "at" / "above" is where the construction
expects it, a label only), so a kernel bound that is off by one has windows on both sides of the real edge.

Three instantiations of the graph merge (dispatch: launch_msa_split / poa_window_kernel in csrc/gwhip_poa.hip), key "merge":
    lds      LDS tables: max_nodes_per_graph <= 3072 and max_sequence_size <= 2032 -- add_alignment_parallel, 16-bit scratch
    matrix   beyond the LDS tables, static / adaptive band -- add_alignment_parallel<.., int32_t>, scratch in the score matrix.
             BatchConfig(1025, ..) is the smallest max_sequence_size that leaves the tables with the default
             graph_length_factor of 3 (3 * 1025 aligned to 4 = 3076 nodes)
    serial   beyond the LDS tables, traceback-buffer modes and full band -- add_alignment_to_graph only
The serial routine also takes over inside the first two when the parallel merge returns -1 (incomplete alignment, aligned
nodes on the alignment path).

N_pre holds first reads of max_nodes_per_graph - 1 and max_nodes_per_graph bases (max_nodes_per_graph == max_sequence_size,
the smallest the all-explicit BatchConfig admits). A first read of max_nodes_per_graph + 1 bases cannot be handed over:
add_poa_group refuses a read longer than max_sequence_size, the all-explicit BatchConfig refuses max_nodes_per_graph <
max_sequence_size, and a graph_length_factor below 1 would make the backbone itself (kernel and oracle alike) write past
arrays sized by max_nodes_per_graph.

Statuses 7 (exceeded_maximum_predecessor_distance) and 8 (loop_count_exceeded_upper_bound): NOT REACHED, no GPU case.
7 needs a forward pass that leaves no sink with a score within the last max_banded_pred_distance rows of the topological
order; the last row of the order is always a sink and its band always holds the last column. 8 needs a traceback or a
consensus walk that runs in a circle. Grid searched with the oracle (all status 0): static_band_traceback and
adaptive_band_traceback x band 128, 256 x max_banded_pred_distance 1, 2, 3, 4, 8, 16, 32, 64, 127, 128, 200 x 12 windows
of max_sequence_size 512 (four each of: synthetic.generate_window(100 + seed, 300, 8, 20, 10, 10); a 320-base backbone with
a dangling 100-base branch behind position 300, a copy of the branch inserted at position 40 and a half branch; a 300-base
backbone with six reads that insert 10 + 15 k bases and delete 5 k bases at 50 + 20 k), and both modes x band 128 x distance
2 .. 64 on a 300-base backbone with insertions of 1 .. 70 and deletions of up to 60 bases.

Everything is seeded and deterministic; a case is a dict
    id, class, side, merge, output ("consensus" | "msa"), config, reads
and the cases of one (config, output) are meant to share one batch."""
import random

BAND_MODES = {"full_band": 0, "static_band": 1, "adaptive_band": 2, "static_band_traceback": 3, "adaptive_band_traceback": 4}
SHORT = {"full_band": "full", "static_band": "static", "adaptive_band": "adaptive", "static_band_traceback": "statictb",
         "adaptive_band_traceback": "adaptivetb"}
FAILURE = {"E_out": (5,), "E_in": (5,), "N": (4,), "N_pre": (4,), "P": (4, 5), "S6": (6,), "X_cons": (2,), "X_msa": (2,)}
MAX_EDGES = 50  # CUDAPOA_MAX_NODE_EDGES


def make_config(band_mode, max_seq, max_seqs, band_width=256, graph_factor=3.0, storage_factor=2.0, max_nodes=None, max_consensus=None):
    """max_nodes / max_consensus None: BatchConfig(max_seq, max_seqs, band_width, band_mode, storage_factor, graph_factor)
    (CudaPoaBatch.from_batch_config); else the all-explicit BatchConfig with these two and the other dimensions as the first
    constructor derives them."""
    return dict(band_mode=band_mode, max_seq=max_seq, max_seqs=max_seqs, band_width=band_width, graph_factor=graph_factor,
                storage_factor=storage_factor, max_nodes=max_nodes, max_consensus=max_consensus)


def config_key(config):
    return tuple(sorted((k, -1 if v is None else v) for k, v in config.items()))


def merge_of(config, max_nodes):
    if max_nodes <= 3072 and config["max_seq"] <= 2032:
        return "lds"
    return "matrix" if config["band_mode"] in ("static_band", "adaptive_band") else "serial"


def oracle_cfg(config, output_mask=1):
    """The oracle's config of a case: what the HIP side builds from the same numbers (test_gpu_poa_capacity.make_batch)."""
    import oracle_poa as O
    cfg = O.make_cfg(config["max_seq"], config["max_seqs"], config["band_width"], BAND_MODES[config["band_mode"]],
                     storage_factor=config["storage_factor"], graph_factor=config["graph_factor"], output_mask=output_mask)
    if config["max_nodes"] is not None:
        assert config["max_nodes"] % 4 == 0  # the explicit constructor aligns it up to 4
        cfg.max_nodes_per_graph = config["max_nodes"]
    if config["max_consensus"] is not None:
        cfg.max_consensus_size = config["max_consensus"]
    O.lib().poa_cfg_select_types(cfg)
    return cfg


def random_read(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def no_equal_neighbours(rng, n, alphabet, prev):
    out = []
    for _ in range(n):
        prev = rng.choice([c for c in alphabet if c != prev])
        out.append(prev)
    return "".join(out)


def _case(cls, cid, side, config, reads, output="consensus"):
    from_cfg = oracle_cfg(config)
    return {"class": cls, "id": "%s_%s" % (cid, output), "side": side, "config": config, "reads": reads, "output": output,
            "merge": merge_of(config, from_cfg.max_nodes_per_graph)}


def side_of(value, last_good):
    return "below" if value < last_good else ("at" if value == last_good else "above")


# ---- E: edge slots ---------------------------------------------------------------------------------------------------------
def edge_backbone(head=99, tail=200, seed=1):
    """`head` random bases, "A", 80 bases over C/G/T with no two equal neighbours, `tail` random bases: a deletion that starts
    behind the "A" (or ends in front of position head + 81) has one optimal placement."""
    rng = random.Random(seed)
    return random_read(rng, head) + "A" + no_equal_neighbours(rng, 80, "CGT", "A") + random_read(rng, tail)


def edge_reads(direction, K, bb, head=99):
    """bb and K reads that delete d = 1 .. K bases: behind node `head` (out-degree K + 1) or in front of node head + 81
    (in-degree K + 1)."""
    if direction == "out":
        return [bb] + [bb[:head + 1] + bb[head + 1 + d:] for d in range(1, K + 1)]
    return [bb] + [bb[:head + 81 - d] + bb[head + 81:] for d in range(1, K + 1)]


SIZES = (("short", 1024), ("beyond_lds", 1025))  # max_sequence_size: LDS tables / the smallest beyond them


def edge_cases():
    out = []
    bb = edge_backbone()
    for size, max_seq in SIZES:
        for mode in BAND_MODES:
            cfg = make_config(mode, max_seq, 100)
            for direction in ("out", "in"):
                for K in range(46, 52):
                    for output in ("consensus", "msa"):
                        out.append(_case("E_" + direction, "E_%s_%s_%s_K%d" % (direction, SHORT[mode], size, K), side_of(K, 48), cfg,
                                         edge_reads(direction, K, bb), output))
    return out


# ---- N: node count ---------------------------------------------------------------------------------------------------------
def node_cases():
    out = []
    # short reads: max_seq 256, graph_length_factor 1.5 -> 384 nodes. 200 bases over G/T, four reads that insert 40 bases over
    # A/C each, a last read that inserts `extra` at position 190: 360 + extra nodes
    rng = random.Random(5)
    bb = random_read(rng, 200, "GT")
    grown = [bb] + [bb[:at] + random_read(rng, 40, "AC") + bb[at:] for at in (30, 70, 110, 150)]
    for mode in BAND_MODES:
        cfg = make_config(mode, 256, 8, band_width=128, graph_factor=1.5)
        for extra in range(20, 26):
            last = bb[:190] + random_read(random.Random(77), extra, "AC") + bb[190:]
            out.append(_case("N", "N_%s_short_extra%d" % (SHORT[mode], extra), side_of(extra, 23), cfg, grown + [last]))
    # beyond the LDS tables: max_seq 1025 -> 3076 nodes. 1000 x "T", 1000 x "A" and 1000 x "C" (2000 new nodes, each aligned
    # to its backbone node: the merge's aligned-node lists; one letter per read, so that no shifted alignment finds a match),
    # a last read that begins with `extra` x "G": 3000 + extra nodes
    bb = "T" * 1000
    grown = [bb, "A" * 1000, "C" * 1000]
    for mode in BAND_MODES:
        cfg = make_config(mode, 1025, 8)
        for extra in range(73, 79):
            last = "G" * extra + bb[extra:]
            out.append(_case("N", "N_%s_beyond_lds_extra%d" % (SHORT[mode], extra), side_of(extra, 75), cfg, grown + [last]))
    # the check in front of a read: max_nodes_per_graph == max_sequence_size == 256, a first read of 255 and of 256 bases and
    # one more read (a copy: no new node either way)
    for mode in BAND_MODES:
        cfg = make_config(mode, 256, 8, band_width=128, max_nodes=256, max_consensus=512)
        for n in (255, 256):
            r = random_read(random.Random(9), n)
            out.append(_case("N_pre", "Npre_%s_first%d_of256" % (SHORT[mode], n), side_of(n, 255), cfg, [r, r[:200]]))
    return out


# ---- P: precedence ---------------------------------------------------------------------------------------------------------
P_INSERT = "ACGTTGCAAC"


def precedence_last_reads(bb, head=99):
    """name -> (side, last read) on top of an E_out window stopped at K = 48 (node `head` has 49 out-edges: the next new one
    overflows) with room for three more nodes. bb[:head + 1] + bb[head + 50:] is the read that creates that edge."""
    a, b = bb[:head + 1], bb[head + 50:]
    return {
        "three_nodes_no_edge": ("below", bb[:50] + P_INSERT[:3] + bb[50:300] + bb[303:]),      # fits: status 0
        "edge_alone": ("above", a + b),
        "nodes_before_edge": ("above", bb[:50] + P_INSERT + bb[50:head + 1] + b),              # node overflow at an earlier read position
        "edge_before_nodes": ("above", a + b[:101] + P_INSERT + b[101:]),                      # edge overflow at an earlier read position
        "both_at_one_position": ("above", bb[:50] + P_INSERT[:3] + bb[50:head + 1] + "AAAAAA" + b),  # the 4th new node is the edge's end
        "edge_one_position_earlier": ("above", bb[:50] + P_INSERT[:2] + bb[50:head + 1] + "AAAAAA" + b),  # 3rd new node: edge; 4th: nodes
    }


def precedence_cases(node_count_after):
    out = []
    # LDS tables: the E_out window itself (380 nodes), max_nodes_per_graph = 384 by the explicit constructor
    bb = edge_backbone()
    base = edge_reads("out", 48, bb)
    for mode in BAND_MODES:
        cfg = make_config(mode, 380, 100, max_nodes=384, max_consensus=760)
        for name, (side, last) in precedence_last_reads(bb).items():
            out.append(_case("P", "P_%s_short_%s" % (SHORT[mode], name), side, cfg, base + [last]))
    # beyond the LDS tables the graph has to hold more than 3072 nodes: the same 180 bases with a tail of 820 x "T", grown
    # by three copies whose tail is all A, all C and all G (2460 nodes aligned to the tail's) before the 48 deletions. The
    # node count G comes from the oracle (roomy config), graph_length_factor is then chosen so that max_nodes_per_graph =
    # G + 4 rounded down to a multiple of 4: room for 3 nodes at the most
    bb = edge_backbone(tail=0, seed=2) + "T" * 820
    grown = [bb] + [bb[:180] + x * 820 for x in "ACG"]
    base = grown + edge_reads("out", 48, bb)[1:]
    for mode in BAND_MODES:
        G = node_count_after(make_config(mode, 1025, 100, graph_factor=4.0), base)
        max_nodes = (G + 4) & ~3
        assert max_nodes > 3072, (mode, G)
        cfg = make_config(mode, 1025, 100, graph_factor=(max_nodes + 0.5) / 1025)
        assert oracle_cfg(cfg).max_nodes_per_graph == max_nodes
        for name, (side, last) in precedence_last_reads(bb).items():
            if name in ("three_nodes_no_edge", "nodes_before_edge", "edge_before_nodes", "both_at_one_position"):
                out.append(_case("P", "P_%s_beyond_lds_G%d_of%d_%s" % (SHORT[mode], G, max_nodes, name), side, cfg, base + [last]))
    return out


# ---- S6: adaptive band storage -----------------------------------------------------------------------------------------------
def storage_cases():
    """adaptive_storage_factor 1.0 (the score matrix holds one band width per row): 446-base backbone, a read with a 60-base
    deletion, a last read that is a prefix of the backbone -- the shorter it is, the further the band has to be widened."""
    out = []
    bb = random_read(random.Random(13), 446)
    for mode in ("adaptive_band", "adaptive_band_traceback"):
        cfg = make_config(mode, 448, 8, band_width=128, graph_factor=1.5, storage_factor=1.0)
        for L in range(358, 370, 2):  # (the rule is not monotone in L: 370 fails again; the sweep stops in front of it)
            out.append(_case("S6", "S6_%s_factor1_prefix%d" % (SHORT[mode], L), side_of(-L, -366), cfg, [bb, bb[:200] + bb[260:], bb[:L]]))
    return out


# ---- X: output size ----------------------------------------------------------------------------------------------------------
X_CONSENSUS_LENGTH = 180


def output_cases(length_of):
    """Two reads x[:150] and three reads x[30:]: consensus and MSA rows (180 columns) are longer than max_sequence_size (152),
    so max_consensus_size one below, at and one above their length is a valid BatchConfig. length_of(config, reads, output) asks
    the oracle (roomy config) for the length."""
    out = []
    x = random_read(random.Random(21), X_CONSENSUS_LENGTH)
    reads = [x[:150], x[:150], x[30:], x[30:], x[30:]]
    for mode in ("static_band", "full_band", "adaptive_band_traceback"):
        for cls, output in (("X_cons", "consensus"), ("X_msa", "msa")):
            n = length_of(make_config(mode, 152, 8, band_width=128), reads, output)
            for size in (n - 1, n, n + 1, n + 2):
                cfg = make_config(mode, 152, 8, band_width=128, max_nodes=456, max_consensus=size)
                out.append(_case(cls, "%s_%s_length%d_max%d" % (cls, SHORT[mode], n, size), side_of(-size, -(n + 1)), cfg, reads, output))
    return out


# ---- short windows for the persistent grid -------------------------------------------------------------------------------------
PERSISTENT_CONFIG = make_config("static_band", 128, 52, band_width=128, graph_factor=1.5)  # 192 nodes


def persistent_windows(count, seed=4000):
    """`count` windows of 90-base reads for one batch of PERSISTENT_CONFIG: three-read windows with a few substitutions and
    one-base indels, and scattered among them (every 97th and every 131st) E_out windows on a 90-base backbone (K = 49) and
    N windows (three reads that insert 30 bases each, a last one that inserts 14). -> list of (kind, reads)."""
    out = []
    ebb = edge_backbone(head=19, tail=0, seed=3)[:90]
    rng = random.Random(seed + 1)
    nbb = random_read(rng, 90, "GT")
    n_reads = [nbb] + [nbb[:at] + random_read(rng, 30, "AC") + nbb[at:] for at in (20, 40, 60)] + [nbb[:80] + random_read(rng, 14, "AC") + nbb[80:]]
    for w in range(count):
        if w % 97 == 5:
            out.append(("E", edge_reads("out", 49, ebb, head=19)))
        elif w % 131 == 7:
            out.append(("N", n_reads))
        else:
            rng = random.Random(seed + 10 * w)
            r = random_read(rng, 90)
            reads = [r]
            for _ in range(2):
                s = list(r)
                for _ in range(3):
                    i = rng.randrange(1, len(s) - 1)
                    op = rng.randrange(3)
                    if op == 0:
                        s[i] = rng.choice("ACGT")
                    elif op == 1:
                        s.insert(i, rng.choice("ACGT"))
                    else:
                        del s[i]
                reads.append("".join(s))
            out.append(("ok", reads))
    return out


# ---- the oracle's answers ----------------------------------------------------------------------------------------------------
def oracle_node_count_after(config, reads):
    import oracle_poa as O
    with O.Workspace(oracle_cfg(config)) as ws:
        ref = ws.process(reads)
        assert ref["status"] == 0, ref["status"]
        return ref["node_count"]


def oracle_output_length(config, reads, output):
    import oracle_poa as O
    with O.Workspace(oracle_cfg(config, 1 if output == "consensus" else 2)) as ws:
        ref = ws.process(reads)
        assert ref["status"] == 0, ref["status"]
        return len(ref["consensus"]) if output == "consensus" else len(ref["msa"][0])


_ALL = []


def all_cases():
    """Built once per process."""
    if not _ALL:
        _ALL.extend(edge_cases() + node_cases() + precedence_cases(oracle_node_count_after) + storage_cases() +
                    output_cases(oracle_output_length))
        assert len({c["id"] for c in _ALL}) == len(_ALL)
    return _ALL


def group_by_batch(cases):
    """-> list of (config, output, [cases]) in first-seen order: one batch per entry."""
    groups = {}
    for c in cases:
        groups.setdefault((config_key(c["config"]), c["output"]), (c["config"], c["output"], []))[2].append(c)
    return list(groups.values())


_ORACLE = {}


def oracle_window(config, reads, output):
    import oracle_poa as O
    with O.Workspace(oracle_cfg(config, 1 if output == "consensus" else 2)) as ws:
        return ws.process(reads)


def oracle_result(case):
    """The oracle's answer for a case (Workspace.process's dict), computed once per process and left unchanged."""
    if case["id"] not in _ORACLE:
        _ORACLE[case["id"]] = oracle_window(case["config"], case["reads"], case["output"])
    return _ORACLE[case["id"]]
