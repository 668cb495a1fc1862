"""TEST INFRASTRUCTURE: POA windows at the edges of the 16-bit ranges of the cudapoa hot path, shared by
test_poa_int16_edge_cases.py (CPU: the oracle's answer is well defined for every one of them) and test_gpu_poa_int16_edges.py
(GPU: production kernels = general routines = oracle).

The packed forward passes (poa_device.h nw_banded, poa_tb_device.h nw_banded_tb_packed, poa_forward_moves_full.h nw_full_packed)
admit a read when, with G = nodes of the graph and L = bases of the read,

    |gap| <= 30, |match| <= 100, |mismatch| <= 100
    max(match, 0) * min(L, G) + u_span + |match| <= 32767                (A)
    (G + L) * min(gap, mismatch, 0) >= -32768 + 256                      (B)
    -16384 + 4 * min(gap, mismatch, 0) - u_span >= -32768                (C, banded only)
    u_span = max(band_width, 256) * |gap| (banded), 1024 * |gap| (full band)

and hand every other read to the general routines. The functions lhs_a / lhs_b below restate (A) and (B) ONLY TO PLACE INPUTS
next to the edges: every edge is swept over L = edge - 2 .. edge + 2, so a restatement (or a kernel bound) that is off by one
still has windows on both sides of the real edge, and no expected result ever comes from them -- that is the oracle's job.

(C) cannot fail inside the magnitude limits: its left side is smallest at the widest band, the largest |gap| and the largest
penalty, -16384 - 4 * 100 - 512 * 30 = -32144 >= -32768. That corner itself (gap -30, mismatch -100, band 512) admits no read:
a band of 512 columns needs a read of at least 511 bases (max_column >= band_width), and (B) then caps the penalty at
32512 / (511 + G). The cases "C_" below hold that combination (declined, on the admitted side of (A) and (B)) and the
nearest one the packed pass does admit (gap -30, mismatch -31, band 512: (C) = -31868).

Everything is seeded and deterministic; a case is a dict
    id, config (dict: max_seq, max_seqs, band_width, band_mode, gap, mismatch, match, graph_factor), reads, weights (or None),
    identical (the consensus must be reads[0]), kind ("A", "B", "M", "C", "W")
and cases of one config are meant to share one batch."""
import random

BAND_MODES = {"full_band": 0, "static_band": 1, "adaptive_band": 2, "static_band_traceback": 3, "adaptive_band_traceback": 4}
SHORT = {"full_band": "full", "static_band": "static", "adaptive_band": "adaptive", "static_band_traceback": "statictb",
         "adaptive_band_traceback": "adaptivetb"}


def label(config):
    """static256, adaptivetb256 ...; the full band has no width"""
    return "full" if config["band_mode"] == "full_band" else "%s%d" % (SHORT[config["band_mode"]], config["band_width"])


def u_span(config):
    return (1024 if config["band_mode"] == "full_band" else max(config["band_width"], 256)) * abs(config["gap"])


def lhs_a(config, read_length, graph_count):
    return max(config["match"], 0) * min(read_length, graph_count) + u_span(config) + abs(config["match"])


def lhs_b(config, read_length, graph_count):
    return (graph_count + read_length) * min(config["gap"], config["mismatch"], 0)


def last_admitted_identical(config):
    """Largest L for which a read of L bases on a graph of L nodes passes (A)."""
    L = 1
    while lhs_a(config, L + 1, L + 1) <= 32767:
        L += 1
    return L


def last_admitted_b(config, graph_count):
    """Largest L for which a read of L bases on a graph of graph_count nodes passes (B)."""
    L = 1
    while lhs_b(config, L + 1, graph_count) >= -32768 + 256:
        L += 1
    return L


def make_config(band_mode, band_width, max_seq, gap, mismatch, match, max_seqs=6, graph_factor=3.0):
    return dict(max_seq=max_seq, max_seqs=max_seqs, band_width=band_width, band_mode=band_mode, gap=gap, mismatch=mismatch, match=match,
                graph_factor=graph_factor)


def config_key(config):
    return tuple(sorted(config.items()))


def random_read(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def substitute(rng, s, fraction):
    s = list(s)
    for i in rng.sample(range(len(s)), max(1, int(len(s) * fraction))):
        s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
    return "".join(s)


def with_indels(rng, s, fraction):
    """Substitutions, insertions and deletions at `fraction` of the positions, then cut or extended to the length of s."""
    n, s = len(s), list(s)
    for _ in range(max(1, int(n * fraction))):
        i = rng.randrange(1, len(s) - 1)
        op = rng.randrange(3)
        if op == 0:
            s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
        elif op == 1:
            s.insert(i, rng.choice("ACGT"))
        else:
            del s[i]
    s = "".join(s)
    return (s + random_read(rng, n))[:n]


def substitute_every(s, step):
    s = list(s)
    for i in range(step, len(s), step):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1) % 4]
    return "".join(s)


def _case(kind, cid, config, reads, weights=None, identical=False, **extra):
    return dict(kind=kind, id=cid, config=config, reads=reads, weights=weights, identical=identical, **extra)


# (band mode, width, max_seq, match): the table of the edges of (A), gap -4, mismatch -6. The last admitted / first declined
# lengths in the comments are what test_poa_int16_edge_cases.py pins for the restatement above.
UPPER_EDGES = (
    ("static_band", 256, 1024, 31),              # 1022 / 1023
    ("adaptive_band", 256, 1024, 31),
    ("static_band_traceback", 256, 1024, 31),
    ("adaptive_band_traceback", 256, 1024, 31),
    ("static_band", 512, 1024, 31),              # 989 / 990
    ("static_band", 384, 1024, 31),              # 1006 / 1007
    ("full_band", 256, 1024, 31),                # 923 / 924
    ("static_band", 128, 512, 63),               # 502 / 503
    ("static_band", 256, 328, 99),               # 319 / 320
)


def upper_bound_cases():
    """(A): windows of 3 identical random reads (the score really reaches match * L), L swept over the edge; at band 256 and
    match 31 also the longest read of the configuration (1024); windows of mutated copies and asymmetric windows on the edge."""
    out = []
    for mode, width, max_seq, match in UPPER_EDGES:
        cfg = make_config(mode, width, max_seq, -4, -6, match)
        edge = last_admitted_identical(cfg)
        lengths = list(range(edge - 2, edge + 3))
        if max_seq not in lengths and width == 256 and match == 31:
            lengths.append(max_seq)
        for L in lengths:
            r = random_read(random.Random(1000 * match + L), L)
            out.append(_case("A", "A_%s_m%d_L%d_lhs%d" % (label(cfg), match, L, lhs_a(cfg, L, L)), cfg, [r, r, r], identical=True,
                             read_length=L))
    # 3 % mutated copies on the admitted edge: substitutions only (every read has exactly the edge's length and the graph is no
    # smaller, so min(L, G) is the edge), and indels with the copies cut or extended to the edge's length
    for mode, width, max_seq, match in (UPPER_EDGES[0], UPPER_EDGES[2], UPPER_EDGES[6], UPPER_EDGES[7]):
        cfg = make_config(mode, width, max_seq, -4, -6, match)
        edge = last_admitted_identical(cfg)
        rng = random.Random(77 + width + match)
        r = random_read(rng, edge)
        out.append(_case("A", "A_%s_m%d_L%d_lhs%d_substituted" % (label(cfg), match, edge, lhs_a(cfg, edge, edge)), cfg,
                         [r] + [substitute(rng, r, 0.03) for _ in range(3)]))
        out.append(_case("A", "A_%s_m%d_L%d_lhs%d_indels" % (label(cfg), match, edge, lhs_a(cfg, edge, edge)), cfg,
                         [r] + [with_indels(rng, r, 0.03) for _ in range(3)]))
    # asymmetric windows: min(read_length, graph_count) is what admits the second read. A 900-base backbone and a read of
    # 1024 (the backbone with four inserts of 31 bases): 31 * 1024 alone is over the edge, 31 * 900 is not. The third read, a copy
    # of the second, meets a graph of 1024 nodes and is declined: a hand-over inside the window. And the mirror image.
    for mode in ("static_band", "static_band_traceback"):
        cfg = make_config(mode, 256, 1024, -4, -6, 31)
        rng = random.Random(4242)
        backbone = random_read(rng, 900)
        long_read = backbone
        for at in (720, 540, 360, 180):
            long_read = long_read[:at] + random_read(rng, 31) + long_read[at:]
        assert len(long_read) == 1024
        out.append(_case("A", "A_%s256_m31_G900_L1024_lhs%d_not%d" % (SHORT[mode], lhs_a(cfg, 1024, 900), lhs_a(cfg, 1024, 1024)), cfg,
                         [backbone, long_read, long_read]))
        out.append(_case("A", "A_%s256_m31_G1024_L900_lhs%d_not%d" % (SHORT[mode], lhs_a(cfg, 900, 1024), lhs_a(cfg, 1024, 1024)), cfg,
                         [long_read, backbone, backbone]))
    return out


B_SEED = 2


def lower_bound_cases(node_count_after):
    """(B): gap = mismatch = -21, match 8, max_seq 512, 1536 nodes (still int16: lower bound -32256). Five mutually unrelated
    500-mers grow the graph to G nodes -- node_count_after(config, reads) asks the oracle, per band mode -- and a sixth
    unrelated read sits on either side of G + L = 1548: reads 2 to 5 go through the packed pass, the sixth through the
    general routine on the declined side."""
    out = []
    for mode in BAND_MODES:
        cfg = make_config(mode, 256, 512, -21, -21, 8)
        rng = random.Random(B_SEED)
        five = [random_read(rng, 500) for _ in range(5)]
        sixth = random_read(rng, 512)
        G = node_count_after(cfg, five)
        edge = last_admitted_b(cfg, G)
        for L in range(edge - 2, edge + 3):
            out.append(_case("B", "B_%s_g21_G%d_L%d_lhs%d" % (label(cfg), G, L, lhs_b(cfg, L, G)), cfg, five + [sixth[:L]],
                             graph_count=G, read_length=L))
    return out


def _three(r, step=37, cut=7):
    return [r, substitute_every(r, step), r[:-cut]]


def magnitude_cases():
    """Each magnitude limit and one past it: the read, a copy with a substitution every 37 bases, the read cut by 7 bases."""
    out = []
    rng = random.Random(31)
    r300, r150 = random_read(rng, 300), random_read(rng, 150)
    for gap in (-30, -31):
        cfg = make_config("static_band", 256, 328, gap, -6, 8)
        out.append(_case("M", "M_static256_gap%d_L300_lhsA%d_lhsB%d" % (gap, lhs_a(cfg, 300, 300), lhs_b(cfg, 300, 308)), cfg, _three(r300)))
    for match in (100, 101):
        cfg = make_config("static_band", 256, 320, -4, -6, match)
        for L in (316, 317):  # match 100 sits at its own edge of (A)
            r = random_read(random.Random(100 * match + L), L)
            out.append(_case("M", "M_static256_match%d_L%d_lhsA%d" % (match, L, lhs_a(cfg, L, L)), cfg, _three(r)))
    for mismatch in (-100, -101):
        cfg = make_config("static_band", 128, 160, -8, mismatch, 8)
        out.append(_case("M", "M_static128_mismatch%d_L150_lhsB%d_edge-32512" % (mismatch, lhs_b(cfg, 150, 154)), cfg, _three(r150)))
    # (C), see the module docstring: its worst corner, which admits nothing, and the nearest admitted combination
    cfg = make_config("static_band", 512, 520, -30, -100, 8, graph_factor=2.0)
    out.append(_case("C", "C_static512_gap-30_mismatch-100_L150_lhsC-32144_band_wider_than_read", cfg, _three(r150)))
    cfg = make_config("static_band", 512, 520, -30, -31, 8, graph_factor=2.0)
    r515 = random_read(rng, 515)
    out.append(_case("C", "C_static512_gap-30_mismatch-31_L515_lhsC-31868_lhsB%d" % lhs_b(cfg, 515, 515 + 13), cfg, _three(r515)))
    return out


# ---- heavy edge weights ---------------------------------------------------------------------------------------------------
WEIGHT_SEED = 140
WEIGHT_MODES = (("static_band", 128), ("full_band", 128))
WEIGHT_ROWS = ((140, 120), (258, 100), (259, 100))  # (reads of r, reads of v): heaviest edge 35 560, 65 532, 65 786 -> 250


def weight_reads(branches=(70,), length=140):
    """r and its variant v with one substitution per branch position."""
    r = random_read(random.Random(WEIGHT_SEED), length)
    v = list(r)
    for at in branches:
        v[at] = "ACGT"[("ACGT".index(v[at]) + 1) % 4]
    return r, "".join(v)


def weight_cases():
    """Edge weights are uint16 sums of the base weights of the two ends of every traversal, as the reference's are: they pass
    32767 (a sign extension anywhere would show) and wrap at 65536, where the consensus flips from r to v."""
    out = []
    for mode, width in WEIGHT_MODES:
        cfg = make_config(mode, width, 160, -8, -6, 8, max_seqs=400)
        r, v = weight_reads()
        for na, nb in WEIGHT_ROWS:
            reads = [v, r] + [r] * (na - 1) + [v] * (nb - 1)
            out.append(_case("W", "W_%s_r%d_v%d_sum%d" % (label(cfg), na, nb, 254 * na), cfg, reads, [[127] * 140] * len(reads),
                             r=r, v=v, na=na, nb=nb))
        # two branches 40 bases apart: the heavy edges fall into different 64-node chunks of the chunked bundle pass, and behind
        # each branch the heavy edge is not the node's first in-edge (the backbone v came first)
        r2, v2 = weight_reads(branches=(45, 85))
        for na, nb in WEIGHT_ROWS[1:]:
            reads = [v2, r2] + [r2] * (na - 1) + [v2] * (nb - 1)
            out.append(_case("W", "W_%s_r%d_v%d_sum%d_two_branches" % (label(cfg), na, nb, 254 * na), cfg, reads,
                             [[127] * 140] * len(reads), r=r2, v=v2, na=na, nb=nb))
        # Phred-shaped weights: 110 + 90 reads, every base weight drawn from 60 .. 93
        rng = random.Random(93)
        reads = [v, r] + [r] * 109 + [v] * 89
        out.append(_case("W", "W_%s_r110_v90_phred60to93" % label(cfg), cfg, reads,
                         [[rng.randint(60, 93) for _ in range(140)] for _ in reads], r=r, v=v, na=110, nb=90))
    return out


def oracle_cfg(config, output_mask=1):
    """The oracle's BatchConfig(max_seq_sz, max_seq_per_poa, band_width, banding, ...) for a case's config: what
    CudaPoaBatch.from_batch_config builds on the HIP side and RefBatch on the reference's."""
    import oracle_poa as O
    return O.make_cfg(config["max_seq"], config["max_seqs"], config["band_width"], BAND_MODES[config["band_mode"]],
                      graph_factor=config["graph_factor"], gap=config["gap"], mismatch=config["mismatch"], match=config["match"],
                      output_mask=output_mask)


def oracle_node_count_after(config, reads):
    import oracle_poa as O
    with O.Workspace(oracle_cfg(config)) as ws:
        ref = ws.process(reads)
        assert ref["status"] == 0
        return ref["node_count"]


_ALL = {}


def all_cases():
    """Parts 1 and 2, built once per process."""
    if not _ALL:
        _ALL["score"] = upper_bound_cases() + lower_bound_cases(oracle_node_count_after) + magnitude_cases()
        _ALL["weight"] = weight_cases()
    return _ALL["score"], _ALL["weight"]


_ORACLE = {}


def oracle_result(case, output_mask=1):
    """The oracle's answer for a case (computed once per process, with the other cases of its config, and left unchanged):
    Workspace.process's dict plus score32 (the configuration's score type) and overflow (the window's overflow events)."""
    import oracle_poa as O
    if (case["id"], output_mask) not in _ORACLE:
        score, weight = all_cases()
        for config, group in group_by_config(score + weight):
            if config_key(config) != config_key(case["config"]):
                continue
            cfg = oracle_cfg(config, output_mask)
            with O.Workspace(cfg) as ws:
                seen = 0
                for c in group:
                    ref = ws.process(c["reads"], c["weights"])
                    ref["score32"] = int(cfg.score32)
                    ref["overflow"] = ws.overflow_events() - seen
                    seen += ref["overflow"]
                    _ORACLE[c["id"], output_mask] = ref
    return _ORACLE[case["id"], output_mask]


def group_by_config(cases):
    """-> list of (config, [cases]) in first-seen order: one batch per entry."""
    groups = {}
    for c in cases:
        groups.setdefault(config_key(c["config"]), (c["config"], []))[1].append(c)
    return list(groups.values())
