"""The POA kernels at the edges of their 16-bit ranges (windows: poa_int16_edge_cases.py, whose oracle answers
test_poa_int16_edge_cases.py shows to be well defined): the admission bounds of the packed forward passes -- reads swept across
the last admitted and the first declined length of (A) and (B), the magnitude limits of the scores and one past each -- and
edge weights past 32767 and past the uint16 wrap.

Every window runs in three arms that must agree bit for bit: the production kernels, the same batch with GWHIP_DEBUG=256
(packed passes off: every read takes the general routines, whose narrowing stores are checked) and the CPU oracle. A packed
pass that lets a score leave int16 on the admitted side, or an admission bound that is off, shows as a difference; nothing
here knows where the edge is.

Path evidence (that both sides of an edge are really hit) exists for the packed pass of bands 256 and 128 in the
score-matrix modes, through its per-kind row counters; the two-pass bands, the traceback-buffer passes and the full band
have no such counter and rest on the three-arm equality."""
import os
import time

import pytest

import poa_int16_edge_cases as E
from genomeworks_amd import debug_flags as D

pytestmark = pytest.mark.gpu

SCORE_CASES, WEIGHT_CASES = E.all_cases()
GENERAL = D.env_value(D.kDbgNoPackedPasses)  # GWHIP_DEBUG: packed passes off
_GPU = {}


def ids(cases):
    return [c["id"] for c in cases]


def run_batch(config, cases, output_type, env):
    """One batch of all the windows of a config under the given environment -> per window (status, consensus, coverage) or
    (status, msa rows), and the batch's cell count."""
    from genomeworks_amd import cudapoa
    saved = {k: os.environ.get(k) for k in ("GWHIP_DEBUG", "GWHIP_CONSENSUS_SERIAL")}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(env)
        b = cudapoa.CudaPoaBatch.from_batch_config(config["max_seq"], config["max_seqs"], config["band_width"], config["band_mode"], 2 << 30,
                                                   output_type=output_type, gap_score=config["gap"], mismatch_score=config["mismatch"],
                                                   match_score=config["match"], graph_length_factor=config["graph_factor"])
        for c in cases:
            st, seq_st = b.add_poa_group(c["reads"], c["weights"])
            assert st == 0 and not any(seq_st), (c["id"], st, seq_st)
        b.generate_poa()
        if output_type == "msa":
            msa, status = b.get_msa()
            return [(status[i], msa[i]) for i in range(len(cases))], b.total_cells()
        cons, cov, status = b.get_consensus()
        return [(status[i], cons[i], cov[i]) for i in range(len(cases))], b.total_cells()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def gpu_results(case, arms, output_type="consensus"):
    """{arm: (this window's result, the batch's cells)}; every batch (one per config, arm and output type) runs once per
    process, with all the windows of the config in it."""
    key = (E.config_key(case["config"]), output_type)
    group = [c for c in SCORE_CASES + WEIGHT_CASES if E.config_key(c["config"]) == key[0]]
    for name, env in arms:
        if (key, name) not in _GPU:
            t = time.time()
            _GPU[key, name] = run_batch(case["config"], group, output_type, env)
            print("batch %s %s %s: %d windows, %.2f s" % (E.label(case["config"]), output_type, name, len(group), time.time() - t))
    at = ids(group).index(case["id"])
    return {name: (_GPU[key, name][0][at], _GPU[key, name][1]) for name, _ in arms}, group


def oracle_cells(group):
    return sum(E.oracle_result(c)["cells"] for c in group)


SCORE_ARMS = (("production", {}), ("general_routines", {"GWHIP_DEBUG": GENERAL}))


@pytest.mark.parametrize("case", SCORE_CASES, ids=ids(SCORE_CASES))
def test_production_equals_the_general_routines_and_the_oracle(case):
    got, group = gpu_results(case, SCORE_ARMS)
    ref = E.oracle_result(case)
    want = (ref["status"], ref["consensus"], [int(x) for x in ref["coverage"]])
    assert ref["status"] == 0
    for arm, (result, cells) in got.items():
        assert result[0] == want[0], (arm, result[0])
        assert result[1] == want[1], "%s: consensus differs from the oracle's" % arm
        assert result[2] == want[2], "%s: coverage differs from the oracle's" % arm
        assert cells == oracle_cells(group), (arm, cells)
    if case["identical"]:
        assert got["production"][0][1] == case["reads"][0]


MSA_CASES = [c for c in SCORE_CASES if c["id"].startswith(("A_static256_m31_L", "B_static256_"))]


@pytest.mark.parametrize("case", MSA_CASES, ids=ids(MSA_CASES))
def test_msa_output_at_the_edges(case):
    """An (A) sweep and the (B) sweep as MSA output (the MSA instantiations of the graph-build kernel)."""
    got, group = gpu_results(case, SCORE_ARMS, "msa")
    ref = E.oracle_result(case, output_mask=2)
    assert ref["status"] == 0 and ref["overflow"] == 0
    assert [row.replace("-", "") for row in ref["msa"]] == case["reads"]
    for arm, (result, cells) in got.items():
        assert result == (ref["status"], ref["msa"]), arm
        assert cells == got["production"][1], arm


# bit 4: the first bundle pass of the LDS consensus routine node by node instead of in chunks of 64 nodes;
# GWHIP_CONSENSUS_SERIAL=1: the HBM consensus routine (generate_consensus) instead of the LDS one
WEIGHT_ARMS = SCORE_ARMS + (("bundle_pass_node_by_node", {"GWHIP_DEBUG": D.env_value(D.kDbgConsensusNodeByNode)}), ("hbm_consensus_routine", {"GWHIP_CONSENSUS_SERIAL": "1"}))


@pytest.mark.parametrize("case", WEIGHT_CASES, ids=ids(WEIGHT_CASES))
def test_heavy_edge_weights_in_every_consensus_routine(case):
    """Edge weights are uint16 in the graph, two to a word in the LDS consensus pass: sums past 32767 must not pick up a sign and
    sums past 65535 wrap as the reference's do (reference_simt_heavy_weights.json holds its own answers; the CPU test ties the
    oracle to that file)."""
    got, group = gpu_results(case, WEIGHT_ARMS)
    ref = E.oracle_result(case)
    want = (ref["status"], ref["consensus"], [int(x) for x in ref["coverage"]])
    assert ref["status"] == 0
    for arm, (result, cells) in got.items():
        assert result == want, arm
        assert cells == oracle_cells(group), (arm, cells)
    if case["na"] in (258, 259):
        assert got["production"][0][1] == (case["r"] if case["na"] == 258 else case["v"])


# (band mode, width, max_seq, match): configurations whose packed pass counts its rows
COUNTED = (("static_band", 256, 1024, 31), ("adaptive_band", 256, 1024, 31), ("static_band", 128, 512, 63), ("adaptive_band", 128, 512, 63))
DESCRIPTOR_KINDS = range(7)


@pytest.mark.parametrize("mode,width,max_seq,match", COUNTED)
def test_both_sides_of_the_upper_edge_are_hit(mode, width, max_seq, match):
    """Two-read windows [r, r] at the last admitted and at the first declined length: the row counters of the packed pass
    (poa_forward_moves.h: GWHIP_DEBUG bits 28-30 = descriptor kind + 1 with bits 13 and 12, a counted row adds 2^32 or 2^48 to
    its window's "other" counter) summed over the kinds are the read's rows on the admitted side and 0 on the declined side.
    With those bits nothing else writes above bit 32 of that counter: the other users of it are selected by bits 1, 16-18,
    20, 22-24 and 25-27 (merge, topological sort, generic row loop, sink search), bit 12 alone times the prologue only
    without a kind selector, and the phase ticks of a window this small stay far below 2^32."""
    from genomeworks_amd import cudapoa
    import random
    cfg = E.make_config(mode, width, max_seq, -4, -6, match)
    edge = E.last_admitted_identical(cfg)
    assert "GWHIP_DEBUG" not in os.environ
    b = cudapoa.CudaPoaBatch.from_batch_config(max_seq, 6, width, mode, 1 << 30, gap_score=-4, mismatch_score=-6, match_score=match)
    for L in (edge, edge + 1):
        r = E.random_read(random.Random(L), L)
        assert b.add_poa_group([r, r])[0] == 0
    b.generate_poa()
    cons, cov, status = b.get_consensus()
    assert status == [0, 0] and [len(c) for c in cons] == [edge, edge + 1]
    rows = [0, 0]
    try:
        for kind in DESCRIPTOR_KINDS:
            os.environ["GWHIP_DEBUG"] = D.env_value(D.kDbgKindFine, D.kDbgKindCount, row_kind=kind)
            for w, counters in enumerate(b.profile_phases_per_window()):
                rows[w] += ((counters["other"] >> 32) & 0xffff) + (counters["other"] >> 48)
    finally:
        del os.environ["GWHIP_DEBUG"]
    print("rows of the packed pass at L = %d, %d:" % (edge, edge + 1), rows)
    assert rows[0] >= 1 and rows[1] == 0, rows
