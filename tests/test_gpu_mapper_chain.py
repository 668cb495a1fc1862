"""The chaining overlapper on the GPU against its CPU oracle (tests/oracle_mapper_chain.py), records and scores byte
for byte: every edge of rules C1-C8 on hand-built groups, many random groups, the Matcher path, map_reads and the
batched driver with overlapper="chained", what runs downstream of them, and the errors."""
import numpy as np
import pytest

import cigar_replay as R
import mapper_cases as MC
import mapper_chain_cases as CC
import oracle_mapper_chain as OC

pytestmark = pytest.mark.gpu

LIMIT = 30000  # bases per index of the batched runs: several index pairs on the synthetic reads


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def synthetic():
    reads, origin = CC.reads_with_origin(CC.SYNTHETIC_SEED)
    return reads, origin


def same(a, b):
    return MC.overlap_bytes(a) == MC.overlap_bytes(b)


def check(cm, anchors, kw, where):
    """chain_overlaps on the host array equals the oracle in records and scores; returns them"""
    o, s = cm.chain_overlaps(anchors, return_scores=True, **kw)
    ref_o, ref_s = OC.chain_overlaps(anchors, **kw)
    assert o.dtype == cm.OVERLAP and s.dtype == np.int32, where
    assert len(o) == len(ref_o), (where, len(o), len(ref_o))
    assert same(o, ref_o), where
    assert s.tobytes() == ref_s.tobytes(), where
    return o, s


@pytest.mark.parametrize("family", ["group_size_cases", "look_back_cases", "tie_cases", "bound_cases",
                                    "orientation_cases", "extraction_cases"])
def test_hand_built_cases(cm, family):
    kept = 0
    for name, anchors, kw in getattr(CC, family)():
        kept += len(check(cm, anchors, kw, name)[0])
    assert kept > 0


def test_look_back_edge_is_taken_at_64_and_not_at_65(cm):
    (_, a64, kw), (_, a65, _) = CC.look_back_cases()
    plus = lambda o: o[o["relative_strand"] == ord("+")]
    got = plus(check(cm, a64, kw, "64 back")[0])
    assert len(got) == 1 and int(got[0]["num_residues"]) == 2 and int(got[0]["query_start_position_in_read"]) == 100
    assert len(plus(check(cm, a65, kw, "65 back")[0])) == 0


def test_interleaved_diagonals(cm):
    a = CC.interleaved_diagonals()
    o, s = check(cm, a, dict(max_chains=2), "M = 2")
    assert s.tolist() == [90, 90] and o["target_start_position_in_read"].tolist() == [1000, 9000]
    o, s = check(cm, a, dict(max_chains=1), "M = 1")
    assert s.tolist() == [90] and o["target_start_position_in_read"].tolist() == [1000]
    assert len(cm.find_overlaps(a)) == 0  # the triggered overlapper returns no record for the pair


@pytest.mark.parametrize("all_to_all", [True, False])
def test_many_groups(cm, all_to_all):
    a = CC.many_groups()
    sizes = np.diff([lo for lo, _ in OC.groups_of(a)] + [len(a)])
    starts = np.cumsum(sizes)[:-1]
    assert len(sizes) >= 290 and 15000 < len(a) < 30000
    for unit in (64, 256):
        assert {0, 1, unit - 1} <= set((starts % unit).tolist())
    assert np.any(a["query_read_id"] == a["target_read_id"])
    for kw in ({}, dict(CC.KEEP_ALL), dict(CC.KEEP_ALL, min_chain_score=0, max_chains=64),
               dict(max_gap=300, bandwidth=20, max_chains=2, kmer_size=19)):
        o, _ = check(cm, a, dict(kw, all_to_all=all_to_all), "many groups %s" % kw)
        assert len(o) > 50
        assert bool(np.any(o["query_read_id"] == o["target_read_id"])) == (not all_to_all)


def test_matcher_path(cm, synthetic):
    reads, origin = synthetic
    with cm.Index(reads, 15, 10, True, 1.0) as index, cm.Matcher(index, index) as m:
        o, s = cm.chain_overlaps(m, return_scores=True)
        assert m.stage_ms["chain_dp"] > 0.0
        a = m.anchors()
        o2, s2 = check(cm, a, {}, "synthetic reads")
        assert same(o, o2) and s.tobytes() == s2.tobytes()
        assert same(cm.chain_overlaps(m), o)
    truth = CC.true_pairs(origin, 1000)
    found = {(int(r["query_read_id"]), int(r["target_read_id"]), chr(r["relative_strand"])) for r in o}
    assert all((q, t, strand) in found for (q, t), strand in truth.items())


def test_map_reads_chained(cm, synthetic):
    reads = synthetic[0]
    half = len(reads) // 2
    chaining = dict(max_gap=2000, bandwidth=300, min_chain_score=50, max_chains=2)
    for queries, targets in ((reads, None), (reads[:half], reads[half:])):
        with cm.Index(queries, 15, 10, True, 1.0) as q, \
                (q if targets is None else cm.Index(targets, 15, 10, True, 1.0)) as t, cm.Matcher(q, t) as m:
            composed = cm.chain_overlaps(m, 15, all_to_all=targets is None)
            composed2 = cm.chain_overlaps(m, 15, all_to_all=targets is None, **chaining)
        got = cm.map_reads(queries, targets, filtering_parameter=1.0, overlapper="chained")
        assert len(got) > 20 and same(got, composed)
        got = cm.map_reads(queries, targets, filtering_parameter=1.0, overlapper="chained", chaining=chaining)
        assert same(got, composed2) and not same(composed, composed2)
    with pytest.raises(ValueError):
        cm.map_reads(reads, overlapper="minimap")
    with pytest.raises(ValueError):
        cm.map_reads_batched(reads, overlapper="")
    with pytest.raises(ValueError):
        cm.map_reads(reads, chaining=chaining)  # chaining values without the chained overlapper
    with pytest.raises(ValueError):
        cm.map_reads(reads, overlapper="chained", chaining=dict(gap=5))


def composed_pairs(cm, queries, targets, chaining, after=lambda o: o):
    """what the batched driver does with overlapper="chained", from its parts: index pairs in driver order, each
    through Index, Matcher, chain_overlaps and `after`"""
    all_to_all = targets is None
    groups_q = cm.group_reads_into_indices([len(r) for r in queries], LIMIT)
    groups_t = groups_q if all_to_all else cm.group_reads_into_indices([len(r) for r in targets], LIMIT)
    out = []
    for fq, nq in groups_q:
        for ft, nt in groups_t:
            if nq == 0 or nt == 0 or (all_to_all and ft < fq):
                continue
            t_reads = queries if all_to_all else targets
            with cm.Index(queries[fq:fq + nq], 15, 10, True, 1.0, first_read_id=fq) as q, \
                    cm.Index(t_reads[ft:ft + nt], 15, 10, True, 1.0, first_read_id=ft) as t, cm.Matcher(q, t) as m:
                out.append(after(cm.chain_overlaps(m, 15, all_to_all=all_to_all, **chaining)))
    assert len(out) >= 3
    return np.concatenate(out)


def test_map_reads_batched_chained(cm, synthetic):
    reads = synthetic[0]
    half = len(reads) // 2
    common = dict(filtering_parameter=1.0, max_basepairs_per_index=LIMIT, overlapper="chained")
    chaining = dict(max_chains=2, min_chain_score=60)
    timings = {}
    got = cm.map_reads_batched(reads, post_process=False, timings=timings, **common)
    assert len(got) > 100 and timings["index_pairs"] >= 3 and timings["chain_fuse_filter"] > 0.0
    assert same(got, composed_pairs(cm, reads, None, {}))
    got = cm.map_reads_batched(reads[:half], reads[half:], post_process=False, chaining=chaining, **common)
    assert len(got) > 20 and same(got, composed_pairs(cm, reads[:half], reads[half:], chaining))
    # post-processing, end rescue and alignment behind the chaining, once each
    got = cm.map_reads_batched(reads, post_process=True, **common)
    assert same(got, composed_pairs(cm, reads, None, {}, cm.post_process_overlaps))
    got = cm.map_reads_batched(reads, post_process=False, rescue_overlap_ends=True, **common)
    assert same(got, composed_pairs(cm, reads, None, {}, lambda o: cm.rescue_overlap_ends(o, reads)))
    got, cigars = cm.map_reads_batched(reads, post_process=False, align=True, **common)
    assert same(got, composed_pairs(cm, reads, None, {}))
    assert cigars == cm.align_overlaps(got, reads)[0]


def test_the_default_overlapper_is_unchanged(cm, synthetic):
    reads = synthetic[0]
    a = cm.map_reads_batched(reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT)
    b = cm.map_reads_batched(reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT, overlapper="triggered")
    assert len(a) > 50 and same(a, b)
    import oracle_mapper_postprocess as P
    assert same(a, P.map_batched(reads, None, 15, 10, 1.0, MC.OVERLAP_PARAMS, LIMIT))
    assert same(cm.map_reads(reads, filtering_parameter=1.0),
                cm.map_reads(reads, filtering_parameter=1.0, overlapper="triggered"))
    import oracle_mapper as O
    assert same(cm.map_reads(reads, filtering_parameter=1.0), O.map_reads(reads, None, 15, 10, 1.0))


def test_downstream_of_chained_overlaps(cm, synthetic):
    reads = synthetic[0]
    o = cm.map_reads(reads, filtering_parameter=1.0, overlapper="chained")
    assert {chr(x) for x in o["relative_strand"]} == {"+", "-"}
    cigars, edits = cm.align_overlaps(o, reads)
    names, lengths = ["read_%d" % i for i in range(len(reads))], [len(r) for r in reads]
    by_name = dict(zip(names, reads))
    lines = cm.format_paf(o, names, lengths, names, lengths, 15, cigars=cigars).splitlines()
    assert len(lines) == len(o) > 100
    for line, e in zip(lines, edits):
        assert R.replay_paf(line, by_name, by_name).edits == e, line
    from genomeworks_amd import polisher
    # the switch travels in polish()'s mapping parameters, the keywords it hands to map_reads_batched
    targets, timings = reads[:2], {}
    polished, report = polisher.polish(reads[2:], targets, timings=timings, overlapper="chained",
                                       chaining=dict(max_chains=2))
    assert len(polished) == len(targets) and all(isinstance(p, str) and p for p in polished)
    assert timings["chain_fuse_filter"] > 0.0 and timings["index_pairs"] == 1


def test_cudamapper_tool_with_chain_prints_the_chained_overlaps(cm, synthetic, tmp_path):
    import os
    import subprocess
    reads = synthetic[0]
    names, lengths = ["read_%d" % i for i in range(len(reads))], [len(r) for r in reads]
    fasta = tmp_path / "reads.fasta"
    fasta.write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genomeworks_amd", "bin", "cudamapper")
    run = subprocess.run([tool, "-i", str(LIMIT / 1e6), "--chain", "--chain-max-chains", "2", "--chain-min-score", "60",
                          str(fasta), str(fasta)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    # less than 0.5 Mbp of input: the tool turns the frequency filter off; it always post-processes
    o = cm.map_reads_batched(reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT, overlapper="chained",
                             chaining=dict(max_chains=2, min_chain_score=60))
    assert len(o) > 100 and run.stdout == cm.format_paf(o, names, lengths, names, lengths, 15)
    plain = cm.map_reads_batched(reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT)
    assert run.stdout != cm.format_paf(plain, names, lengths, names, lengths, 15)


def test_errors_write_nothing(cm):
    a = CC.interleaved_diagonals()
    assert len(cm.chain_overlaps(a)) == 2
    for bad in (dict(max_gap=0), dict(bandwidth=-1), dict(max_chains=0), dict(max_chains=65), dict(kmer_size=33),
                dict(kmer_size=0), dict(min_chain_score=-1), dict(min_residues=-1), dict(min_overlap_len=-1),
                dict(min_bases_per_residue=-1)):
        with pytest.raises(cm.MapperError):
            cm.chain_overlaps(a, **bad)
    # through the C entry point: the output arrays stay as they were
    import ctypes as C
    from genomeworks_amd import _native
    L = _native.mapper()
    out, scores = np.full(8, 0xAB, np.uint8).repeat(36).view(cm.OVERLAP), np.full(8, -7, np.int32)
    before = out.tobytes()
    for chaining in ([15, 0, 500, 40, 4], [15, 5000, -1, 40, 4], [15, 5000, 500, 40, 0], [15, 5000, 500, 40, 65],
                     [33, 5000, 500, 40, 4]):
        c = np.array(chaining, np.int32)
        ms = C.c_float(-1.0)
        n = L.gw_mapper_chain_overlaps_host(a.ctypes.data_as(C.c_void_p), len(a), c.ctypes.data_as(C.c_void_p), 1, 3,
                                            250, 1000, 0.8, out.ctypes.data_as(C.c_void_p),
                                            scores.ctypes.data_as(C.c_void_p), 8, C.byref(ms), None)
        assert n < 0 and out.tobytes() == before and scores.tolist() == [-7] * 8, chaining
        assert b"gwm_chain_overlaps" in L.gw_mapper_last_error()
    # capacity cuts what is written, not what is counted
    c = np.array([15, 5000, 500, 40, 4], np.int32)
    n = L.gw_mapper_chain_overlaps_host(a.ctypes.data_as(C.c_void_p), len(a), c.ctypes.data_as(C.c_void_p), 1, 3, 250,
                                        1000, 0.8, out.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), 1,
                                        None, None)
    assert n == 2 and scores.tolist() == [90] + [-7] * 7 and out[1:].tobytes() == before[36:]


def test_empty_input(cm):
    o, s = cm.chain_overlaps(np.zeros(0, cm.ANCHOR), return_scores=True)
    assert len(o) == 0 and len(s) == 0 and o.dtype == cm.OVERLAP
    assert len(cm.map_reads_batched([], max_basepairs_per_index=100, overlapper="chained")) == 0
