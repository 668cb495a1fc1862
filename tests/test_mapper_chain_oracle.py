"""The CPU oracle of the chaining overlapper (tests/oracle_mapper_chain.py) against answers that do not come from it:
the optimum by enumeration, a copy of itself without the look-back, gap costs worked out by hand, the interleaved
diagonals the triggered overlapper cannot see, reads of known origin; and the exported symbols of the feature. No
GPU."""
import itertools
import os
import re

import numpy as np

import mapper_chain_cases as CC
import oracle_mapper as O
import oracle_mapper_chain as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_groups():
    rng = np.random.default_rng(3)
    for n in range(60):
        m = int(rng.integers(1, 11))
        a = CC.anchors_of(CC.random_group(rng, m, 0, 1))
        # close together, so that most pairs may chain
        q = np.sort(rng.integers(0, 400, m))
        t = rng.integers(0, 400, m)
        yield n, ([int(x) for x in a["query_position_in_read"]], [int(x) for x in a["target_position_in_read"]])
        order = np.lexsort((t, q))
        yield n, ([int(x) for x in q[order]], [int(x) for x in t[order]])


def best_by_enumeration(q, t, sign, k, max_gap, bandwidth):
    """the best score of any subset of the anchors that is a chain by C3 / C4 (consecutive members chain, any
    distance apart in sort order), a single anchor scoring k"""
    best = 0
    for size in range(1, len(q) + 1):
        for subset in itertools.combinations(range(len(q)), size):
            score = k
            for j, i in zip(subset, subset[1:]):
                dq, dt = q[i] - q[j], sign * (t[i] - t[j])
                if not OC.may_precede(dq, dt, max_gap, bandwidth):
                    break
                score += OC.gain(dq, dt, k)
            else:
                best = max(best, score)
    return best


def test_scores_are_the_optimum_by_enumeration():
    chained = 0
    for n, (q, t) in small_groups():
        for sign in (1, -1):
            f, p = OC.scores(q, t, sign, 15, 300, 100)
            # f(i) is the best chain that ends in i or k; a chain scoring below k anywhere is not continued, so the
            # enumeration may only beat it by a chain with a prefix below k -- and such a chain is beaten by its suffix
            assert max(f) == best_by_enumeration(q, t, sign, 15, 300, 100), (n, sign, q, t)
            chained += sum(1 for x in p if x >= 0)
    assert chained > 100


def test_look_back_only_restricts():
    rng = np.random.default_rng(4)
    for m in (1, 5, 30, 64):
        a = CC.anchors_of(CC.random_group(rng, m, 0, 1))
        for kw in (dict(CC.KEEP_ALL), dict(CC.KEEP_ALL, min_chain_score=0, max_chains=64)):
            got, unlimited = OC.chain_overlaps(a, **kw), OC.chain_overlaps(a, lookback=None, **kw)
            assert got[0].tobytes() == unlimited[0].tobytes() and got[1].tolist() == unlimited[1].tolist()
    # and beyond 64 anchors it does restrict: the 65-back predecessor of the look-back case is taken without the limit
    name, a, kw = CC.look_back_cases()[1]
    assert len(OC.chain_overlaps(a, lookback=None, **kw)[0]) == len(OC.chain_overlaps(a, **kw)[0]) + 1


def test_cost_values():
    # d k / 100 + (floor(log2 d) >> 1) at k = 15, by hand
    by_hand = {0: 0, 1: 0 + 0, 2: 0 + 0, 3: 0 + 0, 4: 0 + 1, 7: 1 + 1, 8: 1 + 1, 99: 14 + 3, 100: 15 + 3, 101: 15 + 3}
    for d, c in by_hand.items():
        assert OC.cost(d, 15) == c, d
    assert OC.gain(100, 180, 15) == 0 and OC.gain(100, 179, 15) == 1 and OC.gain(7, 7, 15) == 7


def test_look_back_edge():
    (_, a64, kw), (_, a65, _) = CC.look_back_cases()
    plus = lambda o: o[o["relative_strand"] == ord("+")]
    got = plus(OC.chain_overlaps(a64, **kw)[0])
    assert len(got) == 1 and int(got[0]["num_residues"]) == 2 and int(got[0]["query_start_position_in_read"]) == 100
    assert len(plus(OC.chain_overlaps(a65, **kw)[0])) == 0


def test_ties():
    cases = {name: (a, kw) for name, a, kw in CC.tie_cases()}
    o, s = OC.chain_overlaps(*cases["tie_equal_predecessors"][:1], **cases["tie_equal_predecessors"][1])
    assert len(o) == 1 and int(o[0]["target_start_position_in_read"]) == 160 and s.tolist() == [24]
    assert len(OC.chain_overlaps(cases["tie_best_equals_k"][0], **cases["tie_best_equals_k"][1])[0]) == 0
    o, s = OC.chain_overlaps(cases["tie_best_above_k"][0], **cases["tie_best_above_k"][1])
    assert len(o) == 1 and s.tolist() == [16]
    o, s = OC.chain_overlaps(cases["tie_equal_ends"][0], **cases["tie_equal_ends"][1])
    assert o["query_start_position_in_read"].tolist() == [100, 1000] and s.tolist() == [30, 30]
    o, s = OC.chain_overlaps(cases["tie_equal_ends_M1"][0], **cases["tie_equal_ends_M1"][1])
    assert o["query_start_position_in_read"].tolist() == [100]


def test_fork_is_cut_at_the_used_trunk():
    a = CC.fork_anchors()

    def run(s, m):  # the '+' records; in '-' every anchor of branch A chains with the one of branch B behind it
        o, scores = OC.chain_overlaps(a, **dict(CC.KEEP_ALL, min_chain_score=s, max_chains=m))
        plus = o["relative_strand"] == ord("+")
        return o[plus], scores[plus]

    o, s = run(20, 3)
    assert s.tolist() == [120, 27, 45] and o["num_residues"].tolist() == [8, 3, 3]
    assert o["query_start_position_in_read"].tolist() == [0, 550, 5000]
    assert run(40, 2)[1].tolist() == [120]  # the cut chain is dropped and its round is spent
    assert run(40, 3)[1].tolist() == [120, 45]
    assert run(27, 2)[1].tolist() == [120, 27] and run(28, 2)[1].tolist() == [120]
    assert run(0, 1)[1].tolist() == [120]


def test_minus_records():
    name, a, kw = CC.orientation_cases()[0]
    o, s = OC.chain_overlaps(a, **kw)
    assert len(o) == 1 and chr(o[0]["relative_strand"]) == "-" and s.tolist() == [15 * 12]
    assert (int(o[0]["query_start_position_in_read"]), int(o[0]["query_end_position_in_read"])) == (100, 650)
    assert (int(o[0]["target_start_position_in_read"]), int(o[0]["target_end_position_in_read"])) == (8450, 9000)
    name, a, kw = CC.orientation_cases()[2]
    o, s = OC.chain_overlaps(a, **kw)
    assert sorted(chr(x) for x in o["relative_strand"]) == ["+", "-"] and o["num_residues"].tolist() == [21, 21]


def test_interleaved_diagonals():
    a = CC.interleaved_diagonals()
    assert a["target_position_in_read"][:4].tolist() == [1000, 9000, 1200, 9200]  # they alternate
    o, s = OC.chain_overlaps(a, max_chains=2)
    assert s.tolist() == [90, 90] and o["num_residues"].tolist() == [6, 6]
    assert o["target_start_position_in_read"].tolist() == [1000, 9000]
    assert o["target_end_position_in_read"].tolist() == [2000, 10000]
    o, s = OC.chain_overlaps(a, max_chains=1)
    assert s.tolist() == [90] and o["target_start_position_in_read"].tolist() == [1000]
    # the triggered overlapper, by its oracle, finds neither
    assert len(O.overlaps(a, True)) == 0


def synthetic_anchors():
    reads, origin = CC.reads_with_origin(CC.SYNTHETIC_SEED)
    index = O.index(reads, 15, 10, True, 1.0)
    return reads, origin, O.anchors(index, index)


def found_pairs(overlaps):
    return {(int(o["query_read_id"]), int(o["target_read_id"])): chr(o["relative_strand"]) for o in overlaps}


def test_synthetic_mapping_finds_every_true_pair():
    reads, origin, a = synthetic_anchors()
    assert len(reads) == 40 and {r for _, _, r in origin} == {True, False}
    truth = CC.true_pairs(origin, 1000)
    assert len(truth) > 100
    o, s = OC.chain_overlaps(a)
    strands = {}
    for rec in o:
        strands.setdefault((int(rec["query_read_id"]), int(rec["target_read_id"])), set()).add(chr(rec["relative_strand"]))
    missing = [p for p, strand in truth.items() if strand not in strands.get(p, ())]
    assert not missing, missing
    triggered = found_pairs(O.overlaps(a, True))
    print("true pairs %d, chained finds %d, triggered finds %d" % (
        len(truth), len(truth) - len(missing), sum(1 for p, strand in truth.items() if triggered.get(p) == strand)))


def test_parameters_out_of_range():
    a = CC.interleaved_diagonals()
    for bad in (dict(max_gap=0), dict(bandwidth=-1), dict(max_chains=0), dict(max_chains=65), dict(kmer_size=33),
                dict(kmer_size=0), dict(min_chain_score=-1), dict(min_residues=-1)):
        try:
            OC.chain_overlaps(a, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    assert len(OC.chain_overlaps(a[:0])[0]) == 0


def test_library_surface():
    with open(os.path.join(ROOT, "include", "gw_mapper_capi.h")) as f:
        capi = f.read()
    with open(os.path.join(ROOT, "include", "gwhip_mapper.h")) as f:
        engine = f.read()
    for name in ("gw_mapper_chain_overlaps", "gw_mapper_chain_overlaps_host", "gw_mapper_map_batched_chained"):
        assert re.search(r"\b%s\(" % name, capi), name
    for name in ("gwm_chain_overlaps", "gwm_chain_overlaps_device"):
        assert re.search(r"\bint %s\(" % name, engine), name
    assert "typedef struct gwm_chaining" in engine
    from genomeworks_amd import build as B
    assert "mapper/gwm_chain.hip" in B.MAPPER_KERNEL_SRCS
    with open(os.path.join(ROOT, "genomeworks_amd", "lib", "libcudamapper.so"), "rb") as f:
        data = f.read()
    for sym in (b"gw_mapper_chain_overlaps\0", b"gw_mapper_chain_overlaps_host\0", b"gw_mapper_map_batched_chained\0",
                b"gwm_chain_overlaps\0", b"gwm_chain_overlaps_device\0"):
        assert sym in data, sym
