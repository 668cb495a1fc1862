"""The CPU oracle of the index batcher and of the cached driver's walk (tests/oracle_mapper_batcher.py) against the
expected batches of the reference's own batcher tests (tests/golden/cudamapper_batcher_vectors.json) and against the
pair order of the batched-driver oracle that the GPU tests already use."""
import json
import os
import sys
import types

import numpy as np
import pytest

import oracle_mapper_batcher as B
import oracle_mapper_postprocess as P

HERE = os.path.dirname(os.path.abspath(__file__))


def load_vectors():
    with open(os.path.join(HERE, "golden", "cudamapper_batcher_vectors.json")) as f:
        return json.load(f)


def as_lists(batches):
    return [[[list(d) for d in host[0]], [list(d) for d in host[1]],
             [[[list(d) for d in dq], [list(d) for d in dt]] for dq, dt in device]] for host, device in batches]


def oracle_arguments(case):
    same = case.get("same_query_and_target", True)
    return dict(query_lengths=case["query_lengths"], target_lengths=None if same else case["target_lengths"],
                Q=case["query_indices_per_host_batch"], q=case["query_indices_per_device_batch"],
                C=case["target_indices_per_host_batch"], c=case["target_indices_per_device_batch"],
                query_basepairs_per_index=case["query_basepairs_per_index"],
                target_basepairs_per_index=case["target_basepairs_per_index"])


def test_vector_tables():
    cases = load_vectors()["cases"]
    assert [c["name"] for c in cases] == ["query_and_target_not_the_same", "same_query_and_target"]
    for case in cases:
        got = B.generate_batches_of_indices(**oracle_arguments(case))
        assert len(got) == len(case["expected"]) >= 6, case["source"]
        assert as_lists(got) == case["expected"], case["source"]


def test_vector_exceptions():
    cases = load_vectors()["exceptions"]
    assert len(cases) == 4
    for case in cases:
        if not case["expressible"]:
            continue  # the same set with two parsers: the interface names the same set by leaving the target out
        with pytest.raises(ValueError):
            B.generate_batches_of_indices(**oracle_arguments(case))
    ok = dict(cases[0], target_indices_per_host_batch=cases[0]["query_indices_per_host_batch"])
    assert B.generate_batches_of_indices(**oracle_arguments(ok))


@pytest.mark.parametrize("counts", [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, -1, -1, -1),
                                    (2, 5, 2, 5), (2, 5, 10, 5), (10, 5, 1, 2)])
def test_counts_the_tool_level_refuses(counts):
    lengths = [5] * 12
    with pytest.raises(ValueError):
        B.generate_batches_of_indices(lengths, [5] * 7, *counts, query_basepairs_per_index=10)


def groupings():
    """(query indices, target indices or None) with 1 to 7 indices a side, a zero-read descriptor in front among them"""
    out = []
    for n in range(1, 8):
        lengths = [4, 6] * n                                  # n indices of two reads at 10 basepairs per index
        out.append((P.group_reads_into_indices(lengths, 10), None))
        for m in (1, 3, 7):
            out.append((P.group_reads_into_indices(lengths, 10), P.group_reads_into_indices([7, 3, 2] * m, 10)))
    first_too_long = P.group_reads_into_indices([12, 4, 6, 4, 6], 10)
    assert first_too_long[0] == (0, 0)
    out.append((first_too_long, None))
    out.append((first_too_long, first_too_long))
    return out


def pairs_map_batched_walks(monkeypatch, queries, targets, q_limit, t_limit):
    """the (query index, target index) pairs of oracle_mapper_postprocess.map_batched, in its order: its own loops run
    over stand-ins for the per-pair stages that only write down which indices they were given"""
    seen = []
    fake = types.ModuleType("oracle_mapper")
    fake.index = lambda reads, k, w, hashed, filtering, first_read_id=0: (first_read_id, len(reads))
    fake.anchors = lambda qi, ti: seen.append((qi, ti))
    fake.overlaps = lambda anchors, all_to_all, **kw: np.zeros(0, P.OVERLAP)
    monkeypatch.setitem(sys.modules, "oracle_mapper", fake)
    P.map_batched(queries, targets, 15, 10, 1.0, {}, q_limit, t_limit, post_process=False)
    return seen


@pytest.mark.parametrize("all_to_all", [True, False])
@pytest.mark.parametrize("n", range(1, 8))
def test_one_index_per_batch_is_the_order_of_map_batched(monkeypatch, n, all_to_all):
    queries = ["ACGT", "ACGTAC"] * n
    for targets, t_limit in ([(None, 10)] if all_to_all else [(["ACGTACG", "ACG", "AC"] * m, 10) for m in (1, 3, 7)] +
                             [(["ACGTACG"] * 5, 7)]):
        want = pairs_map_batched_walks(monkeypatch, queries, targets, 10, t_limit)
        assert len(want) >= (n * (n + 1) // 2 if all_to_all else n)
        pairs, builds, restores = B.walk_reads([len(r) for r in queries],
                                               None if targets is None else [len(r) for r in targets],
                                               1, 1, 1, 1, 10, t_limit)
        assert pairs == want
        assert restores == 0
        rows = n
        assert builds <= rows + sum(1 for a, b in want if all_to_all is False or a != b)


def test_pairs_of_map_batched_is_map_batched(monkeypatch):
    for queries, targets in groupings():
        all_to_all = targets is None
        assert B.walk(queries, queries if all_to_all else targets, all_to_all)[0] == \
            B.pairs_of_map_batched(queries, queries if all_to_all else targets, all_to_all)


@pytest.mark.parametrize("counts", [(1, 1, 1, 1), (2, 1, 2, 1), (3, 2, 3, 2), (4, 4, 4, 4), (10, 5, 10, 5),
                                    (2, 1, 3, 2), (7, 2, 2, 1)])
def test_every_setting_walks_the_same_pairs(counts):
    for queries, targets in groupings():
        all_to_all = targets is None
        if all_to_all and (counts[0] != counts[2] or counts[1] != counts[3]):
            continue
        t = queries if all_to_all else targets
        pairs, builds, restores = B.walk(queries, t, all_to_all, *counts)
        base = B.walk(queries, t, all_to_all)[0]
        assert sorted(pairs) == sorted(base) and len(set(pairs)) == len(pairs)
        non_empty = len([d for d in queries if d[1]]) + (0 if all_to_all else len([d for d in t if d[1]]))
        assert builds >= non_empty
        if counts[0] >= len(queries) and counts[2] >= len(t):
            # one host batch: every index is built once and never again
            assert builds == non_empty
        if counts[1] >= len(queries) and counts[3] >= len(t):
            assert restores == 0  # one device batch: nothing goes to the host


def test_walk_counts_by_hand():
    # four indices all against all, two per host batch, one per device batch
    idx = [(0, 2), (2, 2), (4, 2), (6, 2)]
    pairs, builds, restores = B.walk(idx, idx, True, 2, 1, 2, 1)
    # host batches {0,1}x{0,1}: builds 0, 1; device batches (0;0) (0;1) (1;1): 1 restored once
    # {0,1}x{2,3}: 1 is on the device, 0 comes from its host copy; builds 2, 3; (0;2) (0;3) (1;2) (1;3): 3, then 1
    # and 2, then 3 restored
    # {2,3}x{2,3}: 3 is on the device, 2 comes from its host copy; (2;2) (2;3) (3;3): 3 restored
    assert pairs == [(idx[0], idx[0]), (idx[0], idx[1]), (idx[1], idx[1]), (idx[0], idx[2]), (idx[0], idx[3]),
                     (idx[1], idx[2]), (idx[1], idx[3]), (idx[2], idx[2]), (idx[2], idx[3]), (idx[3], idx[3])]
    assert (builds, restores) == (4, 1 + 1 + 4 + 1 + 1)
    # one index at a time: the query index of a row stays, every other index of a pair is built unless the pair before
    # left it on the device (the last row finds its only index there)
    pairs, builds, restores = B.walk(idx, idx, True)
    assert (builds, restores) == (4 + 3 + 2 + 0, 0) and len(pairs) == 10
    pairs, builds, restores = B.walk(idx[:2], idx, False)
    assert (builds, restores) == (2 + 8, 0) and len(pairs) == 8


def test_walk_counts_by_hand_query_vs_target_with_other_target_counts():
    """two query indices against four target indices at Q 2, q 1, C 3, c 2, counted on paper from the rules of
    gw_mapper_map_batched_cached, not from the oracle"""
    a, b = (0, 2), (2, 2)
    x, y, z, u = (0, 3), (3, 3), (6, 3), (9, 3)
    pairs, builds, restores = B.walk([a, b], [x, y, z, u], False, 2, 1, 3, 2)
    # host batch {a,b} x {x,y,z}, device batches (a;x,y) (a;z) (b;x,y) (b;z): all five are built, and all five get a
    # host copy because a later device batch asks for each; a, x, y stay on the device.
    #   (a;z): z restored. (b;x,y): b, x and y restored (x and y left the device with (a;z)). (b;z): z restored.  -> 5
    # host batch {a,b} x {u}, device batches (a;u) (b;u): b is still on the device, a comes from its host copy because
    # the first device batch needs it (6), u is built and packed; (b;u) asks for b, which is not part of the device
    # batch being mapped, so it is restored (7).
    assert pairs == [(a, x), (a, y), (a, z), (b, x), (b, y), (b, z), (a, u), (b, u)]
    assert (builds, restores) == (6, 7)
    # the same sets with everything in one host batch and one device batch: each index once, nothing restored
    assert B.walk([a, b], [x, y, z, u], False, 2, 2, 4, 4)[1:] == (6, 0)
    # one device batch per host batch, two host batches: nothing is packed, so the second host batch finds its
    # queries on the device and builds only its targets
    pairs, builds, restores = B.walk([a, b], [x, y, z, u], False, 2, 2, 2, 2)
    assert (builds, restores) == (2 + 2 + 2, 0) and len(pairs) == 8


def test_walk_reuses_the_host_copies_of_the_previous_host_batch_only():
    """three host batches in a row of queries {a,b} at Q 2, q 1, C 1, c 1: the queries' host copies made in the first
    host batch serve the second and the third, because every host batch hands the copies it still needs on"""
    a, b = (0, 2), (2, 2)
    x, y, z = (0, 3), (3, 3), (6, 3)
    pairs, builds, restores = B.walk([a, b], [x, y, z], False, 2, 1, 1, 1)
    # {a,b} x {x}: (a;x) (b;x): a, b, x built; b and x packed (a later device batch asks for them), a is not.
    #   (b;x): b restored, x shared.                                                          builds 3, restores 1
    # {a,b} x {y}: b is on the device; a has no host copy and is not on the device: built again. y built. b, y packed
    #   (b already has its copy). (b;y): b restored (it was not part of (a;y)).                builds 5, restores 2
    # {a,b} x {z}: the same once more.                                                        builds 7, restores 3
    assert pairs == [(a, x), (b, x), (a, y), (b, y), (a, z), (b, z)]
    assert (builds, restores) == (7, 3)
