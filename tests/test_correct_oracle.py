"""Read correction without a GPU: the two formulations of the query-role records agree on
an all-against-all mapping, the pair selection (C1) and the layer selection over both roles (C3, C4) against answers
worked out on paper -- the Python oracle, the C API of libcudamapper.so and a stand-alone caller of the host source under
the address and undefined-behaviour sanitizers --, the public surface, and the oracle pipeline's effect on reads whose
error-free versions are known."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_correct as OC
import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_polish as OPo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
WINDOW_LENGTHS = (7, 64, 200)


def ov(q, t, qs, qe, ts, te, strand="+"):
    return (q, t, qs, ts, qe, te, ord(strand), 0, 0)


def overlaps_of(rows):
    return np.array(rows, O.OVERLAP).reshape(-1)


def segments_of(rows):
    return np.array(rows, OC.SEGMENT).reshape(-1)


# C1. name -> (overlaps, the positions kept)
PAIRS = {
    "self_only": ([ov(0, 0, 0, 500, 0, 500), ov(1, 1, 0, 300, 0, 300)], []),
    "longer_direction_second": ([ov(0, 1, 0, 100, 50, 150), ov(1, 0, 40, 150, 0, 110, "-")], [1]),
    "tie_keeps_the_first": ([ov(2, 1, 0, 100, 0, 100), ov(1, 2, 50, 150, 50, 150)], [0]),
    "two_records_of_one_direction": ([ov(0, 1, 0, 100, 0, 100), ov(0, 1, 100, 300, 100, 300)], [1]),
    # three pairs among self overlaps, ids from 7: kept records come in input order
    "input_order": ([ov(7, 7, 0, 900, 0, 900), ov(9, 8, 0, 100, 0, 100), ov(7, 9, 0, 50, 0, 50), ov(8, 7, 0, 80, 0, 80),
                     ov(8, 9, 0, 100, 0, 100), ov(9, 7, 0, 60, 0, 60), ov(9, 9, 0, 10, 0, 10)], [1, 3, 5]),
    "none": ([], []),
}

# C3 / C4, the target role. name -> (pairs, target-role records (pair, window, target_first, target_last, query_begin,
# query_end), read lengths, W, max_depth, first read id, {(owner, window): [layer (read, begin, end, reversed), ...]}).
# Windows that are not named hold their backbone alone. mirrored() turns a case into its query-role twin.
LAYERS = {
    # W = 200: W / 100 = 2 bases of slack at the head and at the tail, 3 are one too many
    "slack": (
        [ov(1, 0, 0, 198, 2, 200), ov(2, 0, 0, 197, 3, 200), ov(3, 0, 0, 198, 0, 198), ov(4, 0, 0, 197, 0, 197),
         ov(5, 0, 0, 197, 202, 399), ov(6, 0, 0, 196, 203, 399)],
        [(0, 0, 2, 199, 0, 198), (1, 0, 3, 199, 0, 197), (2, 0, 0, 197, 0, 198), (3, 0, 0, 196, 0, 197),
         (4, 1, 202, 398, 0, 197), (5, 1, 203, 398, 0, 196)],
        [401, 198, 198, 198, 198, 198, 198], 200, 30, 0,
        {(0, 0): [(3, 0, 198, 0), (1, 0, 198, 0)], (0, 1): [(5, 0, 197, 0)]}),
    # W = 10: no slack; 20 bases of the other read are a layer, 21 and none are not
    "length_bound": (
        [ov(1, 0, 0, 20, 0, 10), ov(2, 0, 0, 21, 0, 10), ov(3, 0, 5, 5, 0, 10), ov(4, 0, 7, 8, 0, 10)],
        [(0, 0, 0, 9, 0, 20), (1, 0, 0, 9, 0, 21), (2, 0, 0, 9, 5, 5), (3, 0, 0, 9, 7, 8)],
        [10, 21, 21, 8, 8], 10, 30, 0,
        {(0, 0): [(1, 0, 20, 0), (4, 7, 8, 0)]}),
    # four layers, room for three: by (target_first, pair position); the '-' one is marked reversed
    "depth_cap_order": (
        [ov(1, 0, 0, 99, 1, 100), ov(2, 0, 0, 100, 0, 100, "-"), ov(3, 0, 0, 99, 1, 100), ov(4, 0, 0, 100, 0, 100)],
        [(0, 0, 1, 99, 0, 99), (1, 0, 0, 99, 0, 100), (2, 0, 1, 99, 0, 99), (3, 0, 0, 99, 0, 100)],
        [100, 100, 100, 100, 100], 100, 3, 0,
        {(0, 0): [(2, 0, 100, 1), (4, 0, 100, 0), (1, 0, 99, 0)]}),
    # an owner of 250 bases: its window 2 ends at 250, and the slack counts from there
    "last_window_shorter": (
        [ov(1, 0, 0, 50, 200, 250), ov(2, 0, 0, 49, 200, 249), ov(3, 0, 0, 48, 200, 248)],
        [(0, 2, 200, 249, 0, 50), (1, 2, 200, 248, 0, 49), (2, 2, 200, 247, 0, 48)],
        [250, 50, 50, 50], 100, 30, 0,
        {(0, 2): [(1, 0, 50, 0), (2, 0, 49, 0)]}),
    # read ids count from 5; a read of no bases has no window
    "first_read_id": (
        [ov(6, 5, 3, 43, 0, 40), ov(8, 7, 0, 100, 0, 100, "-")],
        [(0, 0, 0, 39, 3, 43), (1, 0, 0, 99, 0, 100)],
        [40, 50, 100, 100, 0], 100, 30, 5,
        {(0, 0): [(1, 3, 43, 0)], (2, 0): [(3, 0, 100, 1)]}),
}


def mirrored(case):
    """the query-role twin: query and target change places in every pair, the records are query-role records"""
    pairs, records, lengths, W, depth, first, layers = case
    swapped = [(t, q, ts, qs, te, qe, strand, 0, 0) for q, t, qs, ts, qe, te, strand, _, _ in pairs]
    return swapped, records, lengths, W, depth, first, layers


def expected(lengths, W, layers):
    """(plan, windows) from the layers of the named windows: C4's backbones and table by arithmetic"""
    plan, table = [], []
    for r, length in enumerate(lengths):
        for k in range((length + W - 1) // W):
            first = len(plan)
            plan.append((0, r, k * W, min((k + 1) * W, length), 0))
            plan += [(0,) + layer for layer in layers.get((r, k), [])]
            table.append((r, k, first, len(plan) - first))
    return plan, table


def layer_cases():
    """name -> (pairs, target-role records, query-role records, lengths, W, depth, first id, expected (plan, windows))"""
    out = {}
    for name, case in LAYERS.items():
        for role, (pairs, records, lengths, W, depth, first, layers) in (("target", case), ("query", mirrored(case))):
            both = (records, []) if role == "target" else ([], records)
            out["%s_%s_role" % (name, role)] = (pairs,) + both + (lengths, W, depth, first, expected(lengths, W, layers))
    # one pair gives a layer to both of its reads; a window's layers of the two roles are ordered together: read 0's
    # window 0 gets the query-role layer of pair 1 (target_first 0) before the target-role layer of pair 0 (1)
    out["both_roles"] = (
        [ov(1, 0, 0, 99, 1, 100), ov(0, 2, 0, 100, 0, 100, "-")],
        [(0, 0, 1, 99, 0, 99), (1, 0, 0, 99, 0, 100)], [(0, 0, 0, 98, 1, 100), (1, 0, 0, 99, 0, 100)],
        [100, 99, 100], 100, 30, 0,
        expected([100, 99, 100], 100, {(0, 0): [(2, 0, 100, 1), (1, 0, 99, 0)], (1, 0): [(0, 1, 100, 0)],
                                       (2, 0): [(0, 0, 100, 1)]}))
    return out


LAYER_CASES = layer_cases()


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import build, cudamapper
    build.build_mapper()
    return cudamapper


@pytest.fixture(scope="module")
def small():
    """the small case mapped against itself as two sets: reads, all records, the pairs and their alignments"""
    reads, _ = OPo.small_case()
    o = OC.mapped_all_against_all(reads)
    same = o["query_read_id"] == o["target_read_id"]
    directions = {(int(a), int(b)) for a, b in zip(o["query_read_id"], o["target_read_id"])}
    assert same.sum() == len(reads) and any((b, a) in directions for a, b in directions if a < b)
    pairs = o[OC.select_pairs(o)]
    assert len(pairs) >= 100 and {chr(s) for s in pairs["relative_strand"]} == {"+", "-"}
    return reads, o, pairs, OA.alignments(pairs, reads)


@pytest.mark.parametrize("W", WINDOW_LENGTHS)
def test_two_query_role_formulations_agree(small, W):
    reads, _, pairs, alignments = small
    by_states = OC.pair_segments(pairs, reads, W, alignments)
    by_cigar = OC.pair_segments(pairs, reads, W, alignments, "cigar")
    for a, b in zip(by_states[0] + by_states[1], by_cigar[0] + by_cigar[1]):
        assert np.array_equal(a, b)
    s, offsets = by_states[1]
    assert len(s) >= len(pairs) and offsets[-1] == len(s)
    assert np.all(s["target_first"] // W == s["window"]) and np.all(s["target_last"] // W == s["window"])
    # the windows are the query's and the ranges the target's: both lie within the pair's slices
    of = pairs[s["overlap"]]
    assert np.all(s["target_first"] >= of["query_start_position_in_read"])
    assert np.all(s["target_last"] < of["query_end_position_in_read"])
    assert np.all(s["query_begin"] >= of["target_start_position_in_read"])
    assert np.all(s["query_end"] <= of["target_end_position_in_read"])


def test_pairs_of_the_small_case(small):
    reads, o, pairs, _ = small
    seen = set()
    for p in pairs:
        a, b = int(p["query_read_id"]), int(p["target_read_id"])
        assert a != b and (min(a, b), max(a, b)) not in seen
        seen.add((min(a, b), max(a, b)))
    assert seen == {(min(int(a), int(b)), max(int(a), int(b)))
                    for a, b in zip(o["query_read_id"], o["target_read_id"]) if a != b}
    assert len(pairs) < (o["query_read_id"] != o["target_read_id"]).sum()  # fewer records are aligned than came in


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_oracle_pairs_on_hand_cases(name):
    rows, kept = PAIRS[name]
    assert OC.select_pairs(overlaps_of(rows)) == kept


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_c_api_pairs_on_hand_cases(cm, name):
    rows, kept = PAIRS[name]
    got = cm.select_pairs(overlaps_of(rows))
    assert got.dtype == np.int64 and got.tolist() == kept


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_oracle_layers_on_hand_cases(name):
    pairs, t, q, lengths, W, depth, first, want = LAYER_CASES[name]
    assert OC.select_correction_layers(segments_of(t), segments_of(q), overlaps_of(pairs), lengths, W, depth, first) == want


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_c_api_layers_on_hand_cases(cm, name):
    pairs, t, q, lengths, W, depth, first, want = LAYER_CASES[name]
    assert cm.select_correction_layers(segments_of(t), segments_of(q), overlaps_of(pairs), lengths, W, depth, first) == want


def test_a_reverse_query_role_layer_and_its_bases():
    """Q = rc(T[10:90]) aligned to T[10:90] on '-': window 2 of Q (W = 16) is covered by T[42:58], and the layer is that
    slice reversed through the aligner's table -- which is Q[32:48] again, since Q is an exact copy"""
    rng = np.random.default_rng(5)
    T = "".join(rng.choice(list("ACGT"), 100))
    Q = T[10:90].translate(str.maketrans("ACGT", "TGCA"))[::-1]
    pairs = overlaps_of([ov(1, 0, 0, 80, 10, 90, "-")])
    query_role = segments_of([(0, 2, 32, 47, 42, 58)])
    assert OC.query_role_from_states(0, pairs[0], [0] * 80, 16)[2] == tuple(query_role[0].tolist())
    plan, table = OC.select_correction_layers(segments_of([]), query_role, pairs, [100, 80], 16, 30)
    assert table[7 + 2] == (1, 2, 7 + 2, 2) and plan[7 + 2:7 + 4] == [(0, 1, 32, 48, 0), (0, 0, 42, 58, 1)]
    backbone, layer = OC.cut(plan, [T, Q])[7 + 2:7 + 4]
    assert layer == backbone == Q[32:48].encode() and layer != T[42:58].encode()


@pytest.mark.parametrize("W", WINDOW_LENGTHS)
@pytest.mark.parametrize("depth", [0, 3, 30])
def test_c_api_host_functions_equal_the_oracle(cm, small, W, depth):
    reads, o, pairs, alignments = small
    assert cm.select_pairs(o).tolist() == OC.select_pairs(o)
    (t, _, _), (q, _) = OC.pair_segments(pairs, reads, W, alignments)
    lengths = [len(r) for r in reads]
    want = OC.select_correction_layers(t, q, pairs, lengths, W, depth)
    assert cm.select_correction_layers(t, q, pairs, lengths, W, depth) == want
    assert len(want[1]) == sum((n + W - 1) // W for n in lengths) and all(p[0] == 0 for p in want[0])
    assert depth == 0 or len(want[0]) > len(want[1])


def test_c_api_refusals(cm):
    pairs, t, q, lengths, W, depth, first, _ = LAYER_CASES["both_roles"]
    pairs, t, q = overlaps_of(pairs), segments_of(t), segments_of(q)
    for kw in (dict(window_length=0), dict(max_depth=-1)):
        with pytest.raises(cm.MapperError):
            cm.select_correction_layers(t, q, pairs, lengths, **dict(dict(window_length=W, max_depth=depth), **kw))
    for role in (0, 1):
        for field, value in (("overlap", 2), ("window", 1), ("target_last", 100)):
            bad = [t.copy(), q.copy()]
            bad[role][1][field] = value
            with pytest.raises(cm.MapperError):
                cm.select_correction_layers(bad[0], bad[1], pairs, lengths, W, depth)
    with pytest.raises(cm.MapperError):  # a read id outside the set
        cm.select_correction_layers(t, q, pairs, lengths[:2], W, depth)
    with pytest.raises(cm.MapperError):  # a record that starts behind its end
        cm.select_pairs(overlaps_of([ov(0, 1, 10, 5, 0, 5)]))
    assert cm.select_correction_layers(t[:0], q[:0], pairs[:0], [], W, depth) == ([], [])


def test_rules_under_the_sanitizers(tmp_path):
    """the host source and a stand-alone caller, built with -fsanitize=address,undefined, on the hand cases"""
    exe = str(tmp_path / "select_correction_sanitized")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "select_correction_sanitized.cpp"),
           os.path.join(ROOT, "genomeworks_amd", "mapper", "gwm_windows.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text, want = [], []
    for name in sorted(PAIRS):
        rows, kept = PAIRS[name]
        text.append("pairs %d" % len(rows))
        text += ["%d %d %d %d %d %d %c" % row[:7] for row in rows]
        want += ["pairs %d" % len(kept)] + [str(i) for i in kept]
    for name in sorted(LAYER_CASES):
        pairs, t, q, lengths, W, depth, first, (plan, table) = LAYER_CASES[name]
        text.append("layers %d %d %d %d %d %d %d" % (W, depth, len(lengths), first, len(pairs), len(t), len(q)))
        text.append(" ".join(str(x) for x in lengths))
        text += ["%d %d %d %d %d %d %c" % row[:7] for row in pairs]
        text += ["%d %d %d %d %d %d" % row for row in t + q]
        want.append("layers %d %d" % (len(plan), len(table)))
        want += ["p %d %d %d %d %d" % p for p in plan] + ["w %d %d %d %d" % w for w in table]
    # what the rules refuse: a record that starts behind its end, a window length of 0, a record of a pair that does
    # not exist
    text += ["pairs 1", "0 1 10 0 5 5 +", "layers 0 3 1 0 0 0 0", "10", "layers 10 3 1 0 0 0 1", "10", "0 0 0 9 0 10"]
    want += ["error", "error", "error"]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.splitlines() == want


def test_new_c_symbols_are_exported_and_a_caller_compiles(cm, tmp_path):
    C.CDLL(os.path.join(LIB, "libgwhip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIB, "libcudamapper.so"))
    for name in ("gwm_pair_segments", "gw_mapper_select_pairs", "gw_mapper_select_correction_layers",
                 "gw_mapper_correction_windows", "gw_mapper_pair_segments", "gw_mapper_windows_copy_query_role_segments"):
        assert hasattr(lib, name), name
    for name in ("select_pairs", "pair_segments", "select_correction_layers", "correction_windows"):
        assert callable(getattr(cm, name)), name
    src = tmp_path / "caller.c"
    src.write_text("""
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"
#include <stdio.h>
int main(void)
{
    gwm_segment t = {0, 0, 0, 9, 0, 10}, q = {0, 0, 0, 9, 0, 10};
    gwm_overlap o[3] = {{0, 0, 0, 0, 10, 10, '+', 0, 0}, {0, 1, 0, 0, 10, 10, '+', 0, 0}, {1, 0, 0, 0, 10, 10, '+', 0, 0}};
    int64_t lengths[2] = {10, 10}, n_windows = 0, positions[3] = {-1, -1, -1};
    uint32_t plan[20], table[8];
    int (*segments)(const gwm_overlap*, int64_t, const char*, const int64_t*, int32_t, uint32_t, int32_t, int64_t, void*,
                    gwm_segments*, gwm_segments*) = gwm_pair_segments;
    gw_mapper_windows* (*entry)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, int32_t, int32_t,
                                int64_t, void*) = gw_mapper_correction_windows;
    int64_t pairs = gw_mapper_select_pairs(o, 3, positions, 3);
    int64_t n = gw_mapper_select_correction_layers(&t, 1, &q, 1, o + 1, 1, lengths, 2, 0, 10, 30, plan, 4, &n_windows,
                                                   table, 2);
    if (!segments || !entry || pairs != 1 || positions[0] != 1 || n != 4 || n_windows != 2 || plan[5] != 0 ||
        plan[6] != 1 || plan[11] != 1 || plan[16] != 0 || table[3] != 2 || table[7] != 2)
        return 1;
    puts("ok");
    return 0;
}
""")
    exe = str(tmp_path / "caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", LIB,
                        "-lcudamapper", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + LIB,
                        "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) == (0, "ok"), r.stderr


def test_correct_reads_refusals_need_no_device():
    from genomeworks_amd import polisher
    reads, _ = OPo.small_case()
    with pytest.raises(ValueError):
        polisher.correct_reads(reads, window_length=0)
    with pytest.raises(ValueError):
        polisher.correct_reads(reads, max_depth=-1)
    with pytest.raises(ValueError):
        polisher.correct_reads(reads + ["ACGT"])
    with pytest.raises(ValueError):
        polisher.correct_reads(reads, align=True)
    with pytest.raises(TypeError):
        polisher.correct_reads(reads, overlaps=np.zeros(0, O.OVERLAP), k=15)


# (seed, window length) for which the oracle pipeline alone lowers the summed edit distance to the true reads: 24 reads
# of about 600 bases from a 1500-base genome, 5 % errors
IMPROVING = [(1, 150), (2, 200), (3, 300), (4, 150), (5, 200)]


@pytest.mark.parametrize("seed,W", IMPROVING)
def test_oracle_pipeline_lowers_the_distance_to_the_true_reads(seed, W):
    reads, truth = OC.reads_with_truth(seed, 1500, 24, 600, 0.05)
    o = OC.mapped_all_against_all(reads)
    corrected, report = OC.correct(reads, o, W, 15, 64)
    before, after = OC.summed_edit_distance(reads, truth), OC.summed_edit_distance(corrected, truth)
    print("seed %d W %d: %d records, %d pairs, reads %d, corrected %d" % (seed, W, len(o), len(OC.select_pairs(o)),
                                                                        before, after))
    assert after < before
    assert [r[:2] for r in report] == [(i, k) for i, r in enumerate(reads) for k in range((len(r) + W - 1) // W)]
    assert sum(1 for r in report if r[3] == 0 and not r[4]) >= len(reads)
    # polishing's rule 1 would keep every read's overlap with itself: the reads come back as they are
    if seed == 1:
        same = o[o["query_read_id"] == o["target_read_id"]]
        assert len(same) == len(reads)
        assert OPo.polish(reads, reads, o, W, 15, 64)[0] == reads
