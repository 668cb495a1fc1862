"""Anchored overlap alignment without a GPU: rules G1-G6 of the oracle on hand-made anchor
lists, the 16 chained records of the synthetic reads, the capacity case, the shared plan header under the sanitizers,
the exported symbols and a C99 caller, and the refusals that need no device."""
import os
import subprocess

import numpy as np
import pytest

import mapper_anchored_cases as GC
import oracle_affine as OA
import oracle_affine2 as OA2
import oracle_mapper_align as OM
import oracle_mapper_anchored as OG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
K = GC.K


def plus(n=400, m=410):
    return GC.record(0, 0, 100, 100 + n, 120, 120 + m, "+")


def minus(n=380, m=372):
    return GC.record(1, 1, 90, 90 + n, 184, 184 + m, "-")


def test_slice_coordinates():
    assert OG.coordinates(plus(), 100, 120, K) == (0, 0)
    assert OG.coordinates(plus(), 250, 300, K) == (150, 180)
    # '-': the start of the k-mer in the reverse-complemented slice; a k-mer at the slice's end starts at v = 0
    o = minus()
    assert OG.coordinates(o, 90, 556, K) == (0, -K)
    assert OG.coordinates(o, 91, 556 - K, K) == (1, 0)
    assert OG.coordinates(o, 92, 556 - K - 1, K) == (2, 1)
    assert OG.coordinates(o, 92, 184, K) == (2, 372 - K)
    # nothing wraps at the ends of uint32
    far = GC.record(0, 0, 2 ** 32 - 10, 2 ** 32 - 1, 0, 9, "-")
    assert OG.coordinates(far, 2 ** 32 - 5, 2 ** 32 - 1, 32) == (5, 9 - (2 ** 32 - 1) - 32)


def test_only_anchors_strictly_inside_count():
    o = plus()
    n, m = OG.lengths(o)
    inside = (101, 121)
    for q, t, valid in ((100, 125, False), (101, 120, False), inside + (True,), (100 + n - 1, 120 + m - 1, True),
                        (100 + n, 120 + m - 1, False), (100 + n - 1, 120 + m, False), (99, 119, False)):
        assert OG.cuts(o, [(q, t)], K, 256) == ([OG.coordinates(o, q, t, K)] if valid else []), (q, t)
    o = minus()
    for t, valid in ((556, False), (556 - K, False), (556 - K - 1, True), (556 - K - 371, True), (556 - K - 372, False)):
        assert (OG.cuts(o, [(95, t)], K, 256) != []) == valid, t


def test_cuts_are_head_flags_of_the_spacing_cells():
    o = plus()
    at = lambda u, v: (100 + u, 120 + v)
    anchors = [at(63, 60), at(64, 66), at(65, 67), at(127, 130), at(128, 131)]
    assert OG.cuts(o, anchors, K, 64) == [(63, 60), (64, 66), (128, 131)]
    assert OG.cuts(o, anchors, K, 1) == [(63, 60), (64, 66), (65, 67), (127, 130), (128, 131)]
    assert OG.cuts(o, anchors, K, 256) == [(63, 60)]
    assert OG.cuts(o, anchors, K, 63) == [(63, 60), (127, 130)]  # cells 1, 1, 1, 2, 2
    assert OG.pieces(o, anchors, K, 64) == [(0, 0, 63, 60), (63, 60, 1, 6), (64, 66, 64, 65), (128, 131, 272, 279)]
    # an invalid anchor between two valid ones is not "the anchor before"
    assert OG.cuts(o, [at(10, 10), (105, 5000), at(20, 21), at(300, 310)], K, 256) == [(10, 10), (300, 310)]


def test_records_without_valid_anchors_are_one_piece():
    assert OG.pieces(plus(), [], K, 256) == [(0, 0, 400, 410)]
    assert OG.pieces(plus(), [(100, 120), (500, 530)], K, 256) == [(0, 0, 400, 410)]  # a chain's own ends
    assert OG.pieces(plus(0, 20), [(100, 125), (101, 126)], K, 256) == [(0, 0, 0, 20)]
    assert OG.pieces(plus(30, 0), [(110, 120)], K, 256) == [(0, 0, 30, 0)]
    assert OG.pieces(plus(0, 0), [], K, 1) == [(0, 0, 0, 0)]


def test_a_list_that_is_not_monotone_is_refused_with_its_record():
    queries, targets, overlaps, anchors = GC.not_monotone()
    offsets, positions = GC.lists(anchors)
    with pytest.raises(OG.NotMonotone, match="overlap 2 ") as e:
        OG.plan(overlaps, offsets, positions, K, 64)
    assert e.value.record == 2
    # equal in one coordinate is not increasing; on '-' the target runs backwards
    assert OG.cuts(plus(), [(110, 130), (110, 131)], K, 256) is None
    assert OG.cuts(plus(), [(110, 130), (111, 130)], K, 256) is None
    assert OG.cuts(minus(), [(100, 500), (110, 505)], K, 256) is None
    assert OG.cuts(minus(), [(100, 500), (110, 495)], K, 256) == [(10, 41)]
    for k, S in ((0, 256), (33, 256), (15, 0)):
        with pytest.raises(ValueError):
            OG.plan(overlaps[:1], [0, 0], np.zeros((0, 2), np.uint32), k, S)
    for bad in ([1, 1], [0, 2], [0, 1, 0], [0]):
        with pytest.raises(ValueError):
            OG.plan(overlaps[:len(bad) - 1], bad, np.zeros((1, 2), np.uint32), K, 256)


@pytest.mark.parametrize("S", (1, 64, 256))
def test_hand_made_lists_tile_their_slices(S):
    queries, targets, overlaps, anchors, what = GC.hand_made()
    offsets, positions = GC.lists(anchors)
    plans = OG.plan(overlaps, offsets, positions, K, S)
    for o, record, name in zip(overlaps, plans, what):
        n, m = OG.lengths(o)
        assert record[0][:2] == (0, 0) and (record[-1][0] + record[-1][2], record[-1][1] + record[-1][3]) == (n, m), name
        for (u, v, dn, dm), (u2, v2, _, _) in zip(record[:-1], record[1:]):
            assert (u + dn, v + dm) == (u2, v2) and dn > 0 and dm > 0, name
    by_name = dict(zip(what, plans))
    assert len(by_name["corners"]) == (3 if S == 256 else 4)  # u = 1, 200, 399: cells 0, 0, 1 of 256; 0, 3, 6 of 64
    assert len(by_name["no anchors"]) == len(by_name["n = 0"]) == len(by_name["m = 0"]) == len(by_name["both empty"]) == 1
    assert len(by_name["long"]) > (128 if S == 1 else 2)


@pytest.fixture(scope="module")
def sixteen():
    reads, overlaps, offsets, positions = GC.sixteen_records()
    assert len(overlaps) == 16 and {chr(s) for s in overlaps["relative_strand"]} == {"+", "-"}
    assert [int(b - a) for a, b in zip(offsets[:-1], offsets[1:])] == overlaps["num_residues"].tolist()
    return reads, overlaps, offsets, positions


def test_sixteen_records_replay_and_cost_what_the_whole_slice_costs(sixteen):
    reads, overlaps, offsets, positions = sixteen
    x, o, e = 4, 6, 2
    got = OG.alignments(overlaps, reads, None, offsets, positions, K, 256, (x, o, e, 16))
    pieces = widest = 0
    for rec, r in zip(overlaps, got):
        q, t = (s.decode() for s in OM.slices(rec, reads, reads))
        assert r["states"] is not None
        OA.replay(r["states"], q, t)
        piece_costs = [OA.cost_of(p, x, o, e) for p in r["piece_states"]]
        assert OA.cost_of(r["states"], x, o, e) == sum(piece_costs)
        assert sum(piece_costs) == OA.align(q, t, x, o, e, 128)["cost"]
        pieces += len(r["pieces"])
        widest = max([widest] + [abs(dn - dm) for _, _, dn, dm in r["pieces"]])
    assert pieces == 106 and widest == 23
    assert sum(len(p) for p in OG.plan(overlaps, offsets, positions, K, 64)) == 173
    # a chained record starts and ends on an anchor: 38 anchors are dropped at record ends
    valid = sum(1 for rec, a, b in zip(overlaps, offsets[:-1], offsets[1:]) for q, t in positions[a:b]
                if (lambda uv: 0 < uv[0] < OG.lengths(rec)[0] and 0 < uv[1] < OG.lengths(rec)[1])(OG.coordinates(rec, q, t, K)))
    assert len(positions) - valid == 38


def gap_runs(states):
    runs, before = [], None
    for s in states:
        if s in (2, 3) and s == before:
            runs[-1][1] += 1
        elif s in (2, 3):
            runs.append([s, 1])
        before = s
    return [tuple(r) for r in runs]


def test_capacity_case_one_piece():
    query, target, rec, rows = GC.capacity_case(5)
    assert len(target) == 5000 and len(query) == 5000 - 5 * 450
    assert OA.band(len(query), len(target), 16)[2] == 2283
    assert OA.align(query, target, 4, 6, 2, 16)["states"] is None
    offsets, positions = GC.lists([rows])
    r = OG.alignments(np.array([rec]), [query], [target], offsets, positions, K, 256, (4, 6, 2, 16))[0]
    OA.replay(r["states"], query, target)
    assert gap_runs(r["states"]) == [(2, 450)] * 5
    assert OA.cost_of(r["states"], 4, 6, 2) == 5 * (6 + 2 * 450)


@pytest.mark.parametrize("deletions,whole", ((2, True), (3, False)))
def test_capacity_case_two_pieces(deletions, whole):
    query, target, rec, rows = GC.capacity_case(deletions)
    scoring = OA2.DEFAULT + (16,)
    assert OA.band(len(query), len(target), 16)[2] == 450 * deletions + 33
    assert (OA2.align(query, target, *scoring)["states"] is not None) == whole
    offsets, positions = GC.lists([rows])
    r = OG.alignments(np.array([rec]), [query], [target], offsets, positions, K, 256, scoring)[0]
    OA.replay(r["states"], query, target)
    assert gap_runs(r["states"]) == [(2, 450)] * deletions


def _plan_cases():
    """R lines for the stand-alone program: every hand-made record at S = 1, 64, 256, the broken lists, the 16
    records, the capacity case, and positions at the ends of uint32"""
    out = []
    for S in (1, 63, 64, 256):
        _, _, overlaps, anchors, _ = GC.hand_made()
        out += [(o, a, K, S) for o, a in zip(overlaps, anchors)]
        _, _, overlaps, anchors = GC.not_monotone()
        out += [(o, a, K, S) for o, a in zip(overlaps, anchors)]
    _, overlaps, offsets, positions = GC.sixteen_records()
    for S in (64, 256):
        out += [(o, [tuple(int(v) for v in r) for r in positions[a:b]], K, S)
                for o, a, b in zip(overlaps, offsets[:-1], offsets[1:])]
    _, _, rec, rows = GC.capacity_case(5)
    out.append((rec, rows, K, 256))
    far = GC.record(0, 0, 2 ** 32 - 300, 2 ** 32 - 1, 2 ** 32 - 280, 2 ** 32 - 1, "-")
    out.append((far, [(2 ** 32 - 200, 2 ** 32 - 120), (2 ** 32 - 100, 2 ** 32 - 215), (2 ** 32 - 1, 0)], 32, 7))
    out.append((GC.record(0, 0, 100, 500, 120, 530, "+"), [(150, 170)], 1, 2 ** 31 - 1))
    out += [(GC.record(0, 0, 100, 500, 120, 530, "+"), [(150, 170)], k, S) for k, S in ((0, 256), (33, 256), (15, 0))]
    return out


def test_shared_header_under_the_sanitizers(tmp_path):
    exe, listing = str(tmp_path / "anchor_plan_sanitized"), str(tmp_path / "cases.txt")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genomeworks_amd", "mapper"),
           os.path.join(ROOT, "tests", "cpp", "anchor_plan_sanitized.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    todo = _plan_cases()
    offsets = [([0, 2, 2, 5], 5, -1), ([1, 2, 5], 5, 0), ([0, 3, 2, 5], 5, 2), ([0, 2, 4], 5, 2), ([0], 0, -1), ([0], 1, 0)]
    with open(listing, "w") as f:
        for o, anchors, k, S in todo:
            f.write("R %d %d %d %d %s %d %d %d %s\n" % (
                o["query_start_position_in_read"], o["query_end_position_in_read"], o["target_start_position_in_read"],
                o["target_end_position_in_read"], chr(o["relative_strand"]), k, S, len(anchors),
                " ".join("%d %d" % (q, t) for q, t in anchors)))
        for values, n_anchors, _ in offsets:
            f.write("O %d %d %s\n" % (len(values) - 1, n_anchors, " ".join(str(v) for v in values)))
    r = subprocess.run([exe, listing], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo) + len(offsets)
    refused = out_of_range = 0
    for line, (o, anchors, k, S) in zip(lines, todo):
        if not (1 <= k <= 32 and S >= 1):
            out_of_range += 1
            assert line == "range"
            continue
        want = OG.pieces(o, anchors, k, S)
        if want is None:
            refused += 1
            assert line == "-1", (line, anchors)
            continue
        assert [int(v) for v in line.split()] == [len(want)] + [v for p in want for v in p], (line, anchors, k, S)
    assert refused == 8 and out_of_range == 3
    assert [int(v) for v in lines[len(todo):]] == [bad for _, _, bad in offsets]


def _exported(library):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, library)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}


def test_exported_symbols_and_the_build():
    mapper = _exported("libcudamapper.so")
    assert {"gwm_chain_overlaps_anchored", "gwm_chain_overlaps_anchored_device", "gwm_align_overlaps_anchored",
            "gwm_align_bytes_needed_anchored", "gw_mapper_chain_overlaps_anchored", "gw_mapper_chain_overlaps_anchored_host",
            "gw_mapper_align_overlaps_anchored", "gwm_chain_overlaps", "gwm_align_overlaps_scored2"} <= mapper
    from genomeworks_amd import build as B
    assert "mapper/gwm_anchored.hip" in B.MAPPER_KERNEL_SRCS and B.AFFINE_KERNEL_SRCS == ["affine/gwaffine.hip"]
    for name in ("gwm_anchored.hip", "gwm_anchored.hpp", "gwm_anchor_plan.hpp"):
        assert os.path.exists(os.path.join(ROOT, "genomeworks_amd", "mapper", name))


def test_c99_caller_of_both_headers(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text("""
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    gwm_anchor_lists lists = {0, 0, 0, 15, 256};
    int64_t piece_starts[5] = {0, 100, 210, 215, 515};
    int (*align)(const gwm_overlap*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*, const int64_t*,
                 int32_t, uint32_t, const gwm_anchor_lists*, int32_t, const gwm_scoring2*, int64_t, void*, gwm_cigars*) =
        gwm_align_overlaps_anchored;
    int (*chain)(const gwm_anchor*, int64_t, const gwm_chaining*, int32_t, int64_t, int64_t, int64_t, float, void*,
                 gwm_overlap*, int32_t*, int64_t, int64_t*, uint32_t*, int64_t, int64_t*, int64_t*, float*) =
        gwm_chain_overlaps_anchored;
    gw_mapper_cigars* (*entry)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                               const int64_t*, int32_t, uint32_t, const int64_t*, const uint32_t*, int64_t, int32_t, int32_t,
                               const int32_t*, int32_t, int64_t, void*) = gw_mapper_align_overlaps_anchored;
    int64_t (*chained)(const gw_mapper_matcher*, const int32_t[5], int32_t, int64_t, int64_t, int64_t, float, void*, int32_t*,
                       int64_t, int64_t*, uint32_t*, int64_t, int64_t*, float*, void*) = gw_mapper_chain_overlaps_anchored;
    if (!align || !chain || !entry || !chained || lists.spacing != 256)
        return 1;
    printf("%lld %lld %lld\\n", (long long)gwm_align_bytes_needed_anchored(piece_starts, 2, 1, 16, 0),
           (long long)gwm_align_bytes_needed_anchored(piece_starts, 2, 0, 0, 100),
           (long long)gwm_align_bytes_needed_scored(100, 110, 16));
    return 0;
}
""")
    exe = str(tmp_path / "caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", LIB,
                        "-lcudamapper", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + LIB,
                        "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    anchored, default, whole = (int(v) for v in r.stdout.split())
    # the budget of a record in pieces counts the second state buffer and the pieces' small arrays besides
    from genomeworks_amd import cudamapper as cm
    assert anchored == cm.align_bytes_needed_anchored([(100, 110), (5, 300)], (4, 6, 2, 16))
    assert default == cm.align_bytes_needed_anchored([(100, 110), (5, 300)], None, 100)
    one = cm.align_bytes_needed_anchored([(100, 110)], (4, 6, 2, 16))
    assert one == whole + 210 + 64 + 3 * 8 + 4


def test_refusals_that_need_no_device():
    from genomeworks_amd import _native, cudamapper as cm
    queries, targets, overlaps, anchors, _ = GC.hand_made()
    offsets, positions = GC.lists(anchors)
    for kw in (dict(anchor_kmer_size=0), dict(anchor_kmer_size=33), dict(anchor_spacing=0)):
        with pytest.raises(ValueError, match="outside"):
            cm.align_overlaps(overlaps, queries, targets, anchors=(offsets, positions), **kw)
    for bad in (offsets + 1, offsets[:-1], np.concatenate([offsets[:3], offsets[2:3] - 1, offsets[4:]]),
                np.concatenate([offsets[:-1], offsets[-1:] + 1])):
        with pytest.raises(ValueError, match="offsets"):
            cm.align_overlaps(overlaps, queries, targets, anchors=(bad, positions))
    with pytest.raises(ValueError):
        cm.align_overlaps(overlaps, queries, targets, anchors=(offsets, positions), scoring=(4, 6, 0, 16))
    with pytest.raises(ValueError, match="chained"):
        cm.map_reads(queries, return_anchors=True)
    # the C API refuses the same before it uploads anything
    L = _native.mapper()
    q, t = cm._read_set_args(queries, targets)
    records = np.ascontiguousarray(overlaps, cm.OVERLAP)
    sc = np.array((4, 6, 2, 16), np.int32)

    def call(offsets=offsets, k=K, S=256, scoring=sc, values=4, n_anchors=len(positions)):
        return L.gw_mapper_align_overlaps_anchored(cm._p(records), len(records), *q, 0, *t, 0, cm._p(offsets), cm._p(positions),
                                                   n_anchors, k, S, None if scoring is None else cm._p(scoring), values, 0, None)

    for kw, text in ((dict(k=0), "anchor_kmer_size"), (dict(k=33), "anchor_kmer_size"), (dict(S=0), "anchor_spacing"),
                     (dict(offsets=offsets + 1), "offsets"), (dict(n_anchors=len(positions) - 1), "offsets"),
                     (dict(offsets=np.concatenate([offsets[:3], offsets[2:3] - 1, offsets[4:]])), "offsets"),
                     (dict(values=5), "scoring_values"), (dict(scoring=None), "scoring_values"),
                     (dict(scoring=np.array((0, 6, 2, 16), np.int32)), "scoring")):
        assert not call(**kw), kw
        assert text in L.gw_mapper_last_error().decode(), (kw, L.gw_mapper_last_error())
