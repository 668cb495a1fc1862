"""Polishing without a GPU: the two formulations of the segments agree, the layer selection against answers worked out
on paper (the Python oracle, the C API of libcudamapper.so and a stand-alone caller of the host source under the
address and undefined-behaviour sanitizers), the public surface, and the oracle pipeline's effect on a draft."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_polish as OPo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
WINDOW_LENGTHS = (7, 64, 200, 4096)


def ov(q, t, qs, qe, ts, te, strand="+"):
    return (q, t, qs, ts, qe, te, ord(strand), 0, 0)


def overlaps_of(rows):
    return np.array(rows, O.OVERLAP).reshape(-1)


def segments_of(rows):
    return np.array(rows, OPo.SEGMENT).reshape(-1)


# name -> (overlaps, segments (overlap, window, target_first, target_last, query_begin, query_end), n_queries,
#          target lengths, W, max_depth, first ids, expected plan (set, read, begin, end, reversed),
#          expected windows (target_read, window, first_sequence, sequences))
HAND = {
    # query 0: two overlaps of span 100, the first speaks; query 1: the span of 250 beats the span of 100 behind it.
    # Its piece of window 2 ends at 249, 50 short of the window's end
    "tie_on_span": (
        [ov(0, 0, 0, 100, 0, 100), ov(0, 0, 100, 200, 100, 200), ov(1, 0, 0, 250, 0, 250), ov(1, 0, 0, 100, 0, 100)],
        [(0, 0, 0, 99, 0, 100), (1, 1, 100, 199, 100, 200), (2, 0, 0, 99, 0, 100), (2, 1, 100, 199, 100, 200),
         (2, 2, 200, 249, 200, 250), (3, 0, 0, 99, 0, 100)],
        2, [300], 100, 30, (0, 0),
        [(1, 0, 0, 100, 0), (0, 0, 0, 100, 0), (0, 1, 0, 100, 0), (1, 0, 100, 200, 0), (0, 1, 100, 200, 0),
         (1, 0, 200, 300, 0)],
        [(0, 0, 0, 3), (0, 1, 3, 2), (0, 2, 5, 1)]),
    # W = 200: W / 100 = 2 bases of slack on either side, 3 are one too many
    "slack_boundary": (
        [ov(0, 0, 0, 198, 2, 200), ov(1, 0, 0, 197, 3, 200), ov(2, 0, 0, 198, 0, 198), ov(3, 0, 0, 197, 0, 197),
         ov(4, 0, 0, 197, 202, 399), ov(5, 0, 0, 196, 203, 399)],
        [(0, 0, 2, 199, 0, 198), (1, 0, 3, 199, 0, 197), (2, 0, 0, 197, 0, 198), (3, 0, 0, 196, 0, 197),
         (4, 1, 202, 398, 0, 197), (5, 1, 203, 398, 0, 196)],
        6, [401], 200, 30, (0, 0),
        [(1, 0, 0, 200, 0), (0, 2, 0, 198, 0), (0, 0, 0, 198, 0), (1, 0, 200, 400, 0), (0, 4, 0, 197, 0),
         (1, 0, 400, 401, 0)],
        [(0, 0, 0, 3), (0, 1, 3, 2), (0, 2, 5, 1)]),
    # W = 10: no slack; 20 query bases are a layer, 21 and none are not
    "length_bound": (
        [ov(0, 0, 0, 20, 0, 10), ov(1, 0, 0, 21, 0, 10), ov(2, 0, 5, 5, 0, 10), ov(3, 0, 7, 8, 0, 10)],
        [(0, 0, 0, 9, 0, 20), (1, 0, 0, 9, 0, 21), (2, 0, 0, 9, 5, 5), (3, 0, 0, 9, 7, 8)],
        4, [10], 10, 30, (0, 0),
        [(1, 0, 0, 10, 0), (0, 0, 0, 20, 0), (0, 3, 7, 8, 0)],
        [(0, 0, 0, 3)]),
    # four layers, room for three: by (target_first, position in the input); the '-' one is marked reversed
    "depth_cap_order": (
        [ov(0, 0, 0, 99, 1, 100), ov(1, 0, 0, 100, 0, 100, "-"), ov(2, 0, 0, 99, 1, 100), ov(3, 0, 0, 100, 0, 100)],
        [(0, 0, 1, 99, 0, 99), (1, 0, 0, 99, 0, 100), (2, 0, 1, 99, 0, 99), (3, 0, 0, 99, 0, 100)],
        4, [100], 100, 3, (0, 0),
        [(1, 0, 0, 100, 0), (0, 1, 0, 100, 1), (0, 3, 0, 100, 0), (0, 0, 0, 99, 0)],
        [(0, 0, 0, 4)]),
    # a read of 250 bases: window 2 ends at 250, and the slack counts from there
    "last_window_shorter": (
        [ov(0, 0, 0, 50, 200, 250), ov(1, 0, 0, 49, 200, 249), ov(2, 0, 0, 48, 200, 248)],
        [(0, 2, 200, 249, 0, 50), (1, 2, 200, 248, 0, 49), (2, 2, 200, 247, 0, 48)],
        3, [250], 100, 30, (0, 0),
        [(1, 0, 0, 100, 0), (1, 0, 100, 200, 0), (1, 0, 200, 250, 0), (0, 0, 0, 50, 0), (0, 1, 0, 49, 0)],
        [(0, 0, 0, 1), (0, 1, 1, 1), (0, 2, 2, 3)]),
    # targets of 40 bases, of none and of exactly W; read ids count from 5 and 9
    "target_below_w": (
        [ov(5, 9, 3, 43, 0, 40), ov(6, 11, 0, 100, 0, 100, "-")],
        [(0, 0, 0, 39, 3, 43), (1, 0, 0, 99, 0, 100)],
        2, [40, 0, 100], 100, 30, (5, 9),
        [(1, 0, 0, 40, 0), (0, 0, 3, 43, 0), (1, 2, 0, 100, 0), (0, 1, 0, 100, 1)],
        [(0, 0, 0, 2), (2, 0, 2, 2)]),
}


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import build, cudamapper
    build.build_mapper()
    return cudamapper


@pytest.fixture(scope="module")
def small():
    """the small case against a 3 % draft: reads, draft, the oracle's overlaps and their alignments"""
    reads, genome = OPo.small_case()
    draft = OPo.draft_of(genome, 0.03, OPo.SMALL["seed"])
    o = OPo.mapped_overlaps(reads, [draft])
    assert len(o) >= 20 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    return reads, draft, o, OA.alignments(o, reads, [draft])


@pytest.mark.parametrize("W", WINDOW_LENGTHS)
def test_two_segment_formulations_agree(small, W):
    reads, draft, o, alignments = small
    by_states = OPo.segments(o, reads, [draft], W, alignments)
    by_cigar = OPo.segments(o, reads, [draft], W, alignments, "cigar")
    assert len(by_states[0]) >= len(o) and np.array_equal(by_states[0], by_cigar[0])
    assert np.array_equal(by_states[1], by_cigar[1]) and by_states[1][-1] == len(by_states[0])
    s = by_states[0]
    assert np.all(s["target_first"] // W == s["window"]) and np.all(s["target_last"] // W == s["window"])
    if W == 4096:
        assert np.array_equal(s["overlap"], np.arange(len(o)))  # one window per overlap


@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_selection_on_hand_cases(name):
    o, s, _, lengths, W, depth, (fq, ft), plan, table = HAND[name]
    assert OPo.select_layers(segments_of(s), overlaps_of(o), lengths, W, depth, fq, ft) == (plan, table)


@pytest.mark.parametrize("name", sorted(HAND))
def test_c_api_selection_on_hand_cases(cm, name):
    o, s, nq, lengths, W, depth, (fq, ft), plan, table = HAND[name]
    assert cm.select_layers(segments_of(s), overlaps_of(o), nq, lengths, W, depth, fq, ft) == (plan, table)


@pytest.mark.parametrize("W", WINDOW_LENGTHS)
@pytest.mark.parametrize("depth", [0, 3, 30])
def test_c_api_selection_equals_the_oracle(cm, small, W, depth):
    reads, draft, o, alignments = small
    s = OPo.segments(o, reads, [draft], W, alignments)[0]
    want = OPo.select_layers(s, o, [len(draft)], W, depth)
    assert cm.select_layers(s, o, len(reads), [len(draft)], W, depth) == want
    assert len(want[1]) == (len(draft) + W - 1) // W and (depth == 0 or W == 4096 or len(want[0]) > len(want[1]))


def test_c_api_selection_refusals(cm):
    o, s, nq, lengths, W, depth, _, _, _ = HAND["tie_on_span"]
    o, s = overlaps_of(o), segments_of(s)
    for kw in (dict(window_length=0), dict(max_depth=-1)):
        with pytest.raises(cm.MapperError):
            cm.select_layers(s, o, nq, lengths, **dict(dict(window_length=W, max_depth=depth), **kw))
    for field, value in (("overlap", 4), ("window", 3), ("target_last", 300)):
        bad = s.copy()
        bad[4][field] = value
        with pytest.raises(cm.MapperError):
            cm.select_layers(bad, o, nq, lengths, W, depth)
    with pytest.raises(cm.MapperError):  # a read id outside its set
        cm.select_layers(s, o, 1, lengths, W, depth)
    assert cm.select_layers(s[:0], o[:0], 0, [], W, depth) == ([], [])


def test_selection_under_the_sanitizers(tmp_path):
    """the host source and a stand-alone caller, built with -fsanitize=address,undefined, on the hand cases"""
    exe = str(tmp_path / "select_layers_sanitized")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "select_layers_sanitized.cpp"),
           os.path.join(ROOT, "genomeworks_amd", "mapper", "gwm_windows.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = sorted(HAND)
    text, want = [], []
    for name in names:
        o, s, nq, lengths, W, depth, (fq, ft), plan, table = HAND[name]
        text.append("case %d %d %d %d %d %d %d %d" % (W, depth, nq, fq, len(lengths), ft, len(o), len(s)))
        text.append(" ".join(str(x) for x in lengths))
        text += ["%d %d %d %d %d %d %c" % row[:7] for row in o]
        text += ["%d %d %d %d %d %d" % row for row in s]
        want.append("case %d %d" % (len(plan), len(table)))
        want += ["p %d %d %d %d %d" % p for p in plan] + ["w %d %d %d %d" % w for w in table]
    # what the selection refuses: a window length of 0, and a segment of an overlap that does not exist
    text += ["case 0 3 1 0 1 0 0 0", "10", "case 10 3 1 0 1 0 0 1", "10", "0 0 0 9 0 10"]
    want += ["error", "error"]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.splitlines() == want


def test_new_c_symbols_are_exported_and_a_caller_compiles(cm, tmp_path):
    C.CDLL(os.path.join(LIB, "libgwhip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIB, "libcudamapper.so"))
    for name in ("gwm_window_segments", "gwm_segments_free", "gwm_gather_sequences", "gw_mapper_window_overlaps", "gw_mapper_window_segments",
                 "gw_mapper_windows_counts", "gw_mapper_windows_copy_segments", "gw_mapper_windows_copy_windows",
                 "gw_mapper_windows_destroy", "gw_mapper_select_layers"):
        assert hasattr(lib, name), name
    src = tmp_path / "caller.c"
    src.write_text("""
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"
#include <stdio.h>
int main(void)
{
    gwm_segment s = {0, 0, 0, 9, 0, 10};
    gwm_overlap o = {0, 0, 0, 0, 10, 10, '+', 0, 0};
    int64_t lengths[1] = {10}, n_windows = 0;
    uint32_t plan[10], table[4];
    void (*release)(gwm_segments*) = gwm_segments_free;
    gw_mapper_windows* (*entry)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                                const int64_t*, int32_t, uint32_t, int32_t, int32_t, int64_t, void*) =
        gw_mapper_window_overlaps;
    int64_t n = gw_mapper_select_layers(&s, 1, &o, 1, 1, 0, lengths, 1, 0, 10, 30, plan, 2, &n_windows, table, 1);
    if (sizeof(gwm_segment) != 24 || sizeof(gwm_gather_entry) != 20 || !entry || !release || n != 2 || n_windows != 1 ||
        plan[5] != 0 || plan[8] != 10 || table[3] != 2)
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


def test_kernel_digest_ignores_the_new_sources():
    from genomeworks_amd import build
    assert "mapper/gwm_segments.hip" in build.MAPPER_KERNEL_SRCS and "mapper/gwm_windows.cpp" in build.MAPPER_HOST_SRCS
    assert not any(s.startswith("csrc/") for s in build.MAPPER_KERNEL_SRCS + build.MAPPER_HOST_SRCS)


def test_polish_refusals_need_no_device():
    from genomeworks_amd import polisher
    reads, genome = OPo.small_case()
    with pytest.raises(ValueError):
        polisher.polish(reads, [genome], window_length=0)
    with pytest.raises(ValueError):
        polisher.polish(reads + ["ACGT"], [genome])
    with pytest.raises(TypeError):
        polisher.polish(reads, [genome], overlaps=np.zeros(0, O.OVERLAP), k=15)
    assert polisher.poa_batch_shape(200, 15, 64) == (400, 16, 128) == OPo.poa_shape(200, 15, 64)
    assert polisher.poa_batch_shape(7, 3, 256) == (256, 4, 256) == OPo.poa_shape(7, 3, 256)


# seeds of the small case's shape for which the oracle pipeline alone improves the draft, with the window length used
IMPROVING = [(11, 150), (12, 200), (13, 300), (14, 200), (15, 500)]


@pytest.mark.parametrize("seed,W", IMPROVING)
def test_oracle_pipeline_improves_the_draft(seed, W):
    reads, genome = OPo.small_case(seed)
    draft = OPo.draft_of(genome, 0.03, seed)
    o = OPo.mapped_overlaps(reads, [draft])
    polished, report = OPo.polish(reads, [draft], o, W, 15, 64)
    before, after = OPo.edit_distance(draft, genome), OPo.edit_distance(polished[0], genome)
    print("seed %d W %d: draft %d, polished %d" % (seed, W, before, after))
    assert after < before
    # the end windows keep their backbone for want of spanning layers; the windows in between go through the POA
    assert report[0][2:] == (0, None, True) and report[-1][3:] == (None, True)
    assert sum(1 for r in report if r[3] == 0 and not r[4]) >= 1
    assert [r[:2] for r in report] == [(0, k) for k in range((len(draft) + W - 1) // W)]
