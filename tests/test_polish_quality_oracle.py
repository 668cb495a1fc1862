"""Base-quality weights without a GPU: the selection with quality sums (Q2) against answers
worked out on paper -- the Python oracle, the C API of libcudamapper.so and a stand-alone caller of the host source
under the address and undefined-behaviour sanitizers --, the public surface, read_fastq, and the window on which
weights change the consensus, on the POA oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_correct as OC
import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_poa as OP
import oracle_polish as OPo
import oracle_polish_quality as OQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def ov(q, t, qs, qe, ts, te, strand="+"):
    return (q, t, qs, ts, qe, te, ord(strand), 0, 0)


def overlaps_of(rows):
    return np.array(rows, O.OVERLAP).reshape(-1)


def segments_of(rows):
    return np.array(rows, OPo.SEGMENT).reshape(-1)


def whole(i):
    """a record of overlap i that spans window 0 of a 100-base target with 100 bases of its query"""
    return (i, 0, 0, 99, 0, 100)


BACKBONE = (1, 0, 0, 100, 0)

# Polishing, one target of 100 bases, W = 100, query i against it over its whole length.
# name -> (queries, quality sums, min_mean_quality, max_depth, the queries whose layers are expected, in order)
POLISH = {
    # 100 bases at threshold 10: a sum of 1000 is a mean of exactly 10 and stays, 999 is one short
    "threshold_equal_kept_one_below_dropped": (2, [1000, 999], 10, 30, [0]),
    # cudapoa refuses a read whose weights are all zero: a zero sum goes whatever the threshold
    "zero_sum_dropped_at_threshold_0": (2, [0, 1], 0, 30, [1]),
    # room for two: had the cut come first it would have kept queries 0 and 1, and the filter would have left one
    "filter_before_the_depth_cut": (4, [5, 2000, 5, 2000], 10, 2, [1, 3]),
    # 42949672 * 100 lies between 2^31 and 2^32: the product is taken in 64 bits, and a saturated sum passes it
    "threshold_product_beyond_32_bits": (2, [2 ** 32 - 1, 2 ** 31], 42949672, 30, [0]),
    "all_dropped": (3, [1, 2, 3], 93, 30, []),
}


def polish_case(name):
    n, sums, q, depth, kept = POLISH[name]
    o = overlaps_of([ov(i, 0, 0, 100, 0, 100, "-" if i % 2 else "+") for i in range(n)])
    s = segments_of([whole(i) for i in range(n)])
    plan = [BACKBONE] + [(0, i, 0, 100, i % 2) for i in kept]
    return o, s, n, [100], np.array(sums, np.uint32), q, depth, (plan, [(0, 0, 0, len(plan))])


# Read correction: reads 0, 1, 2 of 100 bases, the pairs (1, 0) and (2, 0); read 0 owns the target-role records and
# gets layers from reads 1 and 2, reads 1 and 2 own the query-role records and get their layers from read 0.
# name -> (target-role sums, query-role sums (None: not filtered), min_mean_quality, layers of reads 0, 1, 2 (read, ...))
CORRECT = {
    "threshold_equal_kept_one_below_dropped": ([1000, 999], [1000, 999], 10, ([1], [0], [])),
    "zero_sum_dropped_at_threshold_0": ([0, 1], [1, 0], 0, ([2], [0], [])),
    "one_role_without_sums": ([5, 5], None, 10, ([], [0], [0])),
}


def correct_case(name):
    target_sums, query_sums, q, layers = CORRECT[name]
    pairs = overlaps_of([ov(1, 0, 0, 100, 0, 100), ov(2, 0, 0, 100, 0, 100)])
    records = segments_of([whole(0), whole(1)])
    plan, table = [], []
    for r in range(3):
        table.append((r, 0, len(plan), 1 + len(layers[r])))
        plan += [(0, r, 0, 100, 0)] + [(0, other, 0, 100, 0) for other in layers[r]]
    sums = (np.array(target_sums, np.uint32), None if query_sums is None else np.array(query_sums, np.uint32))
    return pairs, records, records, [100, 100, 100], sums, q, (plan, table)


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import build, cudamapper
    build.build_mapper()
    return cudamapper


@pytest.fixture(scope="module")
def small():
    """the small case against a 3 % draft with the oracle's overlaps: reads, qualities, draft, overlaps, alignments"""
    reads, genome = OPo.small_case()
    draft = OPo.draft_of(genome, 0.03, OPo.SMALL["seed"])
    o = OPo.mapped_overlaps(reads, [draft])
    return reads, OQ.qualities_for(reads), draft, o, OA.alignments(o, reads, [draft])


def test_the_quality_generator():
    reads, _ = OPo.small_case()
    q = OQ.qualities_for(reads)
    assert q == OQ.qualities_for(reads) and [len(x) for x in q] == [len(r) for r in reads]
    OQ.check(q, reads)
    means = [sum(ord(c) - 33 for c in x) / len(x) for x in q]
    assert set(q[3]) == {"!"} and all(m < 10 for i, m in enumerate(means) if i % 5 == 0)
    assert all(m > 10 for i, m in enumerate(means) if i % 5 and i != 3)
    assert all(33 + 2 <= ord(c) <= 33 + 40 for i, x in enumerate(q) if i != 3 for c in x)


@pytest.mark.parametrize("name", sorted(POLISH))
def test_polish_selection_on_hand_cases(cm, name):
    o, s, nq, lengths, sums, q, depth, want = polish_case(name)
    assert OQ.select_layers(s, o, lengths, 100, depth, sums, q) == want
    assert cm.select_layers(s, o, nq, lengths, 100, depth, quality_sums=sums, min_mean_quality=q) == want


@pytest.mark.parametrize("name", sorted(CORRECT))
def test_correction_selection_on_hand_cases(cm, name):
    pairs, a, b, lengths, (sa, sb), q, want = correct_case(name)
    assert OQ.select_correction_layers(a, b, pairs, lengths, 100, 30, sa, sb, q) == want
    assert cm.select_correction_layers(a, b, pairs, lengths, 100, 30, target_role_quality_sums=sa,
                                       query_role_quality_sums=sb, min_mean_quality=q) == want


@pytest.mark.parametrize("W", [64, 200])
def test_selection_of_the_small_case_equals_the_oracle(cm, small, W):
    reads, qualities, draft, o, alignments = small
    s = OPo.segments(o, reads, [draft], W, alignments)[0]
    sums = OQ.quality_sums(s, o, qualities)
    plain = cm.select_layers(s, o, len(reads), [len(draft)], W, 15)
    for q in (0, 10, 25):
        want = OQ.select_layers(s, o, [len(draft)], W, 15, sums, q)
        assert cm.select_layers(s, o, len(reads), [len(draft)], W, 15, quality_sums=sums, min_mean_quality=q) == want
        assert len(want[0]) < len(plain[0])  # read 3 is all '!': its records go at any threshold
    # no sums: the unweighted call, row for row
    L = cm._native.mapper()
    lengths = np.array([len(draft)], np.int64)
    s, o = np.ascontiguousarray(s, cm.SEGMENT), np.ascontiguousarray(o, cm.OVERLAP)
    args = (cm._p(s), len(s), cm._p(o), len(o), len(reads), 0, cm._p(lengths), 1, 0, W, 15)
    assert cm._plan_and_table(L.gw_mapper_select_layers_weighted, args + (None, 10)) == plain
    assert plain == OPo.select_layers(s, o, [len(draft)], W, 15) == OQ.select_layers(s, o, [len(draft)], W, 15)


def test_correction_selection_without_sums_is_the_unweighted_one(cm):
    pairs, a, b, lengths, _, _, _ = correct_case("one_role_without_sums")
    plain = cm.select_correction_layers(a, b, pairs, lengths, 100, 30)
    L = cm._native.mapper()
    n = np.array(lengths, np.int64)
    a, b, pairs = (np.ascontiguousarray(x, t) for x, t in ((a, cm.SEGMENT), (b, cm.SEGMENT), (pairs, cm.OVERLAP)))
    args = (cm._p(a), len(a), cm._p(b), len(b), cm._p(pairs), len(pairs), cm._p(n), 3, 0, 100, 30)
    assert cm._plan_and_table(L.gw_mapper_select_correction_layers_weighted, args + (None, None, 10)) == plain
    assert plain == OC.select_correction_layers(a, b, pairs, lengths, 100, 30)
    assert [w[3] for w in plain[1]] == [3, 2, 2]


def test_selection_refusals(cm):
    o, s, nq, lengths, sums, _, depth, _ = polish_case("all_dropped")
    for kw in (dict(quality_sums=sums, min_mean_quality=-1), dict(min_mean_quality=-1)):
        with pytest.raises(cm.MapperError, match="min_mean_quality"):
            cm.select_layers(s, o, nq, lengths, 100, depth, **kw)
    with pytest.raises(ValueError):
        cm.select_layers(s, o, nq, lengths, 100, depth, quality_sums=sums[:2])
    pairs, a, b, n, (sa, _), _, _ = correct_case("one_role_without_sums")
    with pytest.raises(cm.MapperError, match="min_mean_quality"):
        cm.select_correction_layers(a, b, pairs, n, 100, 30, target_role_quality_sums=sa, min_mean_quality=-1)
    # a record that names an overlap that does not exist is refused before its sum is looked at
    bad = s.copy()
    bad[1]["overlap"] = 3
    with pytest.raises(cm.MapperError, match="overlap"):
        cm.select_layers(bad, o, nq, lengths, 100, depth, quality_sums=sums, min_mean_quality=1)


def test_python_refusals_need_no_device():
    from genomeworks_amd import cudamapper as cm, polisher
    reads, genome = OPo.small_case()
    q = OQ.qualities_for(reads)
    none = np.zeros(0, O.OVERLAP)
    short = q[:1] + [q[1][:-1]] + q[2:]
    low = q[:2] + [chr(32) + q[2][1:]] + q[3:]
    high = q[:2] + [chr(127) + q[2][1:]] + q[3:]
    for bad in (short, low, high, q[:-1]):
        with pytest.raises(ValueError):
            OQ.check(bad, reads)
        with pytest.raises(ValueError):
            cm.pack_qualities(bad, reads)
        with pytest.raises(ValueError):
            polisher.polish(reads, [genome], overlaps=none, read_qualities=bad)
        with pytest.raises(ValueError):
            polisher.correct_reads(reads, overlaps=none, qualities=bad)
    with pytest.raises(ValueError):
        polisher.polish(reads, [genome], overlaps=none, target_qualities=["I" * (len(genome) - 1)])
    with pytest.raises(ValueError):
        polisher.polish(reads, [genome], overlaps=none, read_qualities=q, min_mean_quality=-1)
    with pytest.raises(ValueError):
        polisher.correct_reads(reads, overlaps=none, qualities=q, min_mean_quality=-1)
    assert cm.pack_qualities(None, reads) is None
    flat = cm.pack_qualities(q, reads)
    assert flat.dtype == np.uint8 and flat.tobytes().decode("latin-1") == "".join(q)


def sanitizer_text():
    """(cases, expected answers) of tests/cpp/select_quality_sanitized.cpp"""
    text, want = [], []

    def add(kind, head, lengths, overlaps, records, sums, answer):
        text.append("%s %s %d" % (kind, " ".join(str(x) for x in head), sums is not None))
        text.append(" ".join(str(x) for x in lengths))
        text.extend("%d %d %d %d %d %d %c" % tuple(row)[:7] for row in overlaps.tolist())
        text.extend("%d %d %d %d %d %d" % tuple(row) for row in records.tolist())
        if sums is not None:
            text.append(" ".join(str(int(x)) for x in sums))
        if answer is None:
            want.append("error")
        else:
            plan, table = answer
            want.append("case %d %d" % (len(plan), len(table)))
            want.extend(["p %d %d %d %d %d" % p for p in plan] + ["w %d %d %d %d" % w for w in table])

    for name in sorted(POLISH):
        o, s, nq, lengths, sums, q, depth, answer = polish_case(name)
        add("polish", (100, depth, q, nq, 1, len(o), len(s)), lengths, o, s, sums, answer)
    o, s, nq, lengths, sums, _, depth, _ = polish_case("filter_before_the_depth_cut")
    add("polish", (100, depth, 10, nq, 1, len(o), len(s)), lengths, o, s, None,
        OPo.select_layers(s, o, lengths, 100, depth))
    add("polish", (100, depth, -1, nq, 1, len(o), len(s)), lengths, o, s, sums, None)
    for name in sorted(CORRECT):
        pairs, a, b, lengths, (sa, sb), q, answer = correct_case(name)
        if sb is None:
            continue  # the program gives sums to both roles or to neither
        add("correct", (100, 30, q, 3, len(pairs), len(a), len(b)), lengths, pairs, np.concatenate([a, b]),
            np.concatenate([sa, sb]), answer)
    pairs, a, b, lengths, _, _, _ = correct_case("one_role_without_sums")
    add("correct", (100, 30, 10, 3, len(pairs), len(a), len(b)), lengths, pairs, np.concatenate([a, b]), None,
        OC.select_correction_layers(a, b, pairs, lengths, 100, 30))
    add("correct", (100, 30, -1, 3, len(pairs), len(a), len(b)), lengths, pairs, np.concatenate([a, b]), None, None)
    return text, want


def test_selection_under_the_sanitizers(tmp_path, small):
    """the host source and a stand-alone caller with its own main, built with -fsanitize=address,undefined and run as
    a program: the hand cases, and every record of the small case with the oracle's sums"""
    exe = str(tmp_path / "select_quality_sanitized")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "select_quality_sanitized.cpp"),
           os.path.join(ROOT, "genomeworks_amd", "mapper", "gwm_windows.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text, want = sanitizer_text()
    reads, qualities, draft, o, alignments = small
    s = OPo.segments(o, reads, [draft], 64, alignments)[0]
    sums = OQ.quality_sums(s, o, qualities)
    plan, table = OQ.select_layers(s, o, [len(draft)], 64, 15, sums, 10)
    text.append("polish 64 15 10 %d 1 %d %d 1" % (len(reads), len(o), len(s)))
    text.append(str(len(draft)))
    text.extend("%d %d %d %d %d %d %c" % tuple(row)[:7] for row in o.tolist())
    text.extend("%d %d %d %d %d %d" % tuple(row) for row in s.tolist())
    text.append(" ".join(str(int(x)) for x in sums))
    want.append("case %d %d" % (len(plan), len(table)))
    want.extend(["p %d %d %d %d %d" % p for p in plan] + ["w %d %d %d %d" % w for w in table])
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.splitlines() == want


def test_new_c_symbols_are_exported_and_a_caller_compiles(cm, tmp_path):
    from genomeworks_amd import build
    build.build_host()
    C.CDLL(os.path.join(LIB, "libgwhip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIB, "libcudamapper.so"))
    for name in ("gwm_segment_quality_sums", "gwm_gather_weights", "gw_mapper_window_overlaps_weighted",
                 "gw_mapper_correction_windows_weighted", "gw_mapper_windows_copy_weights",
                 "gw_mapper_select_layers_weighted", "gw_mapper_select_correction_layers_weighted",
                 "gw_mapper_segment_quality_sums"):
        assert hasattr(lib, name), name
    host = C.CDLL(os.path.join(LIB, "libgenomeworks_amd.so"))
    assert hasattr(host, "gw_poa_multi_device_run_weighted")
    src = tmp_path / "caller.c"
    src.write_text("""
#include "gw_capi.h"
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"
#include <stdio.h>
int main(void)
{
    gwm_segment s[2] = {{0, 0, 0, 9, 0, 10}, {1, 0, 0, 9, 0, 10}};
    gwm_overlap o[2] = {{0, 0, 0, 0, 10, 10, '+', 0, 0}, {1, 0, 0, 0, 10, 10, '-', 0, 0}};
    int64_t lengths[1] = {10}, n_windows = 0;
    uint32_t sums[2] = {99, 100}, plan[15], table[4];
    int (*sums_kernel)(const gwm_segment*, int64_t, const gwm_overlap*, int64_t, int32_t, const char*, const int64_t*,
                       int32_t, uint32_t, uint32_t*, void*, float*) = gwm_segment_quality_sums;
    int (*weights_kernel)(const gwm_gather_entry*, int64_t, const int64_t*, const char*, const int64_t*, int32_t,
                          const char*, const int64_t*, int32_t, int8_t*, int64_t, void*, float*) = gwm_gather_weights;
    gw_mapper_windows* (*polish)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                                 const int64_t*, int32_t, uint32_t, const char*, const char*, int32_t, int32_t, int32_t,
                                 int64_t, void*) = gw_mapper_window_overlaps_weighted;
    gw_mapper_windows* (*correct)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                                  int32_t, int32_t, int32_t, int64_t, void*) = gw_mapper_correction_windows_weighted;
    int (*copy)(const gw_mapper_windows*, int8_t*, uint32_t*, uint32_t*, float*) = gw_mapper_windows_copy_weights;
    int (*alone)(const void*, int64_t, const void*, int64_t, int32_t, const char*, const int64_t*, int32_t, uint32_t,
                 uint32_t*, void*, float*) = gw_mapper_segment_quality_sums;
    gw_poa_multi* (*poa)(int32_t, const int32_t*, const char* const*, const int32_t*, const int8_t* const*,
                         const gw_poa_batch_config*, const int32_t*, int32_t, int32_t, int64_t, int8_t, int16_t, int16_t,
                         int16_t) = gw_poa_multi_device_run_weighted;
    int64_t n = gw_mapper_select_layers_weighted(s, 2, o, 2, 2, 0, lengths, 1, 0, 10, 30, sums, 10, plan, 3, &n_windows,
                                                 table, 1);
    int64_t m = gw_mapper_select_correction_layers_weighted(s, 0, s, 0, o, 0, lengths, 1, 0, 10, 30, sums, sums, 10, plan,
                                                            0, &n_windows, table, 0);
    if (!sums_kernel || !weights_kernel || !polish || !correct || !copy || !alone || !poa || n != 2 || m != 1 ||
        n_windows != 1 || plan[6] != 1 || plan[9] != 1 || table[3] != 2)
        return 1;
    if (gw_mapper_select_layers_weighted(s, 2, o, 2, 2, 0, lengths, 1, 0, 10, 30, sums, -1, plan, 3, &n_windows, table,
                                         1) != GW_MAPPER_ERROR)
        return 2;
    puts("ok");
    return 0;
}
""")
    exe = str(tmp_path / "caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", LIB,
                        "-lcudamapper", "-lgenomeworks_amd", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
                        "-Wl,-rpath," + LIB, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) == (0, "ok"), r.stderr


def test_the_new_source_is_part_of_the_mapper_library():
    from genomeworks_amd import build
    assert "mapper/gwm_qualities.hip" in build.MAPPER_KERNEL_SRCS
    assert not any(s.startswith("csrc/") for s in build.MAPPER_KERNEL_SRCS + build.MAPPER_HOST_SRCS)


def test_read_fastq_round_trip_and_refusals(tmp_path):
    from genomeworks_amd import polisher
    reads, _ = OPo.small_case()
    reads = reads[:3] + [""] + reads[3:5] + [""]
    qualities = OQ.qualities_for(reads)
    names = ["read%d" % i for i in range(len(reads))]
    path = tmp_path / "reads.fastq"
    path.write_text("".join("@%s length=%d\n%s\n+%s\n%s\n" % (n, len(r), r, n if i % 2 else "", q)
                            for i, (n, r, q) in enumerate(zip(names, reads, qualities))))
    assert polisher.read_fastq(str(path)) == (names, reads, qualities)
    # a quality line that starts with '@' is no header; windows line ends and empty lines at the end are fine
    path.write_bytes(b"@a\r\nACGT\r\n+\r\n@II!\r\n@b x\r\nAC\r\n+b\r\n~~\r\n\r\n\n")
    assert polisher.read_fastq(str(path)) == (["a", "b"], ["ACGT", "AC"], ["@II!", "~~"])
    path.write_text("")
    assert polisher.read_fastq(str(path)) == ([], [], [])
    refused = {
        "truncated": "@a\nACGT\n+\n",
        "wrapped": "@a\nAC\nGT\n+\nIIII\n",
        "fasta": ">a\nACGT\n+\nIIII\n",
        "no_plus": "@a\nACGT\n-\nIIII\n",
        "no_name": "@\nACGT\n+\nIIII\n",
        "short_quality": "@a\nACGT\n+\nIII\n",
        "byte_32": "@a\nACGT\n+\nII I\n",
        "byte_127": "@a\nACGT\n+\nII\x7fI\n",
        "second_record": "@a\nACGT\n+\nIIII\nb\nAC\n+\nII\n",
    }
    for name, text in refused.items():
        path.write_text(text)
        with pytest.raises(ValueError):
            polisher.read_fastq(str(path))
    with pytest.raises(OSError):
        polisher.read_fastq(str(tmp_path / "missing.fastq"))


def test_weights_flip_the_paper_window_on_the_poa_oracle():
    """backbone and two layers share a substitution at position 100, the third layer is the truth: three against one
    without weights, 1 + 2 + 2 against 40 with them"""
    truth, reads, weights = OQ.paper_case()
    assert len(truth) == 333 and [sum(a != b for a, b in zip(r, truth)) for r in reads] == [1, 1, 1, 0]
    assert reads[0][100] != truth[100]
    with OP.Workspace(OP.make_cfg(512, 8, 128, 1)) as ws:
        plain = ws.process(reads)
        weighted = ws.process(reads, weights)
    assert int(plain["status"]) == 0 and int(weighted["status"]) == 0
    assert plain["consensus"] == reads[0] and weighted["consensus"] == truth


def test_oracle_pipeline_drops_the_low_quality_reads(small):
    reads, qualities, draft, o, alignments = small
    plain = OPo.windows(o, reads, [draft], 200, 15, alignments)
    with_q = OQ.polish_windows(o, reads, [draft], 200, 15, qualities, None, 10, alignments)
    assert [(t, k) for t, k, _ in plain] == [(t, k) for t, k, _, _ in with_q]
    assert sum(len(s) for _, _, s in plain) > sum(len(s) for _, _, s, _ in with_q)
    for _, _, seqs, weights in with_q:
        assert [len(s) for s in seqs] == [len(w) for w in weights] and set(weights[0].tolist()) == {1}
        assert all(w.dtype == np.int8 and w.min() >= 2 and w.max() <= 40 and w.mean() >= 10 for w in weights[1:])
    # threshold 0 and no zero-sum layer: the sequences of the unweighted windows, byte for byte
    keep = [i for i in range(len(reads)) if i != 3]
    kept_o = o[np.isin(o["query_read_id"], keep)]
    kept_a = [a for a, x in zip(alignments, o) if int(x["query_read_id"]) in keep]
    assert [w[:3] for w in OQ.polish_windows(kept_o, reads, [draft], 200, 15, qualities, None, 0, kept_a)] == \
        OPo.windows(kept_o, reads, [draft], 200, 15, kept_a)
