"""cudamapper's on-device overlap alignment (gather -> default aligner -> CIGAR text, tests/oracle_mapper_align.py is
the oracle): the kernel-level call through cm.align_overlaps, the batched driver with align=True and the tool's
--cigar, against answers worked out on paper, the pinned Hirschberg restatement and the existing host path
(the align_overlaps tool), string for string and for every record."""
import os
import subprocess

import numpy as np
import pytest

import mapper_cases as MC
import mapper_postprocess_cases as PC
import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_mapper_postprocess as P
import test_overlap_alignment as TA
from test_mapper_align_oracle import known_answer_overlaps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "genomeworks_amd", "bin", "cudamapper")
HOST_TOOL = os.path.join(ROOT, "genomeworks_amd", "bin", "align_overlaps")
LIMIT = 45000


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def batch_reads():
    return MC.synthetic_reads(23, 20000, 7, 2000, 0.03)


@pytest.fixture(scope="module")
def mapped(cm, batch_reads):
    """the final overlaps of the batched driver with end rescue, and the oracle's alignment of each as ONE call"""
    o = cm.map_reads_batched(batch_reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT,
                             rescue_overlap_ends=True)
    assert len(o) > 100 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    return o, OA.alignments(o, batch_reads)


def same(a, b):
    return a.dtype == O.OVERLAP and np.array_equal(a, np.ascontiguousarray(b, O.OVERLAP))


def slice_lengths(o):
    return (o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"],
            o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"])


def run(tool, args):
    return subprocess.run([tool] + args, capture_output=True, text=True, timeout=300)


def write_fasta(path, names, reads):
    with open(path, "w") as f:
        for n, r in zip(names, reads):
            f.write(">%s some description\n" % n)
            f.write("\n".join(r[i:i + 80] for i in range(0, len(r), 80)) + "\n")


# ---- cm.align_overlaps ---------------------------------------------------------------------------------------------

def test_known_answers(cm, tmp_path):
    o, queries, targets = known_answer_overlaps(tmp_path)
    assert {chr(s) for s in o["relative_strand"]} == {"+", "-"} and "N" in queries[1][:19]
    timings = {}
    cigars, edits = cm.align_overlaps(o, queries, targets, timings=timings)
    assert cigars == [c[5] for c in TA.KNOWN_ANSWERS]
    assert edits.dtype == np.int32 and edits.tolist() == [2] * len(o)
    assert set(timings) == {"gather", "align", "cigar_text"} and all(v > 0 for v in timings.values())


def test_every_mapped_overlap_equals_the_oracle(cm, batch_reads, mapped):
    o, ref = mapped
    cigars, edits = cm.align_overlaps(o, batch_reads)
    assert len(cigars) == len(o)
    assert all(a["status"] == 0 and a["cigar"] for a in ref)
    assert cigars == [a["cigar"] for a in ref]
    assert edits.tolist() == [a["edit_distance"] for a in ref]


@pytest.mark.parametrize("engines", [["-a", "1"], ["-a", "3", "-b", "40"]])
def test_host_path_writes_the_same_cigars(cm, batch_reads, mapped, tmp_path, engines):
    o, _ = mapped
    names = ["read_%d" % i for i in range(len(batch_reads))]
    lengths = [len(r) for r in batch_reads]
    fasta, paf = tmp_path / "reads.fasta", tmp_path / "overlaps.paf"
    write_fasta(fasta, names, batch_reads)
    paf.write_text(cm.format_paf(o, names, lengths, names, lengths, 15))
    host = run(HOST_TOOL, engines + [str(fasta), str(fasta), str(paf)])
    assert host.returncode == 0, host.stderr
    rows = host.stdout.splitlines()
    assert len(rows) == len(o) and all(row.split("\t")[12].startswith("cg:Z:") for row in rows)
    cigars, _ = cm.align_overlaps(o, batch_reads)
    assert [row.split("\t")[12][5:] for row in rows] == cigars


def test_result_does_not_depend_on_the_chunking(cm, batch_reads, mapped):
    o, ref = mapped
    ql, tl = slice_lengths(o)
    capacity = int(ql.max())
    alone = max(cm.align_bytes_needed(int(a), int(b), capacity) for a, b in zip(ql, tl))
    whole = cm.align_overlaps(o, batch_reads, max_device_bytes=0)
    assert whole[0] == [a["cigar"] for a in ref]
    # `alone`: the largest overlap fills a chunk by itself, and no chunk holds many; then a few per chunk
    for budget in (alone, 6 * alone):
        got = cm.align_overlaps(o, batch_reads, max_device_bytes=budget)
        assert got[0] == whole[0] and np.array_equal(got[1], whole[1]), budget
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.align_overlaps(o, batch_reads, max_device_bytes=alone - 1)
    assert cm.align_overlaps(o[:5], batch_reads)[0] == OA.cigars(o[:5], batch_reads)  # no state left behind


def test_bytes_outside_acgt_take_the_aligners_table(cm, batch_reads, mapped):
    o, _ = mapped
    reads = [r.encode() for r in batch_reads]
    rng = np.random.default_rng(5)
    for i in range(len(reads)):
        r = bytearray(reads[i])
        for _ in range(6):
            at = int(rng.integers(0, len(r) - 40))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                r[at:at + 3] = b"NNN"
            elif kind == 1:
                r[at:at + 30] = bytes(r[at:at + 30]).lower()
            else:
                r[at] = int(rng.integers(0x80, 0x100))
        reads[i] = bytes(r)
    ref = OA.alignments(o, reads)
    cigars, edits = cm.align_overlaps(o, reads)
    assert cigars == [a["cigar"] for a in ref] and edits.tolist() == [a["edit_distance"] for a in ref]
    # the check has teeth: with end rescue's complement (other bytes left alone) some '-' overlaps align differently
    saved, OA.COMPLEMENT = OA.COMPLEMENT, bytes.maketrans(b"ACGT", b"TGCA")
    try:
        other = OA.cigars(o, reads)
    finally:
        OA.COMPLEMENT = saved
    differ = [i for i in range(len(o)) if other[i] != cigars[i]]
    assert differ and all(o[i]["relative_strand"] == ord("-") for i in differ)


def test_first_read_ids_and_target_set(cm, batch_reads, mapped):
    o, _ = mapped
    part = o[:150].copy()
    want = OA.cigars(part, batch_reads)  # another call, another capacity
    assert cm.align_overlaps(part, batch_reads, None)[0] == want
    assert cm.align_overlaps(part, batch_reads, batch_reads)[0] == want
    part["query_read_id"] += 1000
    part["target_read_id"] += 70
    got = cm.align_overlaps(part, batch_reads, batch_reads, first_query_read_id=1000, first_target_read_id=70)
    assert got[0] == want == OA.cigars(part, batch_reads, batch_reads, None, 1000, 70)
    with pytest.raises(cm.MapperError):  # ids below the first read id of the set
        cm.align_overlaps(o[:3], batch_reads, None, first_query_read_id=1)


def test_empty_input_and_empty_slices(cm, batch_reads, mapped):
    cigars, edits = cm.align_overlaps(np.zeros(0, O.OVERLAP), ["ACGT"])
    assert cigars == [] and edits.dtype == np.int32 and len(edits) == 0
    assert cm.align_overlaps(np.zeros(0, O.OVERLAP), [], [])[0] == []
    o, _ = mapped
    e = o[:8].copy()
    for i, (q_empty, t_empty) in enumerate([(True, False), (False, True), (True, True), (False, False)] * 2):
        if q_empty:
            e[i]["query_end_position_in_read"] = e[i]["query_start_position_in_read"]
        if t_empty:
            e[i]["target_end_position_in_read"] = e[i]["target_start_position_in_read"]
    e["relative_strand"][:4], e["relative_strand"][4:] = ord("+"), ord("-")
    ref = OA.alignments(e, batch_reads)
    cigars, edits = cm.align_overlaps(e, batch_reads)
    assert cigars == [a["cigar"] for a in ref] and edits.tolist() == [a["edit_distance"] for a in ref]
    tl = slice_lengths(e)[1]
    assert cigars[0] == "%dI" % tl[0] and cigars[2] == "" and edits[2] == 0 and cigars[1].endswith("D")
    both = e[[2, 6]]
    assert cm.align_overlaps(both, batch_reads)[0] == ["", ""]  # a call of nothing but empty slices


def test_errors_leave_nothing_behind(cm):
    reads = ["ACGT" * 30, "ACGT" * 20]
    ok = PC.overlaps_from_dicts([dict(query_read_id=0, target_read_id=1, query_start_position_in_read=10,
                                      query_end_position_in_read=60, target_start_position_in_read=10,
                                      target_end_position_in_read=60, relative_strand="+")] * 3)
    want = OA.cigars(ok, reads)
    assert cm.align_overlaps(ok, reads)[0] == want
    for strand in "+-":
        for field, value in (("target_end_position_in_read", 81), ("query_end_position_in_read", 121),
                             ("target_read_id", 2), ("query_read_id", 7), ("query_start_position_in_read", 200),
                             ("target_start_position_in_read", 4000000000)):
            bad = ok.copy()
            bad["relative_strand"] = ord(strand)
            bad[1][field] = value
            with pytest.raises(cm.MapperError):
                cm.align_overlaps(bad, reads)
            assert cm.align_overlaps(ok, reads)[0] == want
    with pytest.raises(cm.MapperError):
        cm.align_overlaps(ok, reads, max_device_bytes=-1)


# ---- the batched driver --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("rescue", [False, True])
def test_map_reads_batched_align_all_to_all(cm, batch_reads, rescue, drop):
    kw = dict(filtering_parameter=1.0, max_basepairs_per_index=LIMIT, drop_fused_overlaps=drop,
              rescue_overlap_ends=rescue)
    timings = {}
    o, cigars = cm.map_reads_batched(batch_reads, align=True, timings=timings, **kw)
    assert same(o, cm.map_reads_batched(batch_reads, **kw))
    assert same(o, P.map_batched(batch_reads, None, 15, 10, 1.0, MC.OVERLAP_PARAMS, LIMIT, drop_fused_overlaps=drop,
                                 rescue=rescue))
    assert len(o) > 100 and len(cigars) == len(o) and timings["index_pairs"] >= 6
    groups = P.group_reads_into_indices([len(r) for r in batch_reads], LIMIT)
    ref = OA.alignments(o, batch_reads, None, (groups, groups))
    assert cigars == [a["cigar"] for a in ref]
    assert timings["edit_distances"].tolist() == [a["edit_distance"] for a in ref]
    assert all(timings[k] > 0 for k in ("gather", "align", "cigar_text"))
    # small chunks inside every pair change nothing
    ql, tl = slice_lengths(o)
    alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
    assert cm.map_reads_batched(batch_reads, align=True, max_device_bytes=2 * alone, **kw)[1] == cigars


def test_map_reads_batched_align_query_vs_target(cm, batch_reads):
    half = len(batch_reads) // 2
    q, t = batch_reads[:half], batch_reads[half:]
    kw = dict(filtering_parameter=1.0, max_basepairs_per_index=LIMIT, max_basepairs_per_target_index=30000,
              rescue_overlap_ends=True)
    o, cigars = cm.map_reads_batched(q, t, align=True, **kw)
    assert same(o, cm.map_reads_batched(q, t, **kw)) and len(o) > 50
    groups = (P.group_reads_into_indices([len(r) for r in q], LIMIT),
              P.group_reads_into_indices([len(r) for r in t], 30000))
    assert len(groups[0]) != len(groups[1])
    assert cigars == OA.cigars(o, q, t, groups)


def test_short_reads_are_refused_only_with_align(cm, batch_reads):
    reads = batch_reads[:6] + ["ACGTACGT"] + batch_reads[6:12]
    kw = dict(filtering_parameter=1.0, max_basepairs_per_index=LIMIT)
    with pytest.raises(cm.MapperError, match=r"k \+ w - 1"):
        cm.map_reads_batched(reads, align=True, **kw)
    with pytest.raises(cm.MapperError, match=r"target read 2"):
        cm.map_reads_batched(batch_reads[:6], batch_reads[6:8] + ["ACGT"], align=True, **kw)
    # without alignment: as before, the read is skipped and the ids behind it shift
    assert same(cm.map_reads_batched(reads, **kw), P.map_batched(reads, None, 15, 10, 1.0, MC.OVERLAP_PARAMS, LIMIT))
    assert cm.map_reads_batched([], align=True, max_basepairs_per_index=100)[1] == []


# ---- the tool ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [[], ["-R"], ["-D", "-R"]])
def test_cudamapper_tool_cigar(cm, batch_reads, tmp_path, flags):
    names = ["read_%d" % i for i in range(len(batch_reads))]
    lengths = [len(r) for r in batch_reads]
    fasta = tmp_path / "reads.fasta"
    write_fasta(fasta, names, batch_reads)
    got = run(TOOL, ["-i", str(LIMIT / 1e6), "--cigar"] + flags + [str(fasta), str(fasta)])
    assert got.returncode == 0, got.stderr
    o, cigars = cm.map_reads_batched(batch_reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT,
                                     drop_fused_overlaps="-D" in flags, rescue_overlap_ends="-R" in flags, align=True)
    assert len(o) > 100
    assert got.stdout == cm.format_paf(o, names, lengths, names, lengths, 15, cigars=cigars)


def test_cudamapper_tool_cigar_refuses_short_reads(batch_reads, tmp_path):
    fasta = tmp_path / "reads.fasta"
    write_fasta(fasta, ["r%d" % i for i in range(7)], batch_reads[:6] + ["ACGTACGT"])
    got = run(TOOL, ["--cigar", str(fasta), str(fasta)])
    assert got.returncode != 0 and got.stdout == "" and "k + w - 1" in got.stderr and "cudamapper:" in got.stderr
    assert "--cigar" in run(TOOL, ["-h"]).stdout
