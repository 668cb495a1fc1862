"""The CPU oracle of cudamapper's on-device overlap alignment (tests/oracle_mapper_align.py) against answers worked
out on paper, an independent replay of its CIGARs and the optimal edit distance; the PAF text with CIGARs; and the
exported symbols of the feature. No GPU."""
import os

import numpy as np

import cigar_replay as R
import mapper_cases as MC
import oracle_aligner as A
import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_mapper_postprocess as P
import test_overlap_alignment as TA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 45000


def known_answer_overlaps(tmp_path):
    """known_answer_case as overlap records over lists of reads: (overlaps, query reads, target reads)"""
    _, _, _, queries, targets, lines, _ = TA.known_answer_case(tmp_path)
    qnames, tnames = list(queries), list(targets)
    o = np.zeros(len(lines), O.OVERLAP)
    for r, line in zip(o, lines):
        f = line.split("\t")
        r["query_read_id"], r["target_read_id"] = qnames.index(f[0]), tnames.index(f[5])
        r["query_start_position_in_read"], r["query_end_position_in_read"] = int(f[2]), int(f[3])
        r["target_start_position_in_read"], r["target_end_position_in_read"] = int(f[7]), int(f[8])
        r["relative_strand"], r["num_residues"] = ord(f[4]), int(f[9])
    return o, [queries[n] for n in qnames], [targets[n] for n in tnames]


def test_complement_table_is_the_aligners():
    assert len(OA.COMPLEMENT) == 256
    assert bytes(OA.COMPLEMENT[c] for c in b"ACGTacgt") == b"TGCATGCA"
    assert OA.COMPLEMENT[ord("N")] == ord("C") and OA.COMPLEMENT[0x80] == ord("T")  # not left alone, as end rescue does


def test_oracle_gives_the_known_answers(tmp_path):
    o, queries, targets = known_answer_overlaps(tmp_path)
    assert {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    got = OA.alignments(o, queries, targets)
    assert [a["cigar"] for a in got] == [c[5] for c in TA.KNOWN_ANSWERS]
    assert [a["edit_distance"] for a in got] == [2] * len(o)
    assert OA.cigars(o, queries, targets) == [c[5] for c in TA.KNOWN_ANSWERS]


def test_oracle_cigars_replay_and_are_optimal():
    reads = MC.synthetic_reads(23, 20000, 7, 2000, 0.03)
    o = P.map_batched(reads, None, 15, 10, 1.0, MC.OVERLAP_PARAMS, LIMIT, rescue=True)
    assert len(o) > 100 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    names = ["read_%d" % i for i in range(len(reads))]
    lengths = [len(r) for r in reads]
    by_name = dict(zip(names, reads))
    groups = P.group_reads_into_indices(lengths, LIMIT)
    got = OA.alignments(o, reads, None, (groups, groups))
    lines = P.format_paf(o, names, lengths, names, lengths, 15).splitlines()
    assert len(got) == len(lines) == len(o)
    for rec, a, line in zip(o, got, lines):
        assert a["status"] == 0 and a["cigar"], line
        replay = R.replay_paf(line + "\tcg:Z:" + a["cigar"], by_name, by_name)
        q, t = OA.slices(rec, reads, reads)
        assert replay.edits == a["edit_distance"] == A.myers_full(q, t)["edit_distance"], line


def test_format_paf_with_cigars(tmp_path):
    from genomeworks_amd import cudamapper as cm
    o, queries, targets = known_answer_overlaps(tmp_path)
    qn, tn = ["q%d" % i for i in range(len(queries))], ["t%d" % i for i in range(len(targets))]
    ql, tl = [len(r) for r in queries], [len(r) for r in targets]
    plain = cm.format_paf(o, qn, ql, tn, tl, 15)
    assert plain == P.format_paf(o, qn, ql, tn, tl, 15)  # unchanged without cigars
    cigars = [c[5] for c in TA.KNOWN_ANSWERS]
    text = cm.format_paf(o, qn, ql, tn, tl, 15, cigars=cigars)
    # print_paf: the twelve columns, a tab, cg:Z:<cigar>
    assert text.splitlines() == [line + "\tcg:Z:" + c for line, c in zip(plain.splitlines(), cigars)]
    assert text.endswith("\n") and text.count("\n") == len(o)
    first = text.splitlines()[0].split("\t")
    assert len(first) == 13 and first[11] == "255" and first[12] == "cg:Z:10M2D110M"
    assert cm.format_paf(o[:0], qn, ql, tn, tl, 15, cigars=[]) == ""
    try:
        cm.format_paf(o, qn, ql, tn, tl, 15, cigars=cigars[:-1])
    except ValueError:
        pass
    else:
        raise AssertionError("one CIGAR per overlap")


def test_mapper_library_exports_the_alignment_api():
    from genomeworks_amd import build as B
    assert "mapper/gwm_align.hip" in B.MAPPER_KERNEL_SRCS
    assert all(not s.startswith("mapper/") for s in B.KERNEL_SRCS + B.HOST_SRCS)
    with open(os.path.join(ROOT, "genomeworks_amd", "lib", "libcudamapper.so"), "rb") as f:
        data = f.read()
    for sym in (b"gwm_align_overlaps", b"gwm_cigars_free", b"gwm_align_bytes_needed", b"gw_mapper_align_overlaps",
                b"gw_mapper_cigars_count", b"gw_mapper_cigars_text_bytes", b"gw_mapper_cigars_copy",
                b"gw_mapper_cigars_destroy", b"gw_mapper_map_batched_aligned", b"gw_mapper_overlaps_cigar_text_bytes",
                b"gw_mapper_overlaps_copy_cigars"):
        assert sym in data, sym
    assert b"libgwhip.so" in data  # the aligner comes from there
    # host arithmetic only: the budget of one overlap grows with its slices and covers bases, states and text
    from genomeworks_amd import cudamapper as cm
    small, large = cm.align_bytes_needed(100, 100, 3000), cm.align_bytes_needed(3000, 3000, 3000)
    assert 4 * 200 < small < large and large > 4 * 6000
