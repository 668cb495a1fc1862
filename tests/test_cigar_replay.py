"""The CIGAR replayer (tests/cigar_replay.py) on records built by hand: it must accept the correct SAM record of a
reverse-strand overlap and reject the one `align_overlaps -S` used to write for it (the runs in forward order), and
reject every other kind of record that does not describe an alignment of its reads."""
import pytest

import cigar_replay as R

CORE = "ACGTTGCAAGGCTTACCGATCAGTGGTACA"          # 30 bases, the aligned part of the target
RC_CORE = "TGTACCACTGATCGGTAAGCCTTGCAACGT"
TARGETS = {"t1": "GATTACA" + CORE + "CCG"}     # aligned span [7, 37), POS 8
QUERIES = {
    # '-': reverse complement of CORE with "GG" inserted after 3 bases; clips "CA" (left) and "GGATC" (right)
    "q1": "CA" + RC_CORE[:3] + "GG" + RC_CORE[3:] + "GGATC",
    # '-': the same with "AA" inserted in the middle (a palindromic CIGAR); one clip, with an N in it
    "q2": "N" + RC_CORE[:15] + "AA" + RC_CORE[15:],
    # '+': the twin of q1
    "q3": "CA" + CORE[:3] + "GG" + CORE[3:] + "GGATC",
}


def paf(q, qs, qe, strand, cigar):
    return "\t".join(map(str, [q, len(QUERIES[q]), qs, qe, strand, "t1", 40, 7, 37, 3, 32, 255, "cg:Z:" + cigar]))


def sam(q, flag, cigar, pos=8, seq=None):
    if seq is None:
        seq = R.revcomp(QUERIES[q]) if flag == 16 else QUERIES[q]
    return "\t".join(map(str, [q, flag, "t1", pos, 255, cigar, "*", 0, 0, seq, "*"]))


# q1 on paper: the PAF CIGAR walks q1[2:34] against rc(t1[7:37]): 3 matches, the 2 inserted bases (query only:
# cudaaligner's D), 27 matches. SEQ is rc(q1) = "GATCC" + CORE[:27] + "CC" + CORE[27:] + "TG": after the 5-base clip,
# 27 matches against t1[7:34], the 2 bases of the query only (SAM's I), 3 matches, the 2-base clip.
Q1_PAF = paf("q1", 2, 34, "-", "3M2D27M")
Q1_SAM = sam("q1", 16, "5S27M2I3M2S")
Q1_SAM_FORWARD_RUNS = sam("q1", 16, "5S3M2I27M2S")  # what align_overlaps -S wrote before the runs were reversed


def test_correct_reverse_strand_record_replays_to_the_paf_columns():
    p, s = R.check_sam_against_paf(Q1_SAM, Q1_PAF, QUERIES, TARGETS)
    assert (p.matches, p.mismatches, p.ins, p.dels, p.edits) == (30, 0, 0, 2, 2)
    assert p.query_span == s.query_span == (2, 34) and p.target_span == s.target_span == (7, 37)
    assert p.columns[0] == (2, 36, "=") and p.columns[-1] == (33, 7, "=")   # query start pairs with the target end
    assert s.columns[0] == (33, 7, "=") and s.columns[-1] == (2, 36, "=")
    assert [c for c in p.columns if c[2] != "="] == [(5, None, "D"), (6, None, "D")]
    assert len(p.column_set()) == len(p.columns) == 32


def test_forward_order_reverse_strand_record_fails():
    # its lengths add up, so it replays on its own -- to an alignment that shifts 22 bases of SEQ against the target
    wrong = R.replay_sam(Q1_SAM_FORWARD_RUNS, QUERIES, TARGETS)
    assert wrong.mismatches > 10 and wrong.column_set() != R.replay_paf(Q1_PAF, QUERIES, TARGETS).column_set()
    with pytest.raises(R.ReplayError, match="columns differ"):
        R.check_sam_against_paf(Q1_SAM_FORWARD_RUNS, Q1_PAF, QUERIES, TARGETS)


def test_forward_strand_twin_keeps_its_run_order():
    p3 = paf("q3", 2, 34, "+", "3M2D27M")
    p, _ = R.check_sam_against_paf(sam("q3", 0, "2S3M2I27M5S"), p3, QUERIES, TARGETS)
    assert [c for c in p.columns if c[2] != "="] == [(5, None, "D"), (6, None, "D")]
    with pytest.raises(R.ReplayError):
        R.check_sam_against_paf(sam("q3", 0, "2S27M2I3M5S"), p3, QUERIES, TARGETS)


@pytest.mark.parametrize("cigar,why", [
    ("2S27M2I3M5S", "clips on the wrong side"),
    ("5S26M2I3M2S", "a run one short"),
    ("5S28M2I3M2S", "a run one long"),
    ("5S27M2I3M1S", "a clip one short"),
    ("5S27M2I3Y2S", "an unknown operator"),
    ("5S27M2N3M2S", "an operator the writer never uses"),
    ("5S26M1I2I3M2S", "a target base left unused"),
    ("5S27M2D3M2S", "I and D not swapped"),
    ("5S27M2I3M2S1M", "a run after the closing clip"),
])
def test_broken_sam_records_fail(cigar, why):
    with pytest.raises(R.ReplayError):
        R.check_sam_against_paf(sam("q1", 16, cigar), Q1_PAF, QUERIES, TARGETS)


def test_clips_on_the_wrong_side_fail_against_the_span():
    wrong = sam("q1", 16, "2S27M2I3M5S")
    with pytest.raises(R.ReplayError, match="clips the read"):
        R.replay_sam(wrong, QUERIES, TARGETS, query_span=(2, 34))


@pytest.mark.parametrize("cigar,why", [
    ("3M2D26M", "a query and a target base left unused"),
    ("3M2D26M1D", "a target base left unused"),
    ("3M2D28M", "a run one long"),
    ("3M2D27Z", "an unknown operator"),
    ("3M2D27M1S", "a soft clip, which PAF CIGARs do not have"),
    ("3M0I2D27M", "a zero-length run"),
])
def test_broken_paf_records_fail(cigar, why):
    with pytest.raises(R.ReplayError):
        R.replay_paf(paf("q1", 2, 34, "-", cigar), QUERIES, TARGETS)


def test_palindromic_cigar_gives_the_same_answer_either_way():
    # q2[1:33] against rc(t1[7:37]): 15 matches, 2 query-only bases, 15 matches; SEQ = CORE[:15] + "TT" + CORE[15:] + "N"
    p2 = paf("q2", 1, 33, "-", "15M2D15M")
    forward, reverse = "15M2I15M1S", "".join(reversed(["15M", "2I", "15M"])) + "1S"
    assert forward == reverse
    p, s = R.check_sam_against_paf(sam("q2", 16, forward), p2, QUERIES, TARGETS)
    assert (p.matches, p.dels, p.query_span) == (30, 2, (1, 33))
    assert sam("q2", 16, forward).split("\t")[9].endswith("N")   # N is its own complement


def test_seq_must_be_the_read_on_its_strand():
    with pytest.raises(R.ReplayError, match="SEQ"):
        R.replay_sam(sam("q1", 16, "5S27M2I3M2S", seq=QUERIES["q1"]), QUERIES, TARGETS)
    with pytest.raises(R.ReplayError, match="SEQ"):
        R.replay_sam(sam("q2", 16, "15M2I15M1S", seq=R.revcomp(QUERIES["q2"])[:-1] + "A"), QUERIES, TARGETS)
    with pytest.raises(R.ReplayError, match="FLAG"):
        R.replay_sam(sam("q1", 4, "5S27M2I3M2S", seq=QUERIES["q1"]), QUERIES, TARGETS)
    with pytest.raises(R.ReplayError, match="POS"):
        R.replay_sam(sam("q1", 16, "5S27M2I3M2S", pos=0), QUERIES, TARGETS)


def test_match_and_mismatch_operators_are_checked():
    R.replay_paf(paf("q3", 2, 34, "+", "3=2D27="), QUERIES, TARGETS)
    with pytest.raises(R.ReplayError, match="'X' column"):
        R.replay_paf(paf("q3", 2, 34, "+", "3=2D26=1X"), QUERIES, TARGETS)
    shifted = R.replay_paf(paf("q3", 2, 34, "+", "5M2D25M"), QUERIES, TARGETS)   # the gap in the wrong place
    assert shifted.mismatches > 0 and shifted.edits > 2


@pytest.mark.parametrize("cigar", ["", "*", "3", "M", "0M", "03M", "3M ", "3m", "-3M", "3.5M", "3M2"])
def test_parse_cigar_is_strict(cigar):
    with pytest.raises(R.ReplayError):
        R.parse_cigar(cigar, "MIDS=X")


def test_parse_cigar_runs():
    assert R.parse_cigar("5S27M2I3M2S", "MIDS=X") == [(5, "S"), (27, "M"), (2, "I"), (3, "M"), (2, "S")]
    assert R.parse_cigar("120=", "MID=X") == [(120, "=")]
