"""Variant-calling cases worked out on paper, shared by tests/test_variants_oracle.py and
tests/test_gpu_variants.py. They are built on tests/pileup_cases.py: the target is PC.TARGET, whose slice PC.T has no A
and no two equal neighbours, every read holds one query slice between a G and a C as PC.reads() lays them out, and
every record is made as PC.record makes it. A substituted base may be any letter (two slices of equal length that
differ in one base have one optimal alignment); an inserted base differs from both of its neighbours; a deleted base
differs from both of its neighbours. The alignments are therefore unique and the expectations literal.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle_mapper as O
import oracle_variants as OV
import pileup_cases as PC

T, TS, QS = PC.T, PC.TS, PC.QS
A, C, G, T_ = 0, 1, 2, 3  # channels


def build(slices):
    """(reads, records) of query slices [(slice, strand)] against PC.TARGET: read 0 is the target, read 1 + i holds
    slice i; on '-' the slice is given as the query has it (the reverse complement of what the target sees)"""
    reads = [PC.TARGET] + ["G" + s + "C" for s, _ in slices]
    rows = [(1 + i, 0, QS, TS, QS + len(s), TS + len(T), ord(strand), 0, 0) for i, (s, strand) in enumerate(slices)]
    return reads, np.array(rows, O.OVERLAP).reshape(-1)


def forward(s, strand):
    """a slice written in forward target coordinates, as the query of `strand` holds it"""
    return (s if strand == "+" else PC.rc(s), strand)


def substituted(at, base):
    return T[:at] + base + T[at + 1:]


def inserted(after, bases):
    return T[:after + 1] + bases + T[after + 1:]


def deleted(at, n=1):
    return T[:at] + T[at + n:]


def variant(p, kind, ref, count, depth, alt=0, allele=""):
    """one expected VARIANT row of target 0 at slice position p"""
    return (0, TS + p, count, depth, kind, ref, alt, len(allele), OV.pack_key(allele))


def rows(*variants):
    return np.array(list(variants), OV.VARIANT).reshape(-1)


# name -> (slices in forward target coordinates with their strands, min_count, min_percent, expected records)
def _cases():
    cases = {}
    for strand, tag in (("+", ""), ("-", "_reverse")):
        def on(*slices):
            return [forward(s, strand) for s in slices]
        # T[4] = C reads A in three of four reads
        cases["snv" + tag] = (on(*[substituted(4, "A")] * 3, T), 3, 30, rows(variant(4, OV.SNV, C, 3, 4, alt=A)))
        # T[5] = T, between C and G, is missing from three of four reads
        cases["deleted_base" + tag] = (on(*[deleted(5)] * 3, T), 3, 30, rows(variant(5, OV.DELETION, T_, 3, 4)))
        # AA between T[5] and T[6] in three of four reads; on '-' the queries hold TT
        cases["insertion_of_two" + tag] = (on(*[inserted(5, "AA")] * 3, T), 3, 30,
                                           rows(variant(5, OV.INSERTION, T_, 3, 4, allele="AA")))
        # the count at its edge: min_count - 1 and exactly min_count, the percentage out of the way
        cases["count_below" + tag] = (on(*[substituted(4, "A")] * 2, T, T), 3, 0, rows())
        cases["count_reached" + tag] = (on(*[substituted(4, "A")] * 3, T), 3, 0, rows(variant(4, OV.SNV, C, 3, 4, alt=A)))
        # 100 k == min_percent d: 3 of 10 at 30 per cent is called, 3 of 11 is not
        cases["percent_reached" + tag] = (on(*[substituted(4, "A")] * 3, *[T] * 7), 1, 30,
                                          rows(variant(4, OV.SNV, C, 3, 10, alt=A)))
        cases["percent_below" + tag] = (on(*[substituted(4, "A")] * 3, *[T] * 8), 1, 30, rows())
        # the same three kinds of edge for a deletion and an insertion: 1 of 4 at 25 per cent, and at 26
        cases["percent_reached_others" + tag] = (on(deleted(5), inserted(1, "A"), T, T), 1, 25,
                                                 rows(variant(1, OV.INSERTION, G, 1, 4, allele="A"),
                                                      variant(5, OV.DELETION, T_, 1, 4)))
        cases["percent_below_others" + tag] = (on(deleted(5), inserted(1, "A"), T, T), 1, 26, rows())
        # min_percent 0: one read of twelve is enough; 100: all of them are needed
        cases["percent_0" + tag] = (on(substituted(4, "A"), *[T] * 11), 1, 0, rows(variant(4, OV.SNV, C, 1, 12, alt=A)))
        cases["percent_100" + tag] = (on(*[substituted(4, "A")] * 3), 1, 100, rows(variant(4, OV.SNV, C, 3, 3, alt=A)))
        cases["percent_100_missed" + tag] = (on(*[substituted(4, "A")] * 3, T), 1, 100, rows())
        # two alt bases with equal counts: the smaller channel, G before T
        cases["snv_tie" + tag] = (on(*[substituted(4, "T")] * 2, *[substituted(4, "G")] * 2), 2, 0,
                                  rows(variant(4, OV.SNV, C, 2, 4, alt=G)))
        # alleles A, AA and T after T[0] = C (before T[1] = G) with 2, 2 and 1 records: the shorter of the two best.
        # The count is the allele's; the pileup's insertion channel there is 5
        cases["allele_tie_shorter" + tag] = (on(*[inserted(0, "AA")] * 2, inserted(0, "T"), *[inserted(0, "A")] * 2), 2, 0,
                                             rows(variant(0, OV.INSERTION, C, 2, 5, allele="A")))
        # C against A after T[1] = G (before T[2] = T) with equal counts: the smaller key
        cases["allele_tie_key" + tag] = (on(*[inserted(1, "C")] * 2, *[inserted(1, "A")] * 2), 2, 0,
                                         rows(variant(1, OV.INSERTION, G, 2, 4, allele="A")))
        # all three kinds in one cell and its neighbour, in the order of the result: T[4] reads A twice and is deleted
        # twice (the depth counts the deletions), and AA follows it twice
        cases["three_kinds" + tag] = (on(*[substituted(4, "A")] * 2, *[deleted(4)] * 2, *[inserted(4, "AA")] * 2), 2, 0,
                                      rows(variant(4, OV.SNV, C, 2, 6, alt=A), variant(4, OV.DELETION, C, 2, 6),
                                           variant(4, OV.INSERTION, C, 2, 6, allele="AA")))
        # runs in the first and in the last column have a neighbour on one side only: counted nowhere, never called
        cases["runs_at_both_ends" + tag] = (on("AA" + T + "A"), 1, 0, rows())
    return cases


CASES = _cases()
NAMES = sorted(CASES)
# where the insertion channel of the pileup differs from the count of the called allele
INSERTION_CHANNEL = {"allele_tie_shorter": (TS + 0, 5), "allele_tie_shorter_reverse": (TS + 0, 5)}


def case(name):
    """(reads, records, min_count, min_percent, expected VARIANT rows)"""
    slices, min_count, min_percent, want = CASES[name]
    reads, o = build(slices)
    return reads, o, min_count, min_percent, want


def same_records(a, b):
    """every field of every record; the padding of the dtype is not looked at"""
    return a.dtype == b.dtype == OV.VARIANT and a.shape == b.shape and a.tolist() == b.tolist()


def long_target():
    """150 bases of C, G, T without two equal neighbours (as tests/test_gpu_pileup.py uses for the tile boundary)"""
    return PC.unique_target(np.random.default_rng(150), 150)


def run_case(column, length, strand):
    """(reads, records): one read with `length` A's in front of column `column` of an alignment against long_target()
    -- on '-' against its reverse complement as the target read, so the aligner sees the same two sequences --, and
    the expected position and allele in forward coordinates of the target read (on '-' the A's read as T's)"""
    t = long_target()
    query = t[:column] + "A" * length + t[column:]
    if strand == "+":
        reads, p, allele = [t, query], column - 1, "A" * length
    else:
        # columns column - 1 and column hold bases 150 - column and 149 - column of the target read
        reads, p, allele = [PC.rc(t), query], 150 - 1 - column, "T" * length
    o = np.array([(1, 0, 0, 0, len(query), 150, ord(strand), 0, 0)], O.OVERLAP)
    return reads, o, p, allele
