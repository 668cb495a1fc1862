#!/usr/bin/env python3
"""Writes tests/golden/cudamapper_postprocess_vectors.json: known answers of GenomeWorks' cudamapper tests for overlap
post-processing, end rescue, the k-mer helpers and the grouping of reads into indices. Each case names the reference
test it comes from (file:line). Data only, transcribed by hand.

    python tests/golden/make_mapper_postprocess_vectors.py

The grouping cases read tests/golden/cudamapper_data/20_reads.fasta (the reference's data file of that name)."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def ov(q, t, qs, qe, ts, te, strand="+"):
    return dict(query_read_id=q, target_read_id=t, query_start_position_in_read=qs, query_end_position_in_read=qe,
                target_start_position_in_read=ts, target_end_position_in_read=te, relative_strand=strand)


_T = "Test_CudamapperOverlapperTriggered.cu"
POST_PROCESS = [
    dict(source=_T + ":307", expected_count=6,
         overlaps=[ov(20, 22, 1000, 2000, 4000, 5000), ov(20, 22, 2100, 3100, 5100, 6100),
                   ov(55, 90, 1000, 2000, 4000, 5000), ov(55, 90, 2100, 3100, 5100, 6100)]),
    dict(source=_T + ":360", expected_count=5,
         overlaps=[ov(20, 22, 1000, 2000, 4000, 5000), ov(20, 22, 2100, 3100, 5100, 6100),
                   ov(55, 90, 1000, 2000, 4000, 5000), ov(55, 91, 2100, 3100, 5100, 6100)]),
    dict(source=_T + ":413", expected_count=6,
         overlaps=[ov(20, 22, 1000, 2000, 4000, 5000), ov(20, 22, 2100, 3100, 5100, 6100),
                   ov(55, 90, 1000, 2000, 4000, 5000, "-"), ov(55, 90, 2100, 3100, 2900, 3900, "-")]),
]

_QUERY = (
    "ACCGCCACCAATATCCATGTGACC"
    "TCGCACGGTACGGAATTTACCCTACAAACCCCAACCGGTAGCGTCGATGTTCTGCTGCCGTTGCCGGGGCGTCACAATATTGCGAATGCGCTGGCA"
    "GCCGCTGCGCTCTCCATGTCCGTGGGCGCAACGCTTGATGCTATCAAAGCGGGGCTGGCA"
    "AATCTGAAAGCTGTTCCAGGCCGTCTGTTCCCCATCCAACTGGCAGAAAACCAGTTGCTG"
    "CTCGACGACTCCTACAACGCCAATGTCGGTTCAATGACTGCAGCAGTCCAGGTACTGGCT"
    "GAAATGCCGGGCTACCGCGTGCTGGTGGTGGGCGATATGGCGGAACTGGGCGCTGAAAGC"
    "GAAGCCTGCCATGTACAGGTGGGCGAGGCGGCAAAAGCTGCTGGTATTGACCGCGTGTTA"
    "AGCGTGGGTAAACAAAGCCATGCTATCAGCACCGCCAGCGGCGTTGGCGAACATTTTGCT"
    "GATAAAACTGCGTTAATTACGCGTCTTAAATTACTGATTGCTGAGCAACAGGTAATTACG"
    "ATTTTAGTTAAGGGTTCACGTAGTGCCGCCATGGAAGAGGTAGTACGCGCTTTACAGGAG"
    "AATGGGACATGTTAGTTTGGCTGGCCGAACATTTGGTCAAATATTATTCCGGCTTTAACG"
    "TCTTTTCCTATCTGACGTTTCGCGCCATCGTCAGCCTGCTGACCGCGCTGTTCATCTCAT"
    "TGTGGATGGGCCCGCGTATGATTGCTCATTTGCAAAAACTTTCCTTTGGTCAGGTGGTGC"
    "GTAACGACGGTCCTGAATCACACTTCAGCAAGCGCGGTACGCCGACCATGGGCGGGATTA"
    "TGATCCTGACGGCGATTGTGATCTCCGTACTGCTGTGGGCTTACCCGTCCAATCCGTACG"
    "TCTGGTGCGTGTTGGTGGTGCTGGTAGGTTACGGTGTTATTGGCTTTGTTGATGATTATC"
    "GCAAAGTGGTGCGTAAAGACACCAAAGGGTTGATCGCTCG")
_TARGET = (
    "CAACAACGACATCGGTGTACCGA"
    "TGACGCTGTTGCGCTTAACGCCGGAATACGATTACGC"
    "AGTTATTGAACTTGGCGCGAACCATCAGGGCGAAATAGCCTGGACTGTGAGTCTGACTCG"
    "CCCGGAAGCTGCGCTGGTCAACAACCTGGCAGCGGCGCATCTGGAAGGTTTTGGCTCGCT"
    "TGCGGGTGTCGCGAAAGCGAAAGGTGAAATCTTTAGCGGCCTGCCGGAAAACGGTATCGC"
    "CATTATGAACGCCGACAACAACGACTGGCTGAACTGGCAGAGCGTAATTGGCTCACGCAA"
    "AGTGTGGCGTTTCTCACCCAATGCCGCCAACAGCGATTTCACCGCCACCAATATCCATGT"
    "GACCTCGCACGGTACGGAATTTACCCTACAAACCCCAACCGGTAGCGTCGATGTTCTGCT"
    "GCCGTTGCCGGGGCGTCACAATATTGCGAATGCGCTGGCAGCCGCTGCGCTCTCCATGTC"
    "CGTGGGCGCAACGCTTGATGCTATCAAAGCGGGGCTGGCAAATCTGAAAGCTGTTCCAGG"
    "CCGTCTGTTCCCCATCCAACTGGCAGAAAACCAGTTGCTGCTCGACGACTCCTACAACGC"
    "CAATGTCGGTTCAATGACTGCAGCAGTCCAGGTACTGGCTGAAATGCCGGGCTACCGCGT"
    "GCTGGTGGTGGGCGATATGGCGGAACTGGGCGCTGAAAGCGAAGCCTGCCATGTACAGGT"
    "GGGCGAGGCGGCAAAAGCTGCTGGTATTGACCGCGTGTTAAGCGTGGGTAAACAAAGCCA"
    "TGCTATCAGCACCGCCAGCGGCGTTGGCGAACATTTTGCTGATAAAACTGCGTTAATTAC"
    "GCGTCTTAAATTACTGATTGCTGAGCAACAGGTAATTACGATTTTAGTTAAGGGTTCACG"
    "TAGTGCCGCCATGGAAGAGGTAGTACGCGCTTTACAGGAGAATGGGACATGTTAGTTTGG"
    "CTGGCCGAACATTTGGTCAAATATTATTCCGGCTTTAACG")

# extend_overlap_by_sequence_similarity: one round
EXTENSION = [
    dict(source="Test_CudamapperOverlapper.cpp:30", query=_QUERY, target=_TARGET, extension=50,
         required_similarity=0.8, overlap=ov(0, 0, 1, 636, 341, 976),
         expected=dict(query_start_position_in_read=0, target_start_position_in_read=340,
                       query_end_position_in_read=660, target_end_position_in_read=1000)),
]

DROP_BY_MASK = [
    dict(source="Test_CudamapperOverlapper.cpp:86", query_read_ids=[1, 2, 3, 4, 5],
         mask=[True, False, True, True, False], expected_query_read_ids=[2, 5]),
    dict(source="Test_CudamapperOverlapper.cpp:106", query_read_ids=[], mask=[], expected_query_read_ids=[]),
]

_K = "Test_CudamapperUtilsKmerFunctions.cpp"
KMERS = [
    dict(source=_K + ":31", sequence="AAACCTTCTCT", kmer_size=4, stride=1, expected_count=8, expected_first="AAAC",
         expected_last="CTCT"),
    dict(source=_K + ":42", sequence="", kmer_size=4, stride=1, expected_count=1, expected_first="", expected_last=""),
]
SHARED = [
    dict(source=_K + ":50", a=[1, 2, 5, 10, 1000, 10000], b=[1, 3, 5, 10, 20000], expected=3),
    dict(source=_K + ":58", a=["A", "AA", "BET", "CAT"], b=["A", "B", "BEST", "BET", "cat", "CAT", "CHAT"], expected=3),
    dict(source=_K + ":68", a=[], b=[], expected=0),
    dict(source=_K + ":68", a=[], b=[1], expected=0),
]
SIMILARITY = [
    dict(source=_K + ":79", a="AAACCTATGAGGG", b="AAACCTATGAGGG", kmer_size=4, stride=1, expected="== 1"),
    dict(source=_K + ":87", a="AAACCTATGAGGG", b="CCCAATTTAAATT", kmer_size=4, stride=1, expected="== 0"),
    dict(source=_K + ":94", a="AAACCTATGAGGG", b="AAACCTAAGAGGG", kmer_size=4, stride=1, expected="between 0 and 1"),
]

_D = "Test_CudamapperIndexDescriptor.cpp"
GROUPING = [
    dict(source=_D + ":90", fasta="20_reads.fasta", max_basepairs_per_index=10,
         expected=[[0, 2], [2, 1], [3, 2], [5, 1], [6, 2], [8, 2], [10, 2], [12, 3], [15, 2], [17, 2], [19, 1]]),
    dict(source=_D + ":126", fasta="20_reads.fasta", max_basepairs_per_index=7,
         expected=[[0, 1], [1, 1], [2, 1], [3, 2], [5, 1], [6, 1], [7, 2], [9, 1], [10, 1], [11, 2], [13, 1], [14, 2],
                   [16, 1], [17, 1], [18, 2]]),
]

if __name__ == "__main__":
    out = os.path.join(HERE, "cudamapper_postprocess_vectors.json")
    with open(out, "w") as f:
        json.dump(dict(post_process=POST_PROCESS, extension=EXTENSION, drop_by_mask=DROP_BY_MASK, kmers=KMERS,
                       shared=SHARED, similarity=SIMILARITY, grouping=GROUPING), f, indent=1)
        f.write("\n")
    print("wrote", out)
