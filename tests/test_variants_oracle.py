"""Variant calling without a GPU: the two formulations of the oracle agree on the cases
worked out on paper, whose literal records both give, and on the mapped small case against its 3 % drafts; key packing
and cudamapper.insertion_allele; the joining of deleted neighbours and the literal text of polisher.format_vcf; the
public surface (the record type, the exported symbols, a C99 caller of the two headers, the source list of the build)
and the refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_pileup as OPi
import oracle_polish as OPo
import oracle_variants as OV
import pileup_cases as PC
import variant_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import build, cudamapper
    build.build_mapper()
    return cudamapper


@pytest.fixture(scope="module")
def polished():
    """the small case against two 3 % drafts, one reverse-complemented: reads, drafts, the oracle's overlaps, alignments"""
    reads, genome = OPo.small_case()
    drafts = [OPo.draft_of(genome, 0.03, OPo.SMALL["seed"]), PC.rc(OPo.draft_of(genome, 0.03, 5))]
    o = OPo.mapped_overlaps(reads, drafts)
    assert len(o) >= 30 and set(o["target_read_id"].tolist()) == {0, 1}
    return reads, drafts, o, OA.alignments(o, reads, drafts)


@pytest.mark.parametrize("name", VC.NAMES)
def test_hand_cases(name):
    reads, o, min_count, min_percent, want = VC.case(name)
    alignments = OA.alignments(o, reads)
    by_cigar, piles = OV.overlap_variants(o, reads, None, alignments, "cigar", min_count, min_percent, return_pileup=True)
    by_states = OV.overlap_variants(o, reads, None, alignments, "states", min_count, min_percent)
    assert VC.same_records(by_cigar, by_states)
    assert VC.same_records(by_cigar, want), (by_cigar.tolist(), want.tolist())
    if name in VC.INSERTION_CHANNEL:
        p, n = VC.INSERTION_CHANNEL[name]
        assert piles[0][OPi.INSERTION, p] == n and by_cigar[0]["count"] < n


def test_hand_cases_are_what_their_comments_say():
    cigars = {}
    for name in ("snv", "deleted_base", "insertion_of_two", "insertion_of_two_reverse", "allele_tie_shorter",
                 "allele_tie_key_reverse", "runs_at_both_ends"):
        reads, o, _, _, _ = VC.case(name)
        cigars[name] = [a["cigar"] for a in OA.alignments(o, reads)]
    assert cigars == {"snv": ["12M"] * 4, "deleted_base": ["5M1I6M"] * 3 + ["12M"],
                      "insertion_of_two": ["6M2D6M"] * 3 + ["12M"],
                      "insertion_of_two_reverse": ["6M2D6M"] * 3 + ["12M"],  # columns 6 and 7 of the reversed target
                      "allele_tie_shorter": ["1M2D11M"] * 2 + ["1M1D11M"] * 3,
                      "allele_tie_key_reverse": ["10M1D2M"] * 4, "runs_at_both_ends": ["2D12M1D"]}
    reads, o, _, _, _ = VC.case("insertion_of_two_reverse")
    assert reads[1] == "G" + PC.rc("CGTGCT" + "AA" + "GTCGTC") + "C" and "TT" in reads[1] and chr(o[0]["relative_strand"]) == "-"


def test_runs_of_every_length_and_the_longest_allele():
    for strand in "+-":
        for column, length in ((62, 5), (63, 5), (64, 5), (65, 5), (50, 32), (50, 33), (10, 32)):
            reads, o, p, allele = VC.run_case(column, length, strand)
            alignments = OA.alignments(o, reads)
            assert alignments[0]["cigar"] == "%dM%dD%dM" % (column, length, 150 - column)
            got, piles = OV.overlap_variants(o, reads, None, alignments, "cigar", 1, 0, return_pileup=True)
            assert VC.same_records(got, OV.overlap_variants(o, reads, None, alignments, "states", 1, 0))
            assert piles[0][OPi.INSERTION].nonzero()[0].tolist() == [p] and piles[0][OPi.INSERTION, p] == 1
            ref = int(OPi.CHANNEL_OF[ord(reads[0][p])])
            want = VC.rows((0, p, 1, 1, OV.INSERTION, ref, 0, length, OV.pack_key(allele))) if length <= 32 else VC.rows()
            assert VC.same_records(got, want), (strand, column, length)


def test_two_formulations_agree_on_the_polishing_case(polished):
    reads, drafts, o, alignments = polished
    for min_count, min_percent in ((1, 0), (3, 30)):
        by_cigar = OV.overlap_variants(o, reads, drafts, alignments, "cigar", min_count, min_percent)
        by_states = OV.overlap_variants(o, reads, drafts, alignments, "states", min_count, min_percent)
        assert VC.same_records(by_cigar, by_states)
        kinds = by_cigar["kind"].tolist()
        assert all(kinds.count(k) > 0 for k in range(3)), (min_count, kinds.count(0), kinds.count(1), kinds.count(2))
        cells = [(int(v["target_read"]), int(v["position"]), int(v["kind"])) for v in by_cigar]
        assert cells == sorted(cells) and len(set(cells)) == len(cells)  # the order, and one record of a kind per cell
        assert set(by_cigar["target_read"].tolist()) == {0, 1}
    # with nothing held back every supported difference is a record: every cell with a count off the target's own base
    everything = OV.overlap_variants(o, reads, drafts, alignments, "cigar", 1, 0)
    piles = OPi.overlap_pileup(o, reads, drafts, alignments, "cigar")
    for ti, (pile, draft) in enumerate(zip(piles, drafts)):
        own = OPi.CHANNEL_OF[np.frombuffer(draft.encode(), np.uint8)]
        others = pile[:4].sum(0) - pile[own, np.arange(len(draft))]
        of_target = everything[everything["target_read"] == ti]
        assert of_target[of_target["kind"] == OV.SNV]["position"].tolist() == others.nonzero()[0].tolist()
        assert of_target[of_target["kind"] == OV.DELETION]["position"].tolist() == pile[4].nonzero()[0].tolist()
        # the pileup counts runs of every length; none of more than 32 bases is in a 3 % draft's alignments
        assert of_target[of_target["kind"] == OV.INSERTION]["position"].tolist() == pile[5].nonzero()[0].tolist()


def test_key_packing_and_insertion_allele(cm):
    assert cm.VARIANT == OV.VARIANT and cm.VARIANT.itemsize == 32
    assert cm.VARIANT_KINDS == OV.KINDS == ("snv", "deletion", "insertion")
    assert OV.pack_key("A") == 0 and OV.pack_key("T") == 3 and OV.pack_key("AC") == 1 and OV.pack_key("CA") == 4
    assert OV.pack_key("ACGT") == 0b00011011
    assert OV.pack_key("T" * 32) == 2 ** 64 - 1
    assert cm.insertion_allele(32, 2 ** 64 - 1) == "T" * 32 and cm.insertion_allele(32, 0) == "A" * 32
    assert cm.insertion_allele(np.uint8(32), np.uint64(2 ** 64 - 1)) == "T" * 32  # the fields of a record
    assert cm.insertion_allele(0, 0) == "" and cm.insertion_allele(4, 0b00011011) == "ACGT"
    rng = np.random.default_rng(32)
    for length in (1, 2, 31, 32):
        alleles = sorted({"".join(rng.choice(list("ACGT"), length)) for _ in range(20)})
        keys = [OV.pack_key(a) for a in alleles]
        assert keys == sorted(keys)  # among alleles of one length, key order is alphabetical order
        assert [cm.insertion_allele(length, k) for k in keys] == alleles == [OV.allele_text(length, k) for k in keys]
    for length, key in ((33, 0), (-1, 0), (1, 4), (0, 1)):
        with pytest.raises(ValueError):
            cm.insertion_allele(length, key)


TARGETS = ["ACGTACGTAC", "GGTCA"]
VCF = """##fileformat=VCFv4.2
##contig=<ID=ctg1,length=10>
##contig=<ID=ctg2,length=5>
##INFO=<ID=DP,Number=1,Type=Integer,Description="Aligned reads that put a base at the position or delete it">
##INFO=<ID=AD,Number=1,Type=Integer,Description="Aligned reads that support the alternative allele">
##INFO=<ID=TYPE,Number=1,Type=String,Description="snv, deletion or insertion">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
ctg1\t1\t.\tACG\tG\t.\tPASS\tDP=9;AD=4;TYPE=deletion
ctg1\t4\t.\tT\tG\t.\tPASS\tDP=10;AD=6;TYPE=snv
ctg1\t6\t.\tC\tCTT\t.\tPASS\tDP=11;AD=5;TYPE=insertion
ctg1\t7\t.\tGTA\tG\t.\tPASS\tDP=12;AD=3;TYPE=deletion
ctg2\t2\t.\tGTC\tG\t.\tPASS\tDP=7;AD=7;TYPE=deletion
ctg2\t3\t.\tT\tA\t.\tPASS\tDP=7;AD=3;TYPE=snv
"""


def test_deletion_joining_and_the_vcf_text(cm):
    from genomeworks_amd import polisher
    records = VC.rows((0, 0, 5, 9, OV.DELETION, 0, 0, 0, 0), (0, 1, 4, 8, OV.DELETION, 1, 0, 0, 0),
                      (0, 3, 6, 10, OV.SNV, 3, 2, 0, 0), (0, 5, 5, 11, OV.INSERTION, 1, 0, 2, OV.pack_key("TT")),
                      (0, 7, 3, 12, OV.DELETION, 3, 0, 0, 0), (0, 8, 4, 13, OV.DELETION, 0, 0, 0, 0),
                      # an SNV in the cell of a deleted base stays a record of its own; another target begins another deletion
                      (1, 2, 3, 7, OV.SNV, 3, 0, 0, 0), (1, 2, 7, 7, OV.DELETION, 3, 0, 0, 0),
                      (1, 3, 8, 8, OV.DELETION, 1, 0, 0, 0))
    joined = polisher.join_deletions(records, TARGETS)
    assert joined == OV.join_deletions(records, TARGETS)
    assert joined == [
        dict(target=0, position=0, kind="deletion", ref="AC", alt="", count=4, depth=9),
        dict(target=0, position=3, kind="snv", ref="T", alt="G", count=6, depth=10),
        dict(target=0, position=5, kind="insertion", ref="", alt="TT", count=5, depth=11),
        dict(target=0, position=7, kind="deletion", ref="TA", alt="", count=3, depth=12),
        dict(target=1, position=2, kind="snv", ref="T", alt="A", count=3, depth=7),
        dict(target=1, position=2, kind="deletion", ref="TC", alt="", count=7, depth=7)]
    assert polisher.join_deletions(records, [t.encode() for t in TARGETS]) == joined
    # the end of one target and the beginning of the next are no neighbours
    ends = VC.rows((0, 9, 3, 3, OV.DELETION, 1, 0, 0, 0), (1, 0, 3, 3, OV.DELETION, 2, 0, 0, 0))
    assert [(v["target"], v["position"], v["ref"]) for v in polisher.join_deletions(ends, TARGETS)] == [(0, 9, "C"), (1, 0, "G")]
    text = polisher.format_vcf(joined, ["ctg1", "ctg2"], TARGETS)
    assert text == VCF
    # a deletion with p > 0 stands in front of an SNV of the same base, which call_variants() lists first
    parsed, header = OV.parse_vcf(text, ["ctg1", "ctg2"])
    assert parsed == joined[:4] + [joined[5], joined[4]] and len(header) == 7
    assert polisher.format_vcf([], ["ctg1", "ctg2"], TARGETS) == "".join(line + "\n" for line in VCF.split("\n")[:7])
    with pytest.raises(ValueError):
        polisher.format_vcf(joined, ["ctg1"], TARGETS)
    with pytest.raises(ValueError):  # a whole target deleted has no base to stand at
        polisher.format_vcf([dict(target=1, position=0, kind="deletion", ref="GGTCA", alt="", count=1, depth=1)],
                            ["ctg1", "ctg2"], TARGETS)


def test_new_c_symbols_are_exported_and_a_caller_compiles(cm, tmp_path):
    C.CDLL(os.path.join(LIB, "libgwhip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIB, "libcudamapper.so"))
    for name in ("gwm_overlap_variants", "gwm_variants_free", "gw_mapper_overlap_variants", "gw_mapper_variants_count",
                 "gw_mapper_variants_copy", "gw_mapper_variants_pileup_copy", "gw_mapper_variants_destroy"):
        assert hasattr(lib, name), name
    for name in ("overlap_variants", "insertion_allele"):
        assert callable(getattr(cm, name)), name
    src = tmp_path / "caller.c"
    src.write_text("""
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    gwm_variants v = {0, 0, {0, 0, {0.f, 0.f, 0.f}}, {0.f, 0.f, 0.f, 0.f}};
    int (*call)(const gwm_overlap*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                const int64_t*, int32_t, uint32_t, int32_t, int32_t, int64_t, void*, gwm_variants*) = gwm_overlap_variants;
    gw_mapper_variants* (*entry)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                                 const int64_t*, int32_t, uint32_t, int32_t, int32_t, int64_t, void*) =
        gw_mapper_overlap_variants;
    int64_t (*count)(const gw_mapper_variants*) = gw_mapper_variants_count;
    int (*copy)(const gw_mapper_variants*, void*, float*) = gw_mapper_variants_copy;
    int (*pileup_copy)(const gw_mapper_variants*, uint32_t*) = gw_mapper_variants_pileup_copy;
    void (*destroy)(gw_mapper_variants*) = gw_mapper_variants_destroy;
    gwm_variants_free(&v); /* a zeroed struct: nothing to free */
    if (!call || !entry || !count || !copy || !pileup_copy || !destroy || v.variants || v.n_variants || v.pileup.counts)
        return 1;
    printf("%d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(gwm_variant), (int)offsetof(gwm_variant, target_read),
           (int)offsetof(gwm_variant, position), (int)offsetof(gwm_variant, count), (int)offsetof(gwm_variant, depth),
           (int)offsetof(gwm_variant, kind), (int)offsetof(gwm_variant, ref), (int)offsetof(gwm_variant, alt),
           (int)offsetof(gwm_variant, length), (int)offsetof(gwm_variant, key));
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
    # the struct is what the VARIANT dtype says
    fields = cm.VARIANT.fields
    assert [int(x) for x in r.stdout.split()] == [cm.VARIANT.itemsize] + [fields[name][1] for name in cm.VARIANT.names]


def test_the_build_names_the_new_source():
    from genomeworks_amd import build
    assert "mapper/gwm_variants.hip" in build.MAPPER_KERNEL_SRCS and "mapper/gwm_pileup.hip" in build.MAPPER_KERNEL_SRCS
    for name in ("gwm_variants.hip", "gwm_pileup_kernel.hpp"):
        assert os.path.exists(os.path.join(ROOT, "genomeworks_amd", "mapper", name))
    # the pileup kernel is defined once, in the header both units include
    for name, defines in (("gwm_pileup_kernel.hpp", True), ("gwm_pileup.hip", False), ("gwm_variants.hip", False)):
        with open(os.path.join(ROOT, "genomeworks_amd", "mapper", name)) as f:
            text = f.read()
        assert ("void __launch_bounds__(kThreads) pileup_kernel(" in text) == defines, name
        assert defines or '#include "gwm_pileup_kernel.hpp"' in text


def test_refusals_need_no_device(cm):
    from genomeworks_amd import polisher
    reads, genome = OPo.small_case()
    empty = np.zeros(0, O.OVERLAP)
    for bad in (dict(min_count=0), dict(min_percent=-1), dict(min_percent=101)):
        with pytest.raises(ValueError):
            cm.overlap_variants(empty, reads, [genome], **bad)
        with pytest.raises(ValueError):
            polisher.call_variants(reads, [genome], overlaps=empty, **bad)
    with pytest.raises(ValueError):
        polisher.call_variants(reads + ["ACGT"], [genome])
    with pytest.raises(ValueError):
        polisher.call_variants(reads, ["ACGT"])
    with pytest.raises(ValueError):
        polisher.call_variants(reads, [genome], align=True)
    with pytest.raises(TypeError):
        polisher.call_variants(reads, [genome], overlaps=empty, k=15)
