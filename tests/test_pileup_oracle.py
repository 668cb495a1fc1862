"""Pileups without a GPU: the two formulations of both roles agree cell for cell on the
mapped small cases, the cases worked out on paper through both of them, the depth invariant, the public surface (the
exported symbols, a C99 caller of the two headers, the source list of the build) and the refusals of polisher.pileup
and read_pileup that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_correct as OC
import oracle_mapper as O
import oracle_mapper_align as OA
import oracle_pileup as OPi
import oracle_polish as OPo
import pileup_cases as PC

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
    """the small case against a 3 % draft: reads, draft, the oracle's overlaps and their alignments"""
    reads, genome = OPo.small_case()
    draft = OPo.draft_of(genome, 0.03, OPo.SMALL["seed"])
    o = OPo.mapped_overlaps(reads, [draft])
    assert len(o) >= 20 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    return reads, draft, o, OA.alignments(o, reads, [draft])


@pytest.fixture(scope="module")
def corrected():
    """the small case mapped against itself as two sets, self overlaps and both directions included: reads, the records
    and their alignments"""
    reads, _ = OPo.small_case()
    o = OC.mapped_all_against_all(reads)
    assert (o["query_read_id"] == o["target_read_id"]).sum() == len(reads)
    assert {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    return reads, o, OA.alignments(o, reads)


def test_channels_follow_the_aligners_folding():
    assert OPi.CHANNELS == PC.CHANNELS == ("A", "C", "G", "T", "deletion", "insertion")
    assert [int(OPi.CHANNEL_OF[ord(c)]) for c in "ACGTacgt"] == [0, 1, 2, 3, 0, 1, 2, 3]
    # the complement of channel k is 3 - k, and it is the channel of the aligner's complement table
    for c in range(256):
        assert 3 - OPi.CHANNEL_OF[c] == OPi.CHANNEL_OF[OA.COMPLEMENT[c]]
    assert int(OPi.CHANNEL_OF[ord("N")]) == 2  # other bytes count as what the aligner folds them to


def test_two_formulations_agree_on_the_polishing_case(polished):
    reads, draft, o, alignments = polished
    by_states = OPi.overlap_pileup(o, reads, [draft], alignments)
    by_cigar = OPi.overlap_pileup(o, reads, [draft], alignments, "cigar")
    assert PC.same(by_states, by_cigar)
    pile = by_states[0]
    assert pile.shape == (6, len(draft)) and pile.dtype == np.uint32
    assert all(pile[c].sum() > 0 for c in range(6))  # every channel is used
    # the depth invariant: channels 0..4 sum to the records whose target slice covers the position
    assert np.array_equal(OPi.depth(pile), OPi.covering(o, [draft], False, alignments)[0])
    assert OPi.depth(pile).max() >= 8
    # most of the reads agree with most of the draft
    best = pile[:4].argmax(0)
    agree = best == OPi.CHANNEL_OF[np.frombuffer(draft.encode(), np.uint8)]
    assert agree[OPi.depth(pile) >= 4].mean() > 0.9


def test_two_formulations_agree_on_the_correction_case(corrected):
    reads, o, alignments = corrected
    for roles in ((False, True), (False,), (True,)):
        by_states = OPi.pair_pileup(o, reads, alignments, roles=roles)
        by_cigar = OPi.pair_pileup(o, reads, alignments, "cigar", roles=roles)
        assert PC.same(by_states, by_cigar), roles
    both = OPi.pair_pileup(o, reads, alignments)
    target_role = OPi.pair_pileup(o, reads, alignments, roles=(False,))
    query_role = OPi.pair_pileup(o, reads, alignments, roles=(True,))
    assert PC.same(both, [a + b for a, b in zip(target_role, query_role)])
    assert PC.same(target_role, OPi.overlap_pileup(o, reads, reads, alignments))
    # the depth invariant in either role, self overlaps and '-' records included
    for role, piles in ((False, target_role), (True, query_role)):
        for pile, want in zip(piles, OPi.covering(o, reads, role, alignments)):
            assert np.array_equal(OPi.depth(pile), want)
    # a read's overlap with itself supports every base as it is, in both roles
    same = o[o["query_read_id"] == o["target_read_id"]]
    piles = OPi.pair_pileup(same, reads)
    for pile, r in zip(piles, reads):
        own = np.zeros((6, len(r)), np.uint32)
        own[OPi.CHANNEL_OF[np.frombuffer(r.encode(), np.uint8)], np.arange(len(r))] = 2
        assert np.array_equal(pile, own)


@pytest.mark.parametrize("formulation", ["states", "cigar"])
@pytest.mark.parametrize("name", PC.NAMES)
def test_hand_cases(name, formulation):
    reads, o = PC.reads(), PC.records([name])
    assert PC.same(OPi.overlap_pileup(o, reads, reads, None, formulation), PC.expected([name], (False,)))
    assert PC.same(OPi.pair_pileup(o, reads, None, formulation), PC.expected([name]))
    assert PC.same(OPi.pair_pileup(o, reads, None, formulation, roles=(True,)), PC.expected([name], (True,)))


def test_hand_cases_are_what_their_comments_say():
    reads, alignments = PC.reads(), OA.alignments(PC.records(PC.NAMES), PC.reads())
    cigars = dict(zip(PC.NAMES, (a["cigar"] for a in alignments)))
    assert cigars == {"mismatch": "12M", "deleted_target_base": "5M1I6M", "insertion_of_two": "6M2D6M",
                      "runs_at_both_ends": "2D12M1D", "mismatch_reverse": "12M", "insertion_reverse": "4M2D8M",
                      "deleted_target_base_reverse": "5M1I6M", "runs_at_both_ends_reverse": "1D12M2D"}
    assert PC.rc(PC.T) == PC.RC and len(reads) == 1 + len(PC.NAMES)


@pytest.mark.parametrize("formulation", ["states", "cigar"])
def test_records_count_as_given(formulation):
    reads = PC.reads()
    names = ["insertion_of_two", "insertion_of_two", "mismatch_reverse", "insertion_of_two"]
    got = OPi.pair_pileup(PC.records(names), reads, None, formulation)
    assert PC.same(got, PC.expected(names))
    assert got[0][PC.CHANNELS.index("insertion"), PC.TS + 5] == 3 and OPi.depth(got[0])[PC.TS:PC.TS + 12].tolist() == [4] * 12
    # two empty slices, and no records at all: nothing
    empty = np.array([(1, 0, 3, 4, 3, 4, ord("-"), 0, 0)], O.OVERLAP)
    for o in (empty, empty[:0]):
        assert all(not p.any() for p in OPi.pair_pileup(o, reads, None, formulation))


def test_the_pipelines_keep_the_records_polish_and_correct_reads_align(polished, corrected):
    reads, draft, o, alignments = polished
    kept = OPi.one_overlap_per_read(o)
    assert len(kept) == len(set(o["query_read_id"].tolist())) <= len(o)
    # the kept records are aligned as a call of their own: its longest query slice may differ from the whole call's
    got = OPi.pileup(reads, [draft], o)
    assert PC.same(got, OPi.overlap_pileup(o[kept], reads, [draft]))
    assert OPi.depth(got[0]).max() <= len(reads)  # a read speaks once
    reads, o, alignments = corrected
    pairs = OC.select_pairs(o)
    # the pairs' alignments within a call of their own: the longest query slice of the call may differ
    assert PC.same(OPi.read_pileup(reads, o), OPi.pair_pileup(o[pairs], reads))
    same = o[o["query_read_id"] == o["target_read_id"]]
    assert all(not p.any() for p in OPi.read_pileup(reads, same))


def test_new_c_symbols_are_exported_and_a_caller_compiles(cm, tmp_path):
    C.CDLL(os.path.join(LIB, "libgwhip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIB, "libcudamapper.so"))
    for name in ("gwm_overlap_pileup", "gwm_pair_pileup", "gwm_pileup_free", "gw_mapper_overlap_pileup",
                 "gw_mapper_pair_pileup", "gw_mapper_pileup_bases", "gw_mapper_pileup_copy", "gw_mapper_pileup_destroy"):
        assert hasattr(lib, name), name
    for name in ("overlap_pileup", "pair_pileup"):
        assert callable(getattr(cm, name)), name
    assert cm.PILEUP_CHANNELS == PC.CHANNELS
    src = tmp_path / "caller.c"
    src.write_text("""
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"
#include <stdio.h>
int main(void)
{
    gwm_pileup p = {0, 0, {0.f, 0.f, 0.f}};
    int (*overlap)(const gwm_overlap*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                   const int64_t*, int32_t, uint32_t, int64_t, void*, gwm_pileup*) = gwm_overlap_pileup;
    int (*pair)(const gwm_overlap*, int64_t, const char*, const int64_t*, int32_t, uint32_t, int64_t, void*,
                gwm_pileup*) = gwm_pair_pileup;
    gw_mapper_pileup* (*overlap_entry)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, const char*,
                                       const int64_t*, int32_t, uint32_t, int64_t, void*) = gw_mapper_overlap_pileup;
    gw_mapper_pileup* (*pair_entry)(const void*, int64_t, const char*, const int64_t*, int32_t, uint32_t, int64_t,
                                    void*) = gw_mapper_pair_pileup;
    int64_t (*bases)(const gw_mapper_pileup*) = gw_mapper_pileup_bases;
    int (*copy)(const gw_mapper_pileup*, uint32_t*, float*) = gw_mapper_pileup_copy;
    void (*destroy)(gw_mapper_pileup*) = gw_mapper_pileup_destroy;
    gwm_pileup_free(&p); /* a zeroed struct: nothing to free */
    if (!overlap || !pair || !overlap_entry || !pair_entry || !bases || !copy || !destroy || p.counts || p.n_bases)
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


def test_the_build_names_the_new_source():
    from genomeworks_amd import build
    assert "mapper/gwm_pileup.hip" in build.MAPPER_KERNEL_SRCS
    assert not any(s.startswith("csrc/") for s in build.MAPPER_KERNEL_SRCS + build.MAPPER_HOST_SRCS)
    assert os.path.exists(os.path.join(ROOT, "genomeworks_amd", "mapper", "gwm_pileup.hip"))


def test_pileup_refusals_need_no_device():
    from genomeworks_amd import polisher
    reads, genome = OPo.small_case()
    empty = np.zeros(0, O.OVERLAP)
    with pytest.raises(ValueError):
        polisher.pileup(reads + ["ACGT"], [genome])
    with pytest.raises(ValueError):
        polisher.pileup(reads, ["ACGT"])
    with pytest.raises(ValueError):
        polisher.read_pileup(reads + ["ACGT"])
    with pytest.raises(ValueError):
        polisher.pileup(reads, [genome], align=True)
    with pytest.raises(ValueError):
        polisher.read_pileup(reads, align=True)
    with pytest.raises(TypeError):
        polisher.pileup(reads, [genome], overlaps=empty, k=15)
    with pytest.raises(TypeError):
        polisher.read_pileup(reads, overlaps=empty, w=10)
    pile = np.arange(12, dtype=np.uint32).reshape(6, 2)
    assert polisher.depth(pile).tolist() == [0 + 2 + 4 + 6 + 8, 1 + 3 + 5 + 7 + 9]
