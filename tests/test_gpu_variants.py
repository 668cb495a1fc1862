"""Variant calling on the device (tests/oracle_variants.py is the oracle). The expected
records are the CIGAR formulation of the oracle applied to what align_overlaps() returns on the device for the same
records, so the aligner's tie-breaks cannot make a test pass or fail, and the comparison is exact: the cases worked out
on paper (their literal records asserted too) with the thresholds at their edges and the ties, insertion runs around
the tile boundary and at the longest allele, every record of the mapped small case, independence of chunking, order and
repetition, the empty cases, polisher.call_variants with format_vcf, and the refusals."""
import numpy as np
import pytest

import oracle_mapper as O
import oracle_pileup as OPi
import oracle_polish as OPo
import oracle_variants as OV
import pileup_cases as PC
import variant_cases as VC

pytestmark = pytest.mark.gpu

INSERTION = PC.CHANNELS.index("insertion")


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


def by_cigar(cm, o, queries, targets=None):
    """the oracle's alignments of the CIGAR formulation: the device's own CIGARs of the records"""
    cigars, _ = cm.align_overlaps(o, queries, targets)
    return OPi.of_cigars(cigars)


@pytest.fixture(scope="module")
def polishing(cm):
    """the small case against two 3 % drafts of its genome, mapped on the device: reads, drafts, overlaps, alignments"""
    reads, genome = OPo.small_case()
    drafts = [OPo.draft_of(genome, 0.03, OPo.SMALL["seed"]), PC.rc(OPo.draft_of(genome, 0.03, 5))]
    o = cm.map_reads_batched(reads, drafts, rescue_overlap_ends=True, **OPo.MAPPING)
    assert len(o) >= 30 and {chr(s) for s in o["relative_strand"]} == {"+", "-"}
    assert set(o["target_read_id"].tolist()) == {0, 1}
    return reads, drafts, o, by_cigar(cm, o, reads, drafts)


@pytest.mark.parametrize("name", VC.NAMES)
def test_hand_cases(cm, name):
    """literal records: SNV, deleted base and inserted AA on both strands, the thresholds at their edges, the ties"""
    reads, o, min_count, min_percent, want = VC.case(name)
    timings = {}
    got, piles = cm.overlap_variants(o, reads, None, min_count, min_percent, timings=timings, return_pileup=True)
    assert got.dtype == cm.VARIANT == OV.VARIANT
    oracle = OV.overlap_variants(o, reads, None, by_cigar(cm, o, reads), "cigar", min_count, min_percent)
    assert VC.same_records(got, oracle), (got.tolist(), oracle.tolist())
    assert VC.same_records(got, want), (got.tolist(), want.tolist())
    assert not got.view(np.uint8).reshape(-1, 32)[:, 20:24].any()  # the reserved bytes
    assert PC.same(piles, cm.overlap_pileup(o, reads))
    assert VC.same_records(cm.overlap_variants(o, reads, reads, min_count, min_percent), got)
    assert all(timings[k] > 0 for k in ("gather", "align", "pileup", "call"))
    assert timings["bytes_to_host"] == o.nbytes + 32 * len(got) + 24 * sum(len(r) for r in reads)
    if name in VC.INSERTION_CHANNEL:  # the count is the allele's, not the insertion channel's
        p, n = VC.INSERTION_CHANNEL[name]
        assert piles[0][INSERTION, p] == n and got[0]["count"] < n and cm.insertion_allele(got[0]["length"], got[0]["key"]) == "A"


RUNS = ((62, 5), (63, 5), (64, 5), (65, 5), (50, 32), (50, 33), (10, 32), (118, 32), (127, 2), (128, 2))


@pytest.mark.parametrize("strand", "+-")
def test_runs_around_the_tile_boundary_and_the_longest_allele(cm, strand):
    """Runs that begin in columns 62 to 65 and cross into the second tile, runs of exactly 32 bases within a tile and
    across the boundaries at 64 and 128, and one of 33 bases, which the pileup counts and nobody calls. One read each,
    so min_count = 1 calls whatever has a record."""
    for column, length in RUNS:
        reads, o, p, allele = VC.run_case(column, length, strand)
        cigars, _ = cm.align_overlaps(o, reads)
        assert cigars == ["%dM%dD%dM" % (column, length, 150 - column)]
        got, piles = cm.overlap_variants(o, reads, None, 1, 0, return_pileup=True)
        assert VC.same_records(got, OV.overlap_variants(o, reads, None, OPi.of_cigars(cigars), "cigar", 1, 0))
        assert piles[0][INSERTION].nonzero()[0].tolist() == [p] and piles[0][INSERTION, p] == 1
        if length <= 32:
            ref = int(OPi.CHANNEL_OF[ord(reads[0][p])])
            assert VC.same_records(got, VC.rows((0, p, 1, 1, OV.INSERTION, ref, 0, length, OV.pack_key(allele))))
            assert cm.insertion_allele(got[0]["length"], got[0]["key"]) == allele
        else:
            assert len(got) == 0
    # all of them in one call: every read is its own alignment, the 32-base runs at one cell are one allele
    t = VC.long_target()
    queries = [t[:c] + "A" * n + t[c:] for c, n in RUNS]
    reads = [t if strand == "+" else PC.rc(t)] + queries
    o = np.array([(1 + i, 0, 0, 0, len(q), 150, ord(strand), 0, 0) for i, q in enumerate(queries)], O.OVERLAP)
    got = cm.overlap_variants(o, reads, None, 1, 0)
    assert VC.same_records(got, OV.overlap_variants(o, reads, None, by_cigar(cm, o, reads), "cigar", 1, 0))
    assert len(got) == len({c for c, n in RUNS if n <= 32}) and got["depth"].tolist() == [len(RUNS)] * len(got)
    assert sorted(got["count"].tolist()) == [1] * len(got)
    # runs in the first and in the last column of an alignment are counted nowhere
    reads, o, _, _, _ = VC.case("runs_at_both_ends" if strand == "+" else "runs_at_both_ends_reverse")
    got, piles = cm.overlap_variants(o, reads, None, 1, 0, return_pileup=True)
    assert len(got) == 0 and not piles[0][INSERTION].any()


def test_every_record_of_the_polishing_case(cm, polishing):
    reads, drafts, o, alignments = polishing
    everything, piles = cm.overlap_variants(o, reads, drafts, 1, 0, return_pileup=True)
    want = OV.overlap_variants(o, reads, drafts, alignments, "cigar", 1, 0)
    assert VC.same_records(everything, want)
    assert all((everything["kind"] == k).any() for k in range(3))
    assert PC.same(piles, cm.overlap_pileup(o, reads, drafts))
    assert piles[0].base is not None and piles[0].base is piles[1].base  # views of the one copied buffer
    # every supported difference is a record
    for ti, (pile, draft) in enumerate(zip(piles, drafts)):
        own = OPi.CHANNEL_OF[np.frombuffer(draft.encode(), np.uint8)]
        others = pile[:4].sum(0) - pile[own, np.arange(len(draft))]
        of_target = everything[everything["target_read"] == ti]
        assert of_target[of_target["kind"] == OV.SNV]["position"].tolist() == others.nonzero()[0].tolist()
        assert of_target[of_target["kind"] == OV.DELETION]["position"].tolist() == pile[4].nonzero()[0].tolist()
    timings = {}
    defaults = cm.overlap_variants(o, reads, drafts, timings=timings)
    assert VC.same_records(defaults, OV.overlap_variants(o, reads, drafts, alignments, "cigar", 3, 30))
    assert VC.same_records(defaults, cm.overlap_variants(o, reads, drafts, 3, 30))
    assert 0 < len(defaults) < len(everything) and all((defaults["kind"] == k).any() for k in range(3))
    assert timings["bytes_to_host"] == o.nbytes + defaults.nbytes  # the counters stay on the device
    # read ids that count from 5 and from 3
    shifted = o.copy()
    shifted["query_read_id"] += 5
    shifted["target_read_id"] += 3
    assert VC.same_records(cm.overlap_variants(shifted, reads, drafts, first_query_read_id=5, first_target_read_id=3), defaults)


def test_records_do_not_depend_on_chunking_order_or_repetition(cm, polishing):
    reads, drafts, o, _ = polishing
    ql = o["query_end_position_in_read"].astype(np.int64) - o["query_start_position_in_read"]
    tl = o["target_end_position_in_read"].astype(np.int64) - o["target_start_position_in_read"]
    alone = max(cm.align_bytes_needed(int(a), int(b), int(ql.max())) for a, b in zip(ql, tl))
    # a chunk counts its slices' bases four times and more, so within `alone` bytes so many copies of the records take
    # more than two chunks (as tests/test_gpu_pileup.py sizes them)
    copies = 2 * alone // (4 * int((ql + tl).sum())) + 1
    many = np.tile(o, copies)
    assert 4 * copies * int((ql + tl).sum()) > 2 * alone and copies <= 40
    whole, piles = cm.overlap_variants(many, reads, drafts, return_pileup=True)
    for again in (cm.overlap_variants(many, reads, drafts, max_device_bytes=alone),  # several chunks
                  cm.overlap_variants(many[::-1], reads, drafts),                     # the records in reverse order
                  cm.overlap_variants(many[::-1], reads, drafts, max_device_bytes=alone),
                  cm.overlap_variants(many, reads, drafts)):                          # the call repeated
        assert again.tobytes() == whole.tobytes() and len(whole) > 0
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.overlap_variants(many, reads, drafts, max_device_bytes=alone - 1)
    # k copies of every record: k times the counts, and at min_percent alone the same calls
    once = cm.overlap_variants(o, reads, drafts, 1, 30)
    scaled = cm.overlap_variants(many, reads, drafts, 1, 30)
    assert copies > 1 and len(once) == len(scaled) > 0
    for field in OV.VARIANT.names:
        times = copies if field in ("count", "depth") else 1
        assert (scaled[field] == times * once[field]).all(), field
    # forty copies of one record of the cases on paper
    for name in ("insertion_of_two", "three_kinds_reverse"):
        case_reads, case_o, _, _, _ = VC.case(name)
        one = cm.overlap_variants(case_o, case_reads, None, 1, 0)
        forty = cm.overlap_variants(np.tile(case_o, 40), case_reads, None, 1, 0)
        assert len(one) > 0 and forty["count"].tolist() == (40 * one["count"]).tolist()
        assert forty["depth"].tolist() == (40 * one["depth"]).tolist()
        for field in ("target_read", "position", "kind", "ref", "alt", "length", "key"):
            assert forty[field].tolist() == one[field].tolist()


def test_empty_cases(cm):
    reads = PC.reads()
    empty = np.array([(1, 0, 3, 4, 3, 4, ord("-"), 0, 0)], O.OVERLAP)  # two empty slices
    for o in (empty, empty[:0]):
        for kw in (dict(), dict(min_count=1, min_percent=0)):
            got, piles = cm.overlap_variants(o, reads[1:], reads[:1], return_pileup=True, **kw)
            assert got.dtype == cm.VARIANT and got.shape == (0,)
            assert [p.shape for p in piles] == [(6, len(reads[0]))] and not piles[0].any() and piles[0].dtype == np.uint32
            assert cm.overlap_variants(o, reads, **kw).shape == (0,)
    # an empty target set
    timings = {}
    got, piles = cm.overlap_variants(empty[:0], reads, [], timings=timings, return_pileup=True)
    assert got.shape == (0,) and piles == [] and timings["bytes_to_host"] == 0 and timings["call"] == 0
    got, piles = cm.overlap_variants(empty[:0], [], return_pileup=True)
    assert got.shape == (0,) and piles == []
    # records whose alignments hold nothing to call
    o = PC.records(["mismatch"])
    assert cm.overlap_variants(o, reads).shape == (0,)                         # one read is below min_count = 3
    assert len(cm.overlap_variants(o, reads, None, 1, 0)) == 1


def test_call_variants_end_to_end_and_the_vcf(cm, polishing):
    from genomeworks_amd import polisher
    reads, drafts, o, _ = polishing
    want = OV.call_variants(reads, drafts, o, lambda kept: by_cigar(cm, kept, reads, drafts))
    timings = {}
    got = polisher.call_variants(reads, drafts, overlaps=o, timings=timings)
    assert got == want and len(got) > 10 and timings["call"] > 0
    assert {v["kind"] for v in got} == {"snv", "deletion", "insertion"}
    kept = o[OPi.one_overlap_per_read(o)]
    assert sum(len(v["ref"]) for v in got if v["kind"] == "deletion") == (cm.overlap_variants(kept, reads, drafts)["kind"] == 1).sum()
    for v in got:
        assert 0 <= v["count"] <= v["depth"] <= len(reads)  # a read speaks once
        if v["kind"] != "insertion":
            assert drafts[v["target"]][v["position"]:v["position"] + len(v["ref"])] == v["ref"]
    names = ["draft", "draft_rc"]
    text = polisher.format_vcf(got, names, drafts)
    parsed, header = OV.parse_vcf(text, names)
    assert header[0] == "##fileformat=VCFv4.2" and header[1:3] == ["##contig=<ID=%s,length=%d>" % (n, len(d))
                                                                    for n, d in zip(names, drafts)]
    order = lambda v: (v["target"], v["position"], OV.KINDS.index(v["kind"]))
    assert sorted(parsed, key=order) == got
    # other thresholds, and mapping first with polish()'s defaults
    everything = polisher.call_variants(reads, drafts, overlaps=o, min_count=1, min_percent=0)
    assert everything == OV.call_variants(reads, drafts, o, lambda kept: by_cigar(cm, kept, reads, drafts), 1, 0)
    assert max(len(v["ref"]) for v in everything if v["kind"] == "deletion") >= 2  # neighbours were joined
    parsed, _ = OV.parse_vcf(polisher.format_vcf(everything, names, drafts), names)
    assert sorted(parsed, key=order) == everything
    mapped = cm.map_reads_batched(reads, drafts[:1], post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0)
    assert polisher.call_variants(reads, drafts[:1]) == OV.call_variants(
        reads, drafts[:1], mapped, lambda kept: by_cigar(cm, kept, reads, drafts[:1]))


def test_refusals(cm, polishing):
    from genomeworks_amd import _native, polisher
    reads, drafts, o, _ = polishing
    want = cm.overlap_variants(o[:6], reads, drafts, 1, 0)
    for bad in (dict(min_count=0), dict(min_percent=-1), dict(min_percent=101)):
        with pytest.raises(ValueError):
            cm.overlap_variants(o, reads, drafts, **bad)
        with pytest.raises(ValueError):
            polisher.call_variants(reads, drafts, overlaps=o, **bad)
    with pytest.raises(TypeError):
        polisher.call_variants(reads, drafts, overlaps=o, k=15)
    # the C API refuses the same before it uploads anything
    L = _native.mapper()
    q, t = cm._read_set_args(reads, drafts)
    records = np.ascontiguousarray(o, cm.OVERLAP)
    for min_count, min_percent, text in ((0, 30, "min_count"), (3, -1, "min_percent"), (3, 101, "min_percent")):
        assert not L.gw_mapper_overlap_variants(cm._p(records), len(records), *q, 0, *t, 0, min_count, min_percent, 0, None)
        assert text in L.gw_mapper_last_error().decode()
    calls = [lambda: cm.overlap_variants(o, reads, drafts, max_device_bytes=-1)]
    for field, value in (("query_read_id", len(reads)), ("target_read_id", 2), ("target_end_position_in_read", 10 ** 7)):
        bad = o.copy()
        bad[2][field] = value
        calls.append(lambda bad=bad: cm.overlap_variants(bad, reads, drafts))
    for call in calls:
        with pytest.raises(cm.MapperError):
            call()
        assert VC.same_records(cm.overlap_variants(o[:6], reads, drafts, 1, 0), want)
