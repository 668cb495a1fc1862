"""cudamapper.extend_overlaps on the device against tests/oracle_mapper_extend.py: records,
extensions and scores byte for byte, whatever the chunking, and align_overlaps() on the extended records."""
import numpy as np
import pytest

import cigar_replay
import mapper_extend_cases as cases
import oracle_mapper_extend as OM

pytestmark = pytest.mark.gpu

EXTENSION = (2, 4, 4, 2, 64, 200)


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def exact():
    """error-free reads pulled in by 50 and by 120 bases per end, and what the oracle makes of them, computed once"""
    reads, drafts, records, truth = cases.case(11)
    return reads, drafts, records, truth, OM.extend_overlaps(records, reads, drafts, EXTENSION, 1024)


@pytest.fixture(scope="module")
def noisy():
    """the same with 5 % errors in the reads and 60 unrelated bases on either side of each"""
    reads, drafts, records, truth = cases.case(12, read_error=0.05, tail=60)
    return reads, drafts, records, truth, OM.extend_overlaps(records, reads, drafts, EXTENSION, 1024)


def same_records(got, want):
    """field by field: the three padding bytes of a record hold nothing"""
    assert got.dtype == want.dtype and got.shape == want.shape
    for name in want.dtype.names:
        assert got[name].tobytes() == want[name].tobytes(), name


def same(got, want):
    same_records(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def test_the_oracle_restores_every_original_end_and_the_device_equals_it(cm, exact):
    reads, drafts, records, truth, want = exact
    assert {chr(s) for s in records["relative_strand"]} == {"+", "-"} and len(records) == 12
    for x, ends in zip(want[0], truth):  # on the CPU
        assert (x["query_start_position_in_read"], x["query_end_position_in_read"], x["target_start_position_in_read"],
                x["target_end_position_in_read"]) == ends
    assert sorted(set(want[1].ravel().tolist())) == [50, 120] and sorted(set(want[2].ravel().tolist())) == [100, 240]
    got = cm.extend_overlaps(records, reads, drafts, extension=EXTENSION)
    same(got, want)
    for name in ("query_read_id", "target_read_id", "relative_strand", "num_residues", "overlap_complete"):
        assert got[0][name].tobytes() == records[name].tobytes()
    same(cm.extend_overlaps(records, reads, drafts), want)  # the defaults are EXTENSION and 1024
    same(cm.extend_overlaps(records, reads, drafts, extension=dict(band=64, xdrop=200)), want)


def test_errors_and_unrelated_tails(cm, noisy):
    reads, drafts, records, truth, want = noisy
    got = cm.extend_overlaps(records, reads, drafts, extension=EXTENSION)
    same(got, want)
    gained = want[1]
    assert (gained > 0).all() and (gained < 120 + 60).all()  # every end moved, none ran through its unrelated tail
    for B, X, M in ((7, 20, 1024), (128, -1, 100), (0, 0, 30)):
        same(cm.extend_overlaps(records, reads, drafts, extension=(2, 4, 4, 2, B, X), max_extension=M),
             OM.extend_overlaps(records, reads, drafts, (2, 4, 4, 2, B, X), M))


def test_chunking_does_not_change_the_result(cm, noisy):
    reads, drafts, records, truth, want = noisy
    # a chunk of m overlaps counts its gathered bases + 90 m + 1 360 bytes (include/gwhip_mapper.h)
    M, t = 300, len(drafts[0])
    bases = [min(M, int(x["query_start_position_in_read"])) + min(M, len(reads[k]) - int(x["query_end_position_in_read"])) +
             min(M, int(x["target_start_position_in_read"])) + min(M, t - int(x["target_end_position_in_read"]))
             for k, x in enumerate(records)]
    cost = lambda first, m: sum(bases[first:first + m]) + 90 * m + 1360
    one, two = 2500, 3300
    assert all(cost(k, 1) <= one < cost(k, 2) for k in range(11)) and cost(11, 1) <= one  # one overlap per chunk: twelve chunks
    assert all(cost(k, 3) > two for k in range(10))  # at most two overlaps per chunk: six chunks or more
    want = OM.extend_overlaps(records, reads, drafts, EXTENSION, M)
    for budget in (one, two, 0):
        same(cm.extend_overlaps(records, reads, drafts, extension=EXTENSION, max_extension=M, max_device_bytes=budget), want)
    with pytest.raises(cm.MapperError, match="max_device_bytes"):
        cm.extend_overlaps(records, reads, drafts, extension=EXTENSION, max_extension=M, max_device_bytes=min(cost(k, 1) for k in range(12)) - 1)


def test_max_extension_0_returns_the_input(cm, exact):
    reads, drafts, records, truth, want = exact
    got = cm.extend_overlaps(records, reads, drafts, max_extension=0)
    same_records(got[0], records)
    assert not got[1].any() and not got[2].any()
    assert got[1].shape == (12, 4) and got[2].shape == (12, 2)


def test_ends_at_the_very_start_and_end_of_a_read(cm):
    # nothing pulled in: the query slices are empty at both ends, and read 0 / read 1 leave the target none at one end
    reads, drafts, records, truth = cases.case(13, pulls=(0,))
    got = cm.extend_overlaps(records, reads, drafts, extension=EXTENSION)
    same(got, OM.extend_overlaps(records, reads, drafts, EXTENSION, 1024))
    same_records(got[0], records)
    assert not got[1].any() and not got[2].any()
    empty = cm.extend_overlaps(records[:0], reads, drafts)
    assert len(empty[0]) == 0 and empty[1].shape == (0, 4) and empty[2].shape == (0, 2)


def test_align_overlaps_replays_over_the_extended_slices(cm, noisy):
    reads, drafts, records, truth, want = noisy
    extended = cm.extend_overlaps(records, reads, drafts, extension=EXTENSION)[0]
    cigars, edits = cm.align_overlaps(extended, reads, drafts)
    assert (edits >= 0).all()
    for x, cigar in zip(extended, cigars):
        q, t = reads[int(x["query_read_id"])], drafts[0]
        record = ["q", str(len(q)), str(x["query_start_position_in_read"]), str(x["query_end_position_in_read"]),
                  chr(x["relative_strand"]), "t", str(len(t)), str(x["target_start_position_in_read"]),
                  str(x["target_end_position_in_read"]), "0", "0", "255", "cg:Z:" + cigar]
        cigar_replay.replay_paf(record, {"q": q}, {"t": t})


def test_refusals(cm, exact):
    reads, drafts, records, truth, want = exact
    for bad in ((2, 4, 4, 2, 512, 200), (64, 64, 4, 2, 64, 200), (2, 4, 128, 2, 64, 200), (2, 4, 4, 127, 64, 200),
                (2, 4, 4, 2, 64, -2), (2, 4, 4, 2, 64), dict(bandwidth=3)):
        with pytest.raises(ValueError):
            cm.extend_overlaps(records, reads, drafts, extension=bad)
    for M in (-1, 2 ** 19 + 1):
        with pytest.raises(ValueError):
            cm.extend_overlaps(records, reads, drafts, max_extension=M)
    for field, value, text in (("query_read_id", 12, "outside the read set"), ("target_read_id", 1, "outside the read set"),
                               ("query_end_position_in_read", 5000, "beyond the end"),
                               ("target_start_position_in_read", 1999, "behind its end")):
        broken = records.copy()
        broken[3][field] = value
        with pytest.raises(cm.MapperError, match=text):
            cm.extend_overlaps(broken, reads, drafts)
    with pytest.raises(cm.MapperError, match="negative max_device_bytes"):
        cm.extend_overlaps(records, reads, drafts, max_device_bytes=-1)
