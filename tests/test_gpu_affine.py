"""The affine-gap global aligner on the device, through CudaAlignerBatch(algorithm="affine"): states, lengths, costs
and flags byte for byte those of tests/oracle_affine.py."""
import random

import pytest

import affine_cases as cases
import oracle_affine as O

pytestmark = pytest.mark.gpu


def _batch(n, scores, B, longest=400):
    from genomeworks_amd import cudaaligner
    x, o, e = scores
    return cudaaligner.CudaAlignerBatch(longest, longest, max(n, 1), algorithm="affine", mismatch=x, gap_open=o, gap_extend=e,
                                        band_width=B, max_device_memory_allocator_caching_size=1 << 30)


def _align(batch, pairs):
    from genomeworks_amd import cudaaligner
    for q, t in pairs:
        assert batch.add_alignment(q, t) == cudaaligner.success
    batch.align_all()
    return batch.get_alignments()


def _check(got, pairs, scores, B):
    """every alignment against the oracle; returns the number of pairs without a result"""
    assert len(got) == len(pairs)
    none = 0
    for k, (a, (q, t)) in enumerate(zip(got, pairs)):
        want = O.align(q, t, *scores, B)
        where = (k, q, t, scores, B)
        if want["states"] is None:
            none += 1
            assert (a.status, a.cost, list(a.alignment), a.is_optimal, a.cigar) == (1, -1, [], False, ""), where
            continue
        assert a.status == 0, where
        assert list(a.alignment) == want["states"], where
        assert (a.cost, a.is_optimal) == (want["cost"], want["optimal"]), where
        assert a.edit_distance == sum(1 for s in want["states"] if s != 0), where
        assert a.cigar == O.cigar(want["states"]) and a.cigar_extended == O.cigar(want["states"], True), where
    return none


def test_literal_cases():
    for q, t, scores, B, states, cost, optimal in cases.LITERAL:
        (a,) = _align(_batch(1, scores, B), [(q, t)])
        assert (a.status, a.cost, a.is_optimal) == (0, cost, optimal), (q, t, B)
        if states is not None:
            assert list(a.alignment) == states
        _check([a], [(q, t)], scores, B)


def test_clipped_pair_is_unflagged_at_band_zero():
    (a,) = _align(_batch(1, cases.DEFAULT, 0), [(cases.CLIPPED_Q, cases.CLIPPED_T)])
    assert (a.cost, a.is_optimal, a.status) == (40, False, 0)
    (a,) = _align(_batch(1, cases.DEFAULT, 5), [(cases.CLIPPED_Q, cases.CLIPPED_T)])
    assert (a.cost, a.is_optimal) == (32, True)


def test_two_empty_sequences():
    got = _align(_batch(3, cases.DEFAULT, 4), [("", ""), ("ACGT", "ACGT"), ("", "")])
    assert [(a.status, a.cost, list(a.alignment), a.is_optimal) for a in got] == \
        [(0, 0, [], True), (0, 0, [0, 0, 0, 0], True), (0, 0, [], True)]


@pytest.mark.parametrize("scores", cases.SCORE_SETS)
def test_seeded_pairs_over_the_bands(scores):
    # 0-300 bases, 0-30 % errors, truncated targets; B below, at and above the lane-block edges of the narrow variants
    for B in (0, 1, 7, 31, 32, 33, 64, 200):
        pairs = cases.pairs(1000 + B, 7, 300)
        assert _check(_align(_batch(len(pairs), scores, B), pairs), pairs, scores, B) == 0


@pytest.mark.parametrize("W", [63, 64, 65, 127, 128, 129])
def test_lane_block_edges(W):
    # W = |m - n| + 2 B + 1 exactly, with the longer sequence on either side
    for difference in ((0,) if W % 2 else (1, -1)):
        B = (W - 1 - abs(difference)) // 2
        pairs = [cases.pair_with_band(W * 10 + k, 200 + 13 * k, difference, 0.2) for k in range(3)]
        assert all(O.band(len(q), len(t), B)[2] == W for q, t in pairs)
        assert _check(_align(_batch(len(pairs), cases.DEFAULT, B), pairs), pairs, cases.DEFAULT, B) == 0


def test_sixteen_diagonals_a_lane():
    # W = 601 + |m - n|: the one register variant that the bands above do not reach
    pairs = cases.pairs(91, 6, 300)
    assert all(512 < O.band(len(q), len(t), 300)[2] <= 1024 for q, t in pairs)
    assert _check(_align(_batch(len(pairs), cases.DEFAULT, 300), pairs), pairs, cases.DEFAULT, 300) == 0


def test_band_capacity_2047_2048_2049():
    # about 1 100 bases at B = 1023: W = 2047 (equal lengths) and 2048 (one base apart, either way)
    a1, a2, a3 = (cases.pair_with_band(s, 1100, d, 0.15) for s, d in ((1, 0), (2, 1), (3, -1)))
    pairs = [a1, a2, a3]
    assert [O.band(len(q), len(t), 1023)[2] for q, t in pairs] == [2047, 2048, 2048]
    assert _check(_align(_batch(3, cases.DEFAULT, 1023, 1200), pairs), pairs, cases.DEFAULT, 1023) == 0
    from genomeworks_amd import cudaaligner
    # an aligner has one B, so the pair of W = 2049 that sits between pairs that keep their results is two bases apart
    # at B = 1023; W = 2049 from B = 1024 and equal lengths follows, alone
    over = cases.pair_with_band(4, 1100, 2, 0.15)
    assert O.band(len(over[0]), len(over[1]), 1023)[2] == 2049
    mixed = [a1, over, a2]
    got = _align(_batch(3, cases.DEFAULT, 1023, 1200), mixed)
    assert _check(got, mixed, cases.DEFAULT, 1023) == 1
    assert got[1].status == cudaaligner.uninitialized and got[0].status == got[2].status == 0
    (alone,) = _align(_batch(1, cases.DEFAULT, 1024, 1200), [a1])  # W = 2049 from B = 1024
    assert (alone.status, alone.cost, list(alone.alignment)) == (cudaaligner.uninitialized, -1, [])


def test_short_against_long_at_band_zero():
    r = random.Random(5)
    short, long_ = cases.random_sequence(r, 5), cases.random_sequence(r, 300)
    pairs = [(short, long_), (long_, short)]
    assert _check(_align(_batch(2, cases.DEFAULT, 0), pairs), pairs, cases.DEFAULT, 0) == 0


def test_batch_of_300_mixed_pairs():
    # more than one block's waves, more than the 64 pairs of one traceback wave
    pairs = cases.pairs(77, 300, 120)
    pairs[17], pairs[200] = ("", ""), ("ACGT" * 20, "")
    assert _check(_align(_batch(300, (2, 3, 1), 40), pairs), pairs, (2, 3, 1), 40) == 0


def test_unit_scores_in_a_full_band_equal_the_default_aligner():
    from genomeworks_amd import cudaaligner
    pairs = [p for p in cases.pairs(31, 40, 200) if p[0] or p[1]]
    affine = _align(_batch(len(pairs), (1, 0, 1), 300), pairs)
    default = _align(cudaaligner.CudaAlignerBatch(400, 400, len(pairs), max_device_memory_allocator_caching_size=1 << 30), pairs)
    for a, d in zip(affine, default):
        assert a.is_optimal and a.cost == d.edit_distance
        assert d.cost == -1  # other aligners' alignments carry no cost


def test_reset_and_reuse():
    batch = _batch(8, cases.DEFAULT, 16)
    first, second = cases.pairs(41, 8, 150), cases.pairs(42, 5, 250)
    assert _check(_align(batch, first), first, cases.DEFAULT, 16) == 0
    batch.reset()
    assert _check(_align(batch, second), second, cases.DEFAULT, 16) == 0
    assert batch.stage_ms()[0] > 0
    assert batch.get_alignments_device() is None  # no device-resident form
    with pytest.raises(RuntimeError):
        batch.relaunch()
    with pytest.raises(RuntimeError):
        batch.band_cells()


def test_limits_and_memory_are_statuses():
    from genomeworks_amd import cudaaligner
    batch = cudaaligner.CudaAlignerBatch(100, 100, 2, algorithm="affine", max_device_memory_allocator_caching_size=1 << 26)
    assert batch.add_alignment("A" * 101, "A") == cudaaligner.exceeded_max_length
    assert batch.add_alignment("ACGT", "ACGT") == 0 and batch.add_alignment("ACGT", "ACGA") == 0
    assert batch.add_alignment("ACGT", "ACGT") == cudaaligner.exceeded_max_alignments
    batch.align_all()
    assert [a.cost for a in batch.get_alignments()] == [0, 4]
    # 64 MiB given: a pair of 2 x 200 000 bases at B = 128 needs about 52 MB of bits, a second one does not fit
    big = cudaaligner.CudaAlignerBatch(200000, 200000, 4, algorithm="affine", max_device_memory_allocator_caching_size=1 << 26)
    assert big.add_alignment("A" * 200000, "A" * 200000) == 0
    assert big.add_alignment("A" * 200000, "A" * 200000) == cudaaligner.exceeded_max_alignments


def test_out_of_range_parameters_raise():
    from genomeworks_amd import cudaaligner
    for bad in (dict(mismatch=0), dict(gap_open=256), dict(gap_extend=0), dict(band_width=-1)):
        with pytest.raises(RuntimeError):
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", **bad)
    with pytest.raises(RuntimeError):
        cudaaligner.CudaAlignerBatch(100, 100, 10, mismatch=4)
