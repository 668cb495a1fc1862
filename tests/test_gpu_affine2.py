"""The two-piece affine-gap global aligner on the device, through CudaAlignerBatch(algorithm="affine", gap_open2=,
gap_extend2=): states, lengths, costs and flags byte for byte those of tests/oracle_affine2.py (INTEGRATION.md
section 3p)."""
import random

import pytest

import affine2_cases as cases
import oracle_affine2 as O

pytestmark = pytest.mark.gpu


def _batch(n, scores, B, longest=400):
    from genomeworks_amd import cudaaligner
    x, o1, e1, o2, e2 = scores
    return cudaaligner.CudaAlignerBatch(longest, longest, max(n, 1), algorithm="affine", mismatch=x, gap_open=o1, gap_extend=e1,
                                        gap_open2=o2, gap_extend2=e2, band_width=B,
                                        max_device_memory_allocator_caching_size=1 << 30)


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
    for q, t, scores, B, cost, longest, optimal in cases.LITERAL:
        (a,) = _align(_batch(1, scores, B), [(q, t)])
        assert (a.status, a.cost, a.is_optimal) == (0, cost, optimal), (q, t, B)
        if longest is not None:
            assert O.runs(list(a.alignment)) == [longest]
        _check([a], [(q, t)], scores, B)


def test_defaults_are_the_stated_ones():
    from genomeworks_amd import cudaaligner
    q, t = cases.LITERAL[0][:2]
    batch = cudaaligner.CudaAlignerBatch(400, 400, 1, algorithm="affine", gap_open2=24, gap_extend2=2, band_width=40,
                                         max_device_memory_allocator_caching_size=1 << 30)
    (a,) = _align(batch, [(q, t)])
    assert a.cost == 84  # (6, 4, 3, 24, 2); the one-piece defaults (4, 6, 2) would give 66


@pytest.mark.parametrize("scores", cases.SCORE_SETS)
def test_seeded_pairs_over_the_bands(scores):
    # 0-300 bases, 0-30 % errors, truncated targets, every third with one run of 21-60 bases spliced in or out
    spliced = 0
    for B in cases.BANDS:
        pairs = cases.spliced_pairs(1000 + B, 7, 300)
        got = _align(_batch(len(pairs), scores, B, 480), pairs)
        assert _check(got, pairs, scores, B) == 0
        spliced += sum(1 for a in got if any(L >= 21 for _, L in O.runs(list(a.alignment))))
    assert spliced >= 3  # long runs did come out whole


def test_the_second_piece_crosses_lane_edges_both_ways():
    # K = 4 at B = 64 and K = 8 at B = 200: a run of 40 target-only / query-only columns walks E2 / F2 over 40
    # diagonals, ten / five lanes, upwards and downwards
    r = random.Random(12)
    base = cases.random_sequence(r, 260)
    longer = base[:120] + cases.random_sequence(r, 40) + base[120:]
    pairs = [(base, longer), (longer, base)]
    for B in (64, 200):
        got = _align(_batch(2, cases.DEFAULT, B), pairs)
        assert _check(got, pairs, cases.DEFAULT, B) == 0
        assert [(a.cost, O.runs(list(a.alignment))) for a in got] == [(104, [(2, 40)]), (104, [(3, 40)])]


@pytest.mark.parametrize("W", [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513])
def test_lane_block_edges(W):
    # W = |m - n| + 2 B + 1 exactly, with the longer sequence on either side: every register variant, K = 1 .. 16
    for difference in ((0,) if W % 2 else (1, -1)):
        B = (W - 1 - abs(difference)) // 2
        pairs = [cases.pair_with_band(W * 10 + k, 200 + 13 * k, difference, 0.2) for k in range(3)]
        assert all(O.band(len(q), len(t), B)[2] == W for q, t in pairs)
        assert _check(_align(_batch(len(pairs), cases.DEFAULT, B), pairs), pairs, cases.DEFAULT, B) == 0


def test_band_capacity_1023_1024_1025():
    from genomeworks_amd import cudaaligner
    # about 600 bases at B = 511: W = 1023 (equal lengths), 1024 (one base apart, either way), 1025 (two apart)
    a1, a2, a3 = (cases.pair_with_band(s, 600, d, 0.15) for s, d in ((1, 0), (2, 1), (3, -1)))
    pairs = [a1, a2, a3]
    assert [O.band(len(q), len(t), 511)[2] for q, t in pairs] == [1023, 1024, 1024]
    assert _check(_align(_batch(3, cases.DEFAULT, 511, 700), pairs), pairs, cases.DEFAULT, 511) == 0
    over = cases.pair_with_band(4, 600, 2, 0.15)
    assert O.band(len(over[0]), len(over[1]), 511)[2] == 1025
    mixed = [a1, over, a2]  # the pair over the capacity sits between two that keep their results
    got = _align(_batch(3, cases.DEFAULT, 511, 700), mixed)
    assert _check(got, mixed, cases.DEFAULT, 511) == 1
    assert got[1].status == cudaaligner.uninitialized and got[0].status == got[2].status == 0
    (alone,) = _align(_batch(1, cases.DEFAULT, 512, 700), [a1])  # W = 1025 from B = 512
    assert (alone.status, alone.cost, list(alone.alignment)) == (cudaaligner.uninitialized, -1, [])


def test_batch_of_300_mixed_pairs():
    # more than one block's waves
    pairs = cases.spliced_pairs(77, 300, 120)
    pairs[17], pairs[200] = ("", ""), ("ACGT" * 20, "")
    assert _check(_align(_batch(300, (5, 0, 3, 9, 1), 40), pairs), pairs, (5, 0, 3, 9, 1), 40) == 0


@pytest.mark.parametrize("scores", [cases.DOMINATED, cases.IDENTICAL])
def test_a_second_piece_that_never_wins_is_the_one_piece_aligner(scores):
    from genomeworks_amd import cudaaligner
    pairs = cases.spliced_pairs(55, 40, 300)
    flags = []
    for B in (7, 64):
        two = _align(_batch(len(pairs), scores, B, 480), pairs)
        x, o, e = scores[:3]
        one = _align(cudaaligner.CudaAlignerBatch(480, 480, len(pairs), algorithm="affine", mismatch=x, gap_open=o, gap_extend=e,
                                                  band_width=B, max_device_memory_allocator_caching_size=1 << 30), pairs)
        assert [(a.status, list(a.alignment), a.cost, a.is_optimal) for a in two] == \
            [(a.status, list(a.alignment), a.cost, a.is_optimal) for a in one]
        flags += [a.is_optimal for a in one if a.cost > 0]
    assert True in flags and False in flags


def test_unit_scores_in_a_full_band_equal_the_default_aligner():
    from genomeworks_amd import cudaaligner
    pairs = [p for p in cases.pairs(31, 40, 200) if p[0] or p[1]]
    affine = _align(_batch(len(pairs), (1, 0, 1, 0, 1), 300), pairs)
    default = _align(cudaaligner.CudaAlignerBatch(400, 400, len(pairs), max_device_memory_allocator_caching_size=1 << 30), pairs)
    for a, d in zip(affine, default):
        assert a.is_optimal and a.cost == d.edit_distance


def test_reset_and_reuse():
    batch = _batch(8, cases.DEFAULT, 16)
    first, second = cases.spliced_pairs(41, 8, 150), cases.spliced_pairs(42, 5, 250)
    assert _check(_align(batch, first), first, cases.DEFAULT, 16) == 0
    batch.reset()
    assert _check(_align(batch, second), second, cases.DEFAULT, 16) == 0
    assert batch.stage_ms()[0] > 0
    assert batch.get_alignments_device() is None  # no device-resident form
    with pytest.raises(RuntimeError):
        batch.relaunch()


def test_limits_and_memory_are_statuses():
    from genomeworks_amd import cudaaligner
    batch = cudaaligner.CudaAlignerBatch(100, 100, 2, algorithm="affine", gap_open2=24, gap_extend2=2,
                                         max_device_memory_allocator_caching_size=1 << 26)
    assert batch.add_alignment("A" * 101, "A") == cudaaligner.exceeded_max_length
    assert batch.add_alignment("ACGT", "ACGT") == 0 and batch.add_alignment("ACGT", "ACGA") == 0
    assert batch.add_alignment("ACGT", "ACGT") == cudaaligner.exceeded_max_alignments
    batch.align_all()
    assert [a.cost for a in batch.get_alignments()] == [0, 6]
    # 64 MiB given: a pair of 2 x 200 000 bases at B = 128 needs about 52 MB of bits, a second one does not fit
    big = cudaaligner.CudaAlignerBatch(200000, 200000, 4, algorithm="affine", gap_open2=24, gap_extend2=2,
                                       max_device_memory_allocator_caching_size=1 << 26)
    assert big.add_alignment("A" * 200000, "A" * 200000) == 0
    assert big.add_alignment("A" * 200000, "A" * 200000) == cudaaligner.exceeded_max_alignments
