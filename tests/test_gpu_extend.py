"""The affine X-drop extension on the device, through CudaAlignerBatch(algorithm="extend"): states, lengths, scores, ends
and flags byte for byte those of tests/oracle_extend.py, and the score-only mode at the
kernel level against the full call."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import extend_cases as cases
import oracle_extend as O
from test_extend_oracle import LIB, _Args

pytestmark = pytest.mark.gpu

BANDS = [0, 1, 7, 31, 32, 63, 64, 127, 128, 255, 256, 511]  # every K, both sides of each lane-block edge
XDROPS = [0, 10, 200, -1]


def _batch(n, scores, B, X, longest=400, memory=1 << 30):
    from genomeworks_amd import cudaaligner
    a, x, o, e = scores
    return cudaaligner.CudaAlignerBatch(longest, longest, max(n, 1), algorithm="extend", match=a, mismatch=x, gap_open=o,
                                        gap_extend=e, band_width=B, xdrop=X, max_device_memory_allocator_caching_size=memory)


def _extend(batch, pairs):
    from genomeworks_amd import cudaaligner
    for q, t in pairs:
        assert batch.add_alignment(q, t) == cudaaligner.success
    batch.align_all()
    return batch.get_alignments()


def _check(got, pairs, scores, B, X):
    """every alignment against the oracle, none left out; returns how many dropped"""
    assert len(got) == len(pairs)
    dropped = 0
    for k, (a, (q, t)) in enumerate(zip(got, pairs)):
        want = O.extend(q, t, *scores, B, X)
        where = (k, q, t, scores, B, X)
        assert a.status == 0 and not a.is_optimal, where
        assert list(a.alignment) == want["states"], where
        assert (a.query_end, a.target_end, a.score, a.dropped) == \
            (want["query_end"], want["target_end"], want["score"], bool(want["dropped"])), where
        assert a.edit_distance == sum(1 for s in want["states"] if s != 0), where
        assert a.cigar == O.cigar(want["states"]) and a.cigar_extended == O.cigar(want["states"], True), where
        dropped += want["dropped"]
    return dropped


@pytest.mark.parametrize("q,t,B,X,ends,score,dropped,states", cases.LITERAL)
def test_literal_cases(q, t, B, X, ends, score, dropped, states):
    (a,) = _extend(_batch(1, cases.DEFAULT, B, X), [(q, t)])
    assert (a.status, (a.query_end, a.target_end), a.score, list(a.alignment)) == (0, ends, score, states)
    if dropped is not None:
        assert a.dropped == bool(dropped)
    _check([a], [(q, t)], cases.DEFAULT, B, X)


def test_defaults_are_the_stated_ones():
    from genomeworks_amd import cudaaligner
    batch = cudaaligner.CudaAlignerBatch(400, 400, 1, algorithm="extend", max_device_memory_allocator_caching_size=1 << 30)
    (a,) = _extend(batch, [(cases.ISLAND_Q, cases.ISLAND_T)])  # (2, 4, 4, 2), B = 64, X = 200
    assert (a.query_end, a.target_end, a.score, a.dropped) == (56, 56, 76, False)


@pytest.mark.parametrize("scores", cases.SCORE_SETS)
def test_seeded_pairs_over_the_bands_and_xdrops(scores):
    dropped = total = 0
    for B in BANDS:
        for X in XDROPS:
            pairs = cases.pairs(1000 + 7 * B + X, 5, 300)
            dropped += _check(_extend(_batch(len(pairs), scores, B, X), pairs), pairs, scores, B, X)
            total += len(pairs)
    assert 20 <= dropped <= total - 20  # both ways out of the loop were taken


def test_5_against_300_and_the_reverse():
    r = random.Random(9)
    short, long_ = cases.random_sequence(r, 5), cases.random_sequence(r, 300)
    pairs = [(short, short + long_[:295]), (short + long_[:295], short), (short, long_), (long_, short)]
    for B in (0, 7, 64, 511):
        for X in (5, -1):
            _check(_extend(_batch(4, cases.DEFAULT, B, X), pairs), pairs, cases.DEFAULT, B, X)


def test_batch_of_300_in_which_dropped_and_undropped_pairs_alternate():
    # more than one block's waves; a wave that stops early sits between two that run to the end
    r = random.Random(21)
    pairs = []
    for k in range(300):
        related = cases.random_sequence(r, r.randrange(20, 100))
        if k % 2:
            pairs.append((related + cases.random_sequence(r, 80), cases.mutate(r, related, 0.05) + cases.random_sequence(r, 80)))
        else:
            pairs.append((related, related))
    got = _extend(_batch(300, cases.DEFAULT, 16, 20), pairs)
    assert _check(got, pairs, cases.DEFAULT, 16, 20) >= 140
    assert [a.dropped for a in got[0:300:2]] == [False] * 150


def test_a_pair_over_the_memory_given_sits_between_two_that_keep_their_results():
    from genomeworks_amd import cudaaligner
    r = random.Random(4)
    small = [(s, cases.mutate(r, s, 0.1)) for s in (cases.random_sequence(r, 150), cases.random_sequence(r, 200))]
    big = cases.random_sequence(r, 100000)
    # 8 MiB given: 2 x 100 000 bases at B = 64 need about 13 MB of bits
    batch = _batch(3, cases.DEFAULT, 64, 50, longest=100000, memory=1 << 23)
    assert batch.add_alignment(*small[0]) == 0
    assert batch.add_alignment(big, big) == cudaaligner.exceeded_max_alignments
    assert batch.add_alignment(*small[1]) == 0
    batch.align_all()
    got = batch.get_alignments()
    _check(got, small, cases.DEFAULT, 64, 50)


def test_reset_and_reuse():
    batch = _batch(8, cases.DEFAULT, 16, 30)
    first, second = cases.pairs(41, 8, 150), cases.pairs(42, 5, 250)
    _check(_extend(batch, first), first, cases.DEFAULT, 16, 30)
    batch.reset()
    _check(_extend(batch, second), second, cases.DEFAULT, 16, 30)
    assert batch.stage_ms()[0] > 0
    assert batch.get_alignments_device() is None  # no device-resident form
    with pytest.raises(RuntimeError):
        batch.relaunch()


def test_other_aligners_alignments_carry_no_extension():
    from genomeworks_amd import cudaaligner
    batch = cudaaligner.CudaAlignerBatch(100, 100, 1, max_device_memory_allocator_caching_size=1 << 30)
    assert batch.add_alignment("ACGTACGT", "ACGTACGT") == 0
    batch.align_all()
    (a,) = batch.get_alignments()
    assert (a.query_end, a.target_end, a.score, a.dropped) == (-1, 8, -1, False)
    four = (C.c_int32 * 4)(9, 9, 9, 9)
    assert batch._L.gw_alignment_extension(batch._h, 0, C.byref(four)) == 0 and list(four) == [-1, -1, -1, 0]


def _kernel_level(pairs, scores, B, X, store):
    """gwhip_extend on torch buffers: (lengths, scores, query ends, target ends, flags, states or None). Score-only mode is
    handed the lengths' buffer as well, poisoned with -7, and must leave it as it is."""
    import torch
    L = C.CDLL(os.path.join(LIB, "libgwaffine.so"))
    L.gwhip_extend_workspace_bytes.restype = C.c_size_t
    L.gwhip_extend_workspace_bytes.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32]
    L.gwhip_extend.argtypes = [C.POINTER(_Args), C.c_void_p]
    L.gwhip_affine_last_error.restype = C.c_char_p
    n = len(pairs)
    starts = np.zeros(2 * n + 1, np.int64)
    for k, (q, t) in enumerate(pairs):
        starts[2 * k + 1] = starts[2 * k] + len(q)
        starts[2 * k + 2] = starts[2 * k + 1] + len(t)
    text = np.frombuffer(("".join(q + t for q, t in pairs) + "N" * 16).encode(), np.uint8)
    d_seq, d_starts = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(starts).cuda()
    numbers = torch.full((4, n), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    host_starts = starts.ctypes.data_as(C.POINTER(C.c_int64))
    a = _Args(n, d_seq.data_ptr(), d_starts.data_ptr(), host_starts, *scores, B, X, None, numbers[0].data_ptr(), numbers[1].data_ptr(),
              numbers[2].data_ptr(), numbers[3].data_ptr(), flags.data_ptr(), None, 0)
    results = None
    if store:
        need = L.gwhip_extend_workspace_bytes(n, host_starts, B, 1)
        workspace = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
        results = torch.full((int(starts[-1]) + 16,), 5, dtype=torch.int8, device="cuda")
        a.results, a.workspace, a.workspace_bytes = results.data_ptr(), workspace.data_ptr(), need
    rc = L.gwhip_extend(C.byref(a), None)
    assert rc == 0, L.gwhip_affine_last_error().decode()
    torch.cuda.synchronize()
    numbers = numbers.cpu().numpy()
    states = None
    if store:
        back = results.cpu().numpy()
        states = [list(back[starts[2 * k]:starts[2 * k] + numbers[0][k]][::-1]) for k in range(n)]
        assert all(v == 5 for v in back[starts[-1]:])  # nothing behind the last slot
    return numbers[0], numbers[1], numbers[2], numbers[3], flags.cpu().numpy(), states


@pytest.mark.parametrize("B", [0, 7, 40, 64, 200, 511])
def test_score_only_mode_is_the_full_call_without_its_states(B):
    pairs = cases.pairs(500 + B, 40, 300)
    for X in (10, -1):
        full = _kernel_level(pairs, cases.DEFAULT, B, X, True)
        alone = _kernel_level(pairs, cases.DEFAULT, B, X, False)
        for k in (1, 2, 3, 4):
            assert list(full[k]) == list(alone[k])
        for k, (q, t) in enumerate(pairs):
            want = O.extend(q, t, *cases.DEFAULT, B, X)
            assert (full[1][k], full[2][k], full[3][k], full[4][k], full[5][k]) == \
                (want["score"], want["query_end"], want["target_end"], want["dropped"], want["states"]), (k, q, t, B, X)
        assert (alone[0] == -7).all() and alone[5] is None  # score-only mode writes no length


def test_a_pair_of_2_to_the_21_columns_has_no_result_and_its_neighbours_keep_theirs():
    first, last = cases.pairs(77, 2, 200)
    pairs = [first, ("A" * (1 << 20), "A" * (1 << 20)), last]  # n + m = 2^21: one pair built to have none
    for store in (True, False):
        lengths, scores, query_ends, target_ends, flags, states = _kernel_level(pairs, cases.DEFAULT, 16, 30, store)
        assert sum(1 for s in scores if s < 0) == 1
        assert (scores[1], query_ends[1], target_ends[1], flags[1]) == (-1, -1, -1, 0)
        if store:
            assert lengths[1] == 0 and states[1] == []
        for k in (0, 2):
            want = O.extend(*pairs[k], *cases.DEFAULT, 16, 30)
            assert (scores[k], query_ends[k], target_ends[k], flags[k]) == \
                (want["score"], want["query_end"], want["target_end"], want["dropped"])
            if store:
                assert states[k] == want["states"]


def test_kernel_level_empty_batch_launches_nothing():
    assert _kernel_level([], cases.DEFAULT, 16, 10, False)[1].size == 0
