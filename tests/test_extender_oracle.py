"""The cudaextender contract pinned on the CPU: the plain-C oracle (tests/oracle_extender.c) reproduces the
reference's end-to-end known answer (1 337 segments of the committed sample) and the hand-built cases of
extender_cases.py, which the GPU tests (test_gpu_extender.py) run through the HIP library."""
import numpy as np
import pytest

import extender_cases as K
import oracle_extender as X


def test_oracle_reproduces_sample_golden():
    s = K.load_sample()
    assert len(s["seeds"]) == 143670 and len(s["expected"]) == 1337
    got = X.extend(s["sequence"], s["sequence"], s["score_matrix"], s["xdrop"], s["score_threshold"], s["no_entropy"],
                   s["seeds"])
    assert X.rows(got) == s["expected"]


@pytest.mark.parametrize("case", K.extend_cases(), ids=lambda c: c[0])
def test_oracle_known_answers(case):
    name, T, Q, M, xdrop, thr, no_entropy, seeds, expected = case
    assert X.rows(X.extend(T, Q, M, xdrop, thr, no_entropy, seeds)) == expected


@pytest.mark.parametrize("case", K.sort_unique_cases(), ids=lambda c: c[0])
def test_oracle_sort_unique_known_answers(case):
    name, segs, keep, expected = case
    arr = np.array([(q, t, l, s) for (t, q, l, s) in segs], X.SEGMENT)
    kept = arr[np.asarray(keep, bool)] if len(arr) else arr
    assert X.rows(X.sort_unique(kept)) == expected


def test_adjacent_dedup_differs_from_last_kept():
    """The A/B/C case tells thrust::unique_copy (compare with the input predecessor) from std::unique_copy (compare
    with the last kept element): a last-kept comparison would drop C as well."""
    A, B, C = (0, 0, 100, 900), (10, 10, 20, 200), (15, 15, 50, 500)
    arr = np.array([(q, t, l, s) for (t, q, l, s) in (A, B, C)], X.SEGMENT)
    assert X.rows(X.sort_unique(arr)) == [A, C]
    last_kept = [A]
    for seg in (B, C):
        x = np.array([(seg[1], seg[0], seg[2], seg[3]), (last_kept[-1][1], last_kept[-1][0], last_kept[-1][2], 0)], X.SEGMENT)
        if len(X.sort_unique(x)) == 2:
            last_kept.append(seg)
    assert last_kept == [A]


def test_chunks_are_sorted_and_deduplicated_on_their_own():
    s = K.load_sample()
    seeds = s["seeds"][:20000]
    args = (s["sequence"], s["sequence"], s["score_matrix"], s["xdrop"], s["score_threshold"], s["no_entropy"], seeds)
    whole = X.rows(X.extend(*args))
    parts = X.rows(X.extend(*args[:-1], seeds[:7000])) + X.rows(X.extend(*args[:-1], seeds[7000:14000])) + \
        X.rows(X.extend(*args[:-1], seeds[14000:]))
    assert X.rows(X.extend(*args, chunk=7000)) == parts
    assert set(parts) >= set(whole) and parts != whole  # per-chunk order and de-duplication differ from one pass


def test_negative_diagonal_seeds_sort_last():
    case = dict((c[0], c) for c in K.extend_cases())["unsigned_diagonal"]
    rows = X.rows(X.extend(*case[1:8]))
    diags = [(t - q) & 0xFFFFFFFF for t, q, _, _ in rows]
    assert diags == sorted(diags) and diags[-1] == 0xFFFFFFFF
