"""Hand-built known answers for cudaextender, shared by the oracle tests (CPU) and the GPU tests. Each case gives the
inputs and the rows (target, query, length, score) worked out by hand from the contract in extender.hpp."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "golden", "cudaextender_sample.npz")


def matrix(match=10, mismatch=-10):
    """M[8 t + q] = match on equal A/C/G/T, mismatch everywhere else."""
    m = np.full(64, mismatch, np.int32)
    for b in range(4):
        m[8 * b + b] = match
    return m


def load_sample():
    z = np.load(SAMPLE)
    return dict(sequence=z["sequence"], seeds=np.cumsum(z["seed_deltas"].astype(np.int64), axis=0),
                expected=[tuple(int(v) for v in r) for r in z["expected"]], score_matrix=z["score_matrix"],
                xdrop=int(z["xdrop"]), score_threshold=int(z["score_threshold"]), no_entropy=bool(z["no_entropy"]))


def _rand_acgt(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


RUN200 = _rand_acgt(200, 7)
R1, R2 = _rand_acgt(100, 11), _rand_acgt(100, 12)


def extend_cases():
    """(name, target, query, matrix, xdrop, thr, no_entropy, seeds [(t, q)], expected rows)"""
    M = matrix()
    c = []
    # rpos = -1 (every column right of the seed mismatches), lpos = 10: length lpos - 1 = 9, score 100 (10 matching
    # columns < 20: entropy stays 1)
    c.append(("rpos_minus1_lpos10", "ACGTACGTAC" + "AAAAA", "ACGTACGTAC" + "CCCCC", M, 15, 50, False, [(10, 10)],
              [(0, 0, 9, 100)]))
    # rpos = -1 and lpos = 0: length -1, total 0, kept only because thr = 0
    c.append(("rpos_minus1_lpos0", "AAAA", "CCCC", M, 15, 0, False, [(2, 2)], [(2, 2, -1, 0)]))
    c.append(("rpos_minus1_lpos0_dropped", "AAAA", "CCCC", M, 15, 1, False, [(2, 2)], []))
    # seed at 0 and at |T| - 1 on an identical 200-column run: both give the segment [0, 199], total 2000 > 3 thr
    c.append(("seed_at_0", RUN200, RUN200, M, 50, 500, False, [(0, 0)], [(0, 0, 199, 2000)]))
    c.append(("seed_at_end", RUN200, RUN200, M, 50, 500, False, [(199, 199)], [(0, 0, 199, 2000)]))
    c.append(("seed_both_ends_dedup", RUN200, RUN200, M, 50, 500, False, [(0, 0), (199, 199)], [(0, 0, 199, 2000)]))
    # seeds outside the sequences give nothing; the valid seed next to them is unaffected
    c.append(("out_of_range", RUN200, RUN200[:150], M, 50, 400, False, [(200, 0), (0, 150), (4000000000, 3), (0, 0)],
              [(0, 0, 149, 1500)]))
    # entropy edges: "ACGT" * 10, total 400, counts 10 each -> e = ln 4 / (double)logf(4) just below 1 -> score 399
    acgt = "ACGT" * 10
    c.append(("entropy_off_above_3thr", acgt, acgt, M, 50, 133, False, [(0, 0)], [(0, 0, 39, 400)]))
    c.append(("entropy_on_at_3thr", acgt, acgt, M, 50, 134, False, [(0, 0)], [(0, 0, 39, 399)]))
    c.append(("entropy_on_at_thr_dropped", acgt, acgt, M, 50, 400, False, [(0, 0)], []))
    c.append(("entropy_on_below_thr", acgt, acgt, M, 50, 399, False, [(0, 0)], [(0, 0, 39, 399)]))
    c.append(("entropy_off_total_below_thr", acgt, acgt, M, 50, 401, False, [(0, 0)], []))
    # a single-base run has entropy 0 (score 0), unless fewer than 20 matching columns or no_entropy
    c.append(("entropy_zero", "A" * 40, "A" * 40, M, 50, 200, False, [(0, 0)], []))
    c.append(("entropy_zero_no_entropy", "A" * 40, "A" * 40, M, 50, 200, True, [(0, 0)], [(0, 0, 39, 400)]))
    c.append(("entropy_19_columns", "A" * 19, "A" * 19, M, 50, 100, False, [(0, 0)], [(0, 0, 18, 190)]))
    c.append(("entropy_20_columns", "A" * 20, "A" * 20, M, 50, 100, False, [(0, 0)], []))
    # unsigned diagonal order: R1 on diagonal +1, R2 on diagonal -1 (target - query = 0xFFFFFFFF) sorts after it
    T, Q = "G" + R1 + "NN" + R2, R1 + "NNNN" + R2
    c.append(("unsigned_diagonal", T, Q, M, 50, 300, False, [(150, 151), (1, 0)],
              [(1, 0, 99, 1000), (103, 104, 99, 1000)]))
    return c


def sort_unique_cases():
    """(name, segments [(target, query, length, score)], keep flags, expected rows)"""
    c = []
    # one diagonal, A=[0,+100], B=[10,+20], C=[15,+50]: B lies in its predecessor A (dropped); C is compared with its
    # input predecessor B, not with the last kept A, so it stays (std::unique_copy semantics would drop it)
    A, B, C = (0, 0, 100, 900), (10, 10, 20, 200), (15, 15, 50, 500)
    c.append(("adjacent_not_last_kept", [C, A, B], [1, 1, 1], [A, C]))
    # unsigned diagonals: target - query = 0xFFFFFFFF sorts after every non-negative diagonal
    c.append(("unsigned_diagonal", [(0, 1, 5, 50), (7, 0, 5, 50), (3, 3, 5, 50)], [1, 1, 1],
              [(3, 3, 5, 50), (7, 0, 5, 50), (0, 1, 5, 50)]))
    # same start: longer first, then the shorter one is contained and dropped; a flagged-off segment never appears
    c.append(("length_descending", [(5, 5, 10, 100), (5, 5, 30, 300), (50, 50, 3, 30)], [1, 1, 0], [(5, 5, 30, 300)]))
    # identical records collapse to one; equal targets on different diagonals both stay
    c.append(("duplicates", [(9, 2, 4, 40), (9, 2, 4, 40), (9, 3, 4, 40)], [1, 1, 1], [(9, 3, 4, 40), (9, 2, 4, 40)]))
    # length -1 compares as a signed length (sorts after length 0); its interval end wraps to 0xFFFFFFFF in uint32
    # arithmetic, so it contains its predecessor [0, 0] and is dropped
    c.append(("negative_length", [(0, 0, -1, 0), (0, 0, 0, 0)], [1, 1], [(0, 0, 0, 0)]))
    c.append(("empty", [], [], []))
    return c
