"""Pileup cases worked out on paper, shared by tests/test_pileup_oracle.py and
tests/test_gpu_pileup.py. Every case is one overlap record whose optimal alignment is unique, so that neither the
oracle's nor the device aligner's tie-breaks matter: the target slice T has no A and no two equal neighbours, a
substituted or inserted base is an A (on '-' a T, which the reverse complement of T does not hold), and a deleted base
differs from both of its neighbours. TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle_mapper as O

CHANNELS = ("A", "C", "G", "T", "deletion", "insertion")

T = "CGTGCTGTCGTC"   # C at 0 4 8 11, G at 1 3 6 9, T at 2 5 7 10
RC = "GACGACAGCACG"  # its reverse complement: column j of a '-' alignment holds T[11 - j]
TS, QS = 2, 1        # where the slices begin in their reads
TARGET = "TC" + T + "GT"
OWN = dict(C=[0, 4, 8, 11], G=[1, 3, 6, 9], T=[2, 5, 7, 10])  # every base of T supported as it is

# name -> (query slice, strand, cells of the target read, cells of the query read): channel -> positions within the
# slice with count 1. The target's cells are those of the target role, the query's those of the query role.
HAND = {
    # T[4] = C reads A
    "mismatch": ("CGTGATGTCGTC", "+",
                 dict(A=[4], C=[0, 8, 11], G=[1, 3, 6, 9], T=[2, 5, 7, 10]), OWN),
    # T[5] is missing from the query: a column of state 2; for the query it is an insertion behind its base 4
    "deleted_target_base": ("CGTGC" + "GTCGTC", "+",
                            dict(C=[0, 4, 8, 11], G=[1, 3, 6, 9], T=[2, 7, 10], deletion=[5]),
                            dict(C=[0, 4, 7, 10], G=[1, 3, 5, 8], T=[2, 6, 9], insertion=[4])),
    # AA between T[5] and T[6]: one run of state 3, counted once, at the smaller neighbour; the query has two bases
    # the target deletes
    "insertion_of_two": ("CGTGCT" + "AA" + "GTCGTC", "+",
                         dict(OWN, insertion=[5]),
                         dict(C=[0, 4, 10, 13], G=[1, 3, 8, 11], T=[2, 5, 9, 12], deletion=[6, 7])),
    # runs in the first and in the last column have a neighbour on one side only: not counted
    "runs_at_both_ends": ("AA" + T + "A", "+",
                          OWN,
                          dict(C=[2, 6, 10, 13], G=[3, 5, 8, 11], T=[4, 7, 9, 12], deletion=[0, 1, 14])),
    # '-': column 3 holds T[8] = C, read as G on the reverse strand; the query has T there, which is A on the forward
    # strand. The query's cells are the letters of RC.
    "mismatch_reverse": ("GACTACAGCACG", "-",
                         dict(A=[8], C=[0, 4, 11], G=[1, 3, 6, 9], T=[2, 5, 7, 10]),
                         dict(A=[1, 4, 6, 9], C=[2, 5, 8, 10], G=[0, 3, 7, 11])),
    # '-': TT between columns 3 and 4, that is between T[8] and T[7]: the smaller coordinate is 7
    "insertion_reverse": ("GACG" + "TT" + "ACAGCACG", "-",
                          dict(OWN, insertion=[7]),
                          dict(A=[1, 6, 8, 11], C=[2, 7, 10, 12], G=[0, 3, 9, 13], deletion=[4, 5])),
    # '-': column 5, T[6], is missing from the query
    "deleted_target_base_reverse": ("GACGA" + "AGCACG", "-",
                                    dict(C=[0, 4, 8, 11], G=[1, 3, 9], T=[2, 5, 7, 10], deletion=[6]),
                                    dict(A=[1, 4, 5, 8], C=[2, 7, 9], G=[0, 3, 6, 10], insertion=[4])),
    "runs_at_both_ends_reverse": ("T" + RC + "TT", "-",
                                  OWN,
                                  dict(A=[2, 5, 7, 10], C=[3, 6, 9, 11], G=[1, 4, 8, 12], deletion=[0, 13, 14])),
}
NAMES = sorted(HAND)


def reads():
    """read 0 is the target; read 1 + i holds the query slice of case NAMES[i]"""
    return [TARGET] + ["G" + HAND[name][0] + "C" for name in NAMES]


def record(name):
    """the OVERLAP record of a case over reads()"""
    q = HAND[name][0]
    return (1 + NAMES.index(name), 0, QS, TS, QS + len(q), TS + len(T), ord(HAND[name][1]), 0, 0)


def records(names):
    return np.array([record(name) for name in names], O.OVERLAP).reshape(-1)


def cells(length, at, table, times=1):
    """the (6, length) array of a table of cells whose positions count from `at`"""
    out = np.zeros((6, length), np.uint32)
    for channel, positions in table.items():
        for p in positions:
            out[CHANNELS.index(channel), at + p] += times
    return out


def expected(names, roles=(False, True)):
    """the pileups of reads() under records(names): the target's cells in read 0 (role False) and every query's in
    its own read (role True)"""
    rs = reads()
    out = [np.zeros((6, len(r)), np.uint32) for r in rs]
    for name in names:
        if False in roles:
            out[0] += cells(len(rs[0]), TS, HAND[name][2])
        if True in roles:
            i = 1 + NAMES.index(name)
            out[i] += cells(len(rs[i]), QS, HAND[name][3])
    return out


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
                                    for x, y in zip(a, b))


def unique_target(rng, n):
    """n bases of C, G, T without two equal neighbours"""
    out = [int(rng.integers(0, 3))]
    while len(out) < n:
        out.append((out[-1] + 1 + int(rng.integers(0, 2))) % 3)
    return "".join("CGT"[c] for c in out)


def rc(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
