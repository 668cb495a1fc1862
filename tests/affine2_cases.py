"""Cases of the two-piece affine-gap aligner's tests: the literal ones of INTEGRATION.md section 3p, and seeded
generators on top of those of affine_cases.py."""
import random

from affine_cases import mutate, pair_with_band, pairs, random_sequence  # noqa: F401 (re-exported)

DEFAULT = (6, 4, 3, 24, 2)
ONE_PIECE = (6, 4, 3)  # DEFAULT's first piece alone
DOMINATED, IDENTICAL = (4, 6, 2, 7, 2), (4, 6, 2, 6, 2)  # the second piece never wins / is the first
SCORE_SETS = [DEFAULT, (1, 0, 1, 0, 1), DOMINATED, IDENTICAL, (5, 0, 3, 9, 1), (255, 255, 255, 255, 255),
              (2, 255, 1, 0, 3)]  # the last: the pieces the other way round
BANDS = [0, 1, 7, 31, 32, 33, 64, 200]

_r = random.Random(2)
BASE = random_sequence(_r, 60)
INSERT30, INSERT20 = random_sequence(_r, 30), random_sequence(_r, 20)


def _spliced(insert):
    """BASE with `insert` at position 30: any alignment holds len(insert) more target-only than query-only columns, and
    one whole run is the cheapest way to hold them, so the cost is g(len(insert)) wherever ties place the run"""
    return BASE[:30] + insert + BASE[30:]


# (query, target, (x, o1, e1, o2, e2), B, cost, longest gap run (state, length) or None, optimal)
LITERAL = [
    (BASE, _spliced(INSERT30), DEFAULT, 40, 84, (2, 30), True),   # 24 + 2 * 30: the second piece; (6, 4, 3) prices it 94
    (_spliced(INSERT30), BASE, DEFAULT, 40, 84, (3, 30), True),
    (BASE, _spliced(INSERT20), DEFAULT, 40, 64, (2, 20), True),   # 4 + 3 * 20 == 24 + 2 * 20: a tie, E1 wins it
    (_spliced(INSERT20), BASE, DEFAULT, 40, 64, (3, 20), True),
    ("", "ACG", DEFAULT, 0, 13, (2, 3), True),
    ("ACG", "", DEFAULT, 0, 13, (3, 3), True),
    ("", "", DEFAULT, 0, 0, None, True),
    ("", "A" * 30, DEFAULT, 0, 84, (2, 30), True),
    ("ACGTA", "ACGTA" * 60, DEFAULT, 0, 24 + 2 * 295, None, True),   # 5 against 300 bases at B = 0
    ("ACGTA" * 60, "ACGTA", DEFAULT, 0, 24 + 2 * 295, None, True),
]


def spliced_pairs(seed, count, max_length, max_error=0.30):
    """pairs(): into every third target one run of 21-60 bases is inserted, or one such run of it is deleted, so that the
    second piece of DEFAULT prices it and E2 / F2 are carried across many diagonals"""
    r = random.Random(seed)
    out = []
    for k, (q, t) in enumerate(pairs(seed + 1, count, max_length, max_error)):
        if k % 3 == 0:
            L, at = r.randrange(21, 61), r.randrange(0, len(t) + 1)
            if r.random() < 0.5 or len(t) < L + at:
                t = t[:at] + random_sequence(r, L) + t[at:]
            else:
                t = t[:at] + t[at + L:]
        out.append((q, t))
    return out
