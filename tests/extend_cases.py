"""Cases of the affine X-drop extension's tests: the literal ones of INTEGRATION.md section 3q, and seeded generators."""
import random

from affine_cases import mutate, random_sequence

DEFAULT = (2, 4, 4, 2)
# (match, mismatch, gap_open, gap_extend): the default, unit-like ones, and the corners of the ranges
SCORE_SETS = [(2, 4, 4, 2), (1, 1, 0, 1), (1, 3, 5, 2), (5, 4, 0, 1), (63, 64, 127, 96), (1, 0, 0, 1)]

FORTY = "GATGTACCTCGTAATTACACCTCGTTTAATATGCCTCGAG"  # 40 random bases; a gap at 20..24 cannot slide
ISLAND_L, ISLAND_R = "TCCGGCATCCCAAGGGCATC", "CCCGGTCCACGTTACAAGAGCAAAGCACTT"
ISLAND_Q, ISLAND_T = ISLAND_L + "AAAAAA" + ISLAND_R, ISLAND_L + "CCCCCC" + ISLAND_R
DELETED = FORTY[:20] + FORTY[25:]

# (query, target, B, X, (query_end, target_end), score, dropped, states or None: not stated); DEFAULT scores
LITERAL = [
    ("ACGTACGTAC", "ACGTACGTAC", 3, 0, (10, 10), 20, 0, [0] * 10),
    (FORTY + "A" * 30, FORTY + "C" * 30, 8, 0, (40, 40), 80, 1, [0] * 40),
    (FORTY + "A" * 30, FORTY + "C" * 30, 8, 5, (40, 40), 80, 1, [0] * 40),
    (FORTY + "A" * 30, FORTY + "C" * 30, 8, 20, (40, 40), 80, 1, [0] * 40),
    (FORTY + "A" * 30, FORTY + "C" * 30, 8, -1, (40, 40), 80, 0, [0] * 40),
    (ISLAND_Q, ISLAND_T, 8, 17, (20, 20), 40, 1, [0] * 20),
    (ISLAND_Q, ISLAND_T, 8, 18, (56, 56), 76, 0, [0] * 20 + [1] * 6 + [0] * 30),
    (FORTY, DELETED, 8, 50, (40, 35), 56, None, [0] * 20 + [3] * 5 + [0] * 15),
    (FORTY, DELETED, 4, 50, (20, 20), 40, None, [0] * 20),
    ("", "ACG", 64, 200, (0, 0), 0, 0, []),
    ("ACG", "", 64, 200, (0, 0), 0, 0, []),
    ("AAAA", "CCCC", 64, 200, (0, 0), 0, 0, []),
]


def pair(r, max_length, max_error=0.30):
    """A related prefix at 0 .. max_error errors followed by unrelated tails; one pair in four has an island of related
    bases behind the junk, one in four an indel of 5-40 bases near the start; lengths 0 .. max_length"""
    related = random_sequence(r, r.randrange(0, max_length + 1))
    q, t = related, mutate(r, related, r.random() * max_error)
    kind = r.randrange(4)
    if kind == 1 and len(related) > 10:
        at, size = r.randrange(2, 10), r.randrange(5, 41)
        if r.random() < 0.5:
            t = t[:at] + random_sequence(r, size) + t[at:]
        else:
            q = q[:at] + random_sequence(r, size) + q[at:]
    q += random_sequence(r, r.randrange(0, max_length // 2 + 1))
    t += random_sequence(r, r.randrange(0, max_length // 2 + 1))
    if kind == 2:
        island = random_sequence(r, r.randrange(5, 40))
        q, t = q + island, t + island
    return q[:max_length], t[:max_length]


def pairs(seed, count, max_length, max_error=0.30):
    r = random.Random(seed)
    return [pair(r, max_length, max_error) for _ in range(count)]
