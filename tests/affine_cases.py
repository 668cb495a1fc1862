"""Cases of the affine-gap aligner's tests: the literal ones of INTEGRATION.md section 3o, and seeded generators."""
import random

DEFAULT = (4, 6, 2)
SCORE_SETS = [(4, 6, 2), (1, 0, 1), (2, 3, 1), (5, 0, 3), (255, 255, 255), (1, 255, 1)]

CLIPPED_Q, CLIPPED_T = "G" * 5 + "A" * 20, "A" * 20 + "G" * 5

# (query, target, (x, o, e), B, states, cost, optimal); states / optimal None: not stated
LITERAL = [
    ("CGCGGA", "CGG", DEFAULT, 8, [0, 3, 3, 3, 0, 1], 16, True),
    ("CAAAAG", "CAAAAAG", DEFAULT, 8, [0, 2, 0, 0, 0, 0, 0], 8, True),
    ("CAAAAAG", "CAAAAG", DEFAULT, 8, [0, 3, 0, 0, 0, 0, 0], 8, True),
    (CLIPPED_Q, CLIPPED_T, DEFAULT, 0, None, 40, False),
    (CLIPPED_Q, CLIPPED_T, DEFAULT, 5, None, 32, True),
    (CLIPPED_Q, CLIPPED_T, DEFAULT, 30, None, 32, True),
    ("", "ACG", DEFAULT, 0, [2, 2, 2], 12, True),
    ("ACG", "", DEFAULT, 0, [3, 3, 3], 12, True),
    ("", "", DEFAULT, 0, [], 0, True),
]


def random_sequence(r, n):
    return "".join(r.choice("ACGT") for _ in range(n))


def mutate(r, q, error_rate):
    """q with substitutions, deleted and inserted bases at about error_rate per base"""
    out = []
    for c in q:
        if r.random() >= error_rate:
            out.append(c)
        else:
            out.append(r.choice(["", r.choice("ACGT"), c + r.choice("ACGT")]))
    return "".join(out)


def pairs(seed, count, max_length, max_error=0.30, truncate=0.1):
    """`count` pairs: a random query of 0 .. max_length bases and a copy with 0 .. max_error errors, one in ten of them
    truncated at a random place"""
    r = random.Random(seed)
    out = []
    for _ in range(count):
        q = random_sequence(r, r.randrange(0, max_length + 1))
        t = mutate(r, q, r.random() * max_error)
        if r.random() < truncate:
            t = t[:r.randrange(0, len(t) + 1)]
        out.append((q, t))
    return out


def pair_with_band(seed, length, difference, error_rate=0.1):
    """a pair with len(target) - len(query) == difference exactly (either sign): W = |difference| + 2 B + 1"""
    r = random.Random(seed)
    q = random_sequence(r, length)
    t = mutate(r, q, error_rate)
    want = length + difference
    while len(t) < want:
        at = r.randrange(0, len(t) + 1)
        t = t[:at] + r.choice("ACGT") + t[at:]
    while len(t) > want:
        at = r.randrange(0, len(t))
        t = t[:at] + t[at + 1:]
    return q, t
