"""Seeded inputs of the infix / prefix alignment tests (CPU model and GPU). TEST INFRASTRUCTURE ONLY.

Query lengths sit on the boundaries of the ends scan (genomeworks_amd/semiglobal/gws_ends.hip): a word is 32 bases, a
round 64 words = 2 048 bases, 4 100 bases take a third round. Target lengths per query length n: 1, n - 5, n, 3 n."""
import random

QUERY_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4100]
SMALL_LENGTHS = [n for n in QUERY_LENGTHS if n < 2047]
LARGE_LENGTHS = [n for n in QUERY_LENGTHS if n >= 2047]


def target_lengths(n):
    return sorted({m for m in (1, n - 5, n, 3 * n) if m > 0})


def bases(rng, length):
    return "".join(rng.choice("ACGT") for _ in range(length))


def mutate(rng, s, rate):
    """About rate * len(s) unit edits (substitutions, insertions, deletions), at least one."""
    out = list(s)
    for _ in range(max(1, int(len(s) * rate))):
        kind, at = rng.randrange(3), rng.randrange(len(out) + 1)
        if kind == 0 and at < len(out):
            out[at] = rng.choice([b for b in "ACGT" if b != out[at]])
        elif kind == 1:
            out.insert(at, rng.choice("ACGT"))
        elif out and at < len(out) and len(out) > 1:
            del out[at]
    return "".join(out)


def planted(rng, n, where, edits):
    """(query, target, begin): a query of n bases cut from the 'start', 'middle' or 'end' of a random target of 3 n bases,
    then given 5 % edits when `edits`."""
    target = bases(rng, 3 * n)
    begin = {"start": 0, "middle": n, "end": 2 * n}[where]
    query = target[begin:begin + n]
    return (mutate(rng, query, 0.05) if edits else query), target, begin


def sized_pair(rng, n, m):
    """A query of n bases and a target of m bases that share what fits: the target is the query with 5 % edits, cut or
    extended with random bases at both ends to m."""
    query = bases(rng, n)
    core = mutate(rng, query, 0.05)
    if m <= len(core):
        at = rng.randrange(len(core) - m + 1)
        return query, core[at:at + m]
    left = rng.randrange(m - len(core) + 1)
    return query, bases(rng, left) + core + bases(rng, m - len(core) - left)


def mixed_batch(seed, count=132):
    """`count` pairs of mixed lengths: every small query length in turn, and each large one three times, with the target
    lengths of the list in turn."""
    rng = random.Random(seed)
    lengths = [n for n in LARGE_LENGTHS for _ in range(3)]
    k = 0
    while len(lengths) < count:
        lengths.append(SMALL_LENGTHS[k % len(SMALL_LENGTHS)])
        k += 1
    rng.shuffle(lengths)
    pairs = []
    for i, n in enumerate(lengths):
        ms = target_lengths(n)
        pairs.append(sized_pair(rng, n, ms[i % len(ms)]))
    return pairs
