"""Gap runs of a tile and longer for the consumers of the 64-column tile walk (mapper/gwm_column_walk.hpp), shared by
tests/test_gap_run_cases.py and tests/test_gpu_gap_runs.py. A case is (head, run, tail, strand, run_in_query): with L and
R random strings over CGT of `head` and `tail` bases, long = L + "A" * run + R and short = L + R. With run_in_query false
the query is `short` and the target `long`, so the run is `run` columns of state 2, which the CIGARs here print as I;
with run_in_query true it is the other way round, state 3, printed as D. On '-' the target read is the reverse
complement of the target, so the aligner sees the same two sequences. A occurs nowhere else in the pair: an alignment
with `run` edits has `run` gap columns and nothing but matches besides, every base of `short` then matches a base of
`long` that is no A, in order, and the gap columns are exactly the A's -- "{head}M{run}I{tail}M", or with D, terms of
length 0 left out. Every other alignment has more gap columns, a second run or a mismatch, so the same one is the only
optimum under the affine costs (4, 6, 2) and under the two-piece costs (6, 4, 3, 24, 2) as well.

Each record is the whole of its two reads, reads 2 i and 2 i + 1 of one read set, so every consumer takes the whole
grid in one call and per-read results do not mix. TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle_mapper as O
import pileup_cases as PC

HEADS = (0, 1, 63, 64, 65)
RUNS = (64, 65, 127, 128, 129, 200)
TAILS = (0, 1, 70)
GRID = [(head, run, tail, strand, run_in_query) for head in HEADS for run in RUNS for tail in TAILS if head or tail
        for strand in "+-" for run_in_query in (False, True)]
WINDOW_LENGTHS = (1, 7, 64, 200)
AFFINE = (4, 6, 2, 16)            # a run of 200 at band 16 is 233 diagonals, within both aligners' reach
TWO_PIECE = (6, 4, 3, 24, 2, 16)
SEED = 6400


def cigar_of(head, run, tail, run_in_query):
    """the stated CIGAR of a case"""
    terms = ((head, "M"), (run, "D" if run_in_query else "I"), (tail, "M"))
    return "".join("%d%s" % term for term in terms if term[0])


def grid(cases=None):
    """(reads, records, stated CIGARs) of `cases` (None: GRID): read 2 i is the query of case i, read 2 i + 1 its
    target read"""
    cases = GRID if cases is None else cases
    rng = np.random.default_rng(SEED)
    reads, rows = [], []
    for i, (head, run, tail, strand, run_in_query) in enumerate(cases):
        left, right = ("".join(rng.choice(list("CGT"), n)) for n in (head, tail))
        long, short = left + "A" * run + right, left + right
        query, target = (long, short) if run_in_query else (short, long)
        reads += [query, target if strand == "+" else PC.rc(target)]
        rows.append((2 * i, 2 * i + 1, 0, 0, len(query), len(target), ord(strand), 0, 0))
    return reads, np.array(rows, O.OVERLAP).reshape(-1), [cigar_of(h, r, t, in_q) for h, r, t, _, in_q in cases]


def position(head, run, tail, strand, run_in_query):
    """where a case stands in GRID"""
    return GRID.index((head, run, tail, strand, run_in_query))


def run_positions(case):
    """(read, positions): the read of the case (its place in a pair, 0 the query and 1 the target read) that holds the
    run, and the run's positions in it, forward coordinates of the read: the A's, or on '-' in the target read the T's"""
    head, run, tail, strand, run_in_query = case
    if run_in_query or strand == "+":
        return int(not run_in_query), list(range(head, head + run))
    return 1, list(range(tail, tail + run))


def has_both_neighbours(case):
    """whether the run has a base of the other read on both sides, which is when the pileup counts an insertion"""
    return case[0] > 0 and case[2] > 0


def skipped_windows(rows):
    """how many windows between the first and the last record of one record list have no record"""
    windows = [int(r[1]) for r in rows]
    return windows[-1] - windows[0] + 1 - len(windows) if windows else 0


def tiles_without_aligned_column(states):
    """per tile of 64 columns, whether none of its columns is aligned (state < 2)"""
    return [all(s >= 2 for s in states[at:at + 64]) for at in range(0, len(states), 64)]


# the literals of the three cases worked out on paper, target role at W = 64: (case, [(window, target_first,
# target_last, query_begin, query_end), ...])
LITERAL_1 = ((64, 128, 70, "+", False), [(0, 0, 63, 0, 64), (3, 192, 255, 64, 128), (4, 256, 261, 128, 134)])
LITERAL_2 = ((63, 128, 70, "+", True), [(0, 0, 63, 0, 192), (1, 64, 127, 192, 256), (2, 128, 132, 256, 261)])
LITERAL_3 = ((64, 128, 70, "+", True), [(0, 0, 63, 0, 64), (1, 64, 127, 192, 256), (2, 128, 133, 256, 262)])


def check_literals(target_role_of, target_pile_of, variants_of):
    """The three literals against one source of results: target_role_of(i) gives the target-role records of grid record
    i at W = 64 as tuples (overlap, window, target_first, target_last, query_begin, query_end), target_pile_of(i) the
    (6, length) target-role pileup of its target read, variants_of(i) the VARIANT records of its target read at
    min_count = 1, min_percent = 0."""
    deletion, insertion = PC.CHANNELS.index("deletion"), PC.CHANNELS.index("insertion")
    # 1: 64M128I70M. Target bases 64 to 191 face no query base: windows 1 and 2 have no record, the query goes on at 64
    case, records = LITERAL_1
    i = position(*case)
    assert [tuple(r)[1:] for r in target_role_of(i)] == records
    pile = target_pile_of(i)
    assert pile.shape == (6, 262) and (pile[:5].sum(0) == 1).all()
    assert pile[deletion].nonzero()[0].tolist() == list(range(64, 192)) and not pile[insertion].any()
    # 2: 63M128D70M. Target base 63 is the first behind the run, so window 0 reaches to query base 191: its layer
    # contains the whole run. The run is counted once, behind target base 62, and with 128 bases it is never called
    case, records = LITERAL_2
    i = position(*case)
    assert [tuple(r)[1:] for r in target_role_of(i)] == records
    pile = target_pile_of(i)
    assert pile.shape == (6, 133) and pile[insertion].nonzero()[0].tolist() == [62] and pile[insertion, 62] == 1
    assert len(variants_of(i)) == 0
    # 3: 64M128D70M. The run lies between windows 0 and 1: no record's query range contains any of it
    case, records = LITERAL_3
    i = position(*case)
    got = [tuple(r)[1:] for r in target_role_of(i)]
    assert got == records
    assert all(end <= 64 or begin >= 192 for _, _, _, begin, end in got)


# The window call for the layer selection: one 400-base target over CGT and six reads over its whole length. The
# target's T's are its bases 64 to 191 and nothing else, so that the reads which miss that stretch have one optimal
# alignment, by the argument of the grid with T in the place of A (in a stretch of random C, G and T the 128 gap
# columns could stand in many places); the A's of the reads that carry a run are the only ones of their pairs.
WINDOW_TARGET_LENGTH = 400


def window_call():
    """(reads, [target], records, stated CIGARs): reads 0 and 1 miss the 128 target bases from base 64 on
    (64M128I208M), reads 2 and 3 carry 128 A's behind the target's first 63 bases (63M128D337M: the record of window 0
    at W = 64 spans 192 query bases, more than the 2 W a layer may hold), reads 4 and 5 are exact copies; the second
    read of each kind is reverse-complemented, a '-' record, whose columns run from the target's end."""
    rng = np.random.default_rng(SEED + 1)
    t = "".join(rng.choice(list("CG"), WINDOW_TARGET_LENGTH))
    t = t[:64] + "T" * 128 + t[192:]
    forward = [t[:64] + t[192:], t[:63] + "A" * 128 + t[63:], t]
    reads, rows = [], []
    for kind in forward:
        for strand in "+-":
            rows.append((len(reads), 0, 0, 0, len(kind), len(t), ord(strand), 0, 0))
            reads.append(kind if strand == "+" else PC.rc(kind))
    cigars = ["64M128I208M", "208M128I64M", "63M128D337M", "337M128D63M", "400M", "400M"]
    return reads, [t], np.array(rows, O.OVERLAP).reshape(-1), cigars
