"""Inputs of the chaining-overlapper tests (tests/test_mapper_chain_oracle.py, tests/test_gpu_mapper_chain.py) and of
tools/bench_mapper_chain.py: hand-built anchor groups at every edge of rules C1-C8, seeded random groups, and reads
with a known origin. Every case is (name, anchors, keyword arguments of chain_overlaps)."""
import numpy as np

from oracle_mapper import ANCHOR

# a filter that keeps every candidate, so that the records show what the chaining did
KEEP_ALL = dict(min_residues=1, min_overlap_len=0, min_bases_per_residue=1 << 40, min_overlap_fraction=-1.0)


def anchors_of(rows):
    """ANCHOR array of (query read, target read, query position, target position) rows, sorted as the matcher sorts"""
    a = np.array([tuple(int(v) for v in r) for r in rows], ANCHOR) if len(rows) else np.zeros(0, ANCHOR)
    return a[np.lexsort((a["target_position_in_read"], a["query_position_in_read"], a["target_read_id"],
                         a["query_read_id"]))]


def group(positions, qid=0, tid=1):
    return [(qid, tid, q, t) for q, t in positions]


def random_group(rng, m, qid, tid):
    """m anchors of one read pair: a '+' diagonal and a '-' diagonal with jitter (steps that straddle the band), repeat
    hits beside them and scattered noise"""
    rows = []
    n_plus, n_minus = int(m * rng.uniform(0.2, 0.5)), int(m * rng.uniform(0.1, 0.4))
    q, t = int(rng.integers(0, 500)), int(rng.integers(0, 3000))
    for _ in range(n_plus):
        rows.append((q, t))
        step = int(rng.integers(1, 90))
        q, t = q + step, t + step + int(rng.choice([0, 0, 0, 1, -1, 3, -7, 40, 120])) * int(rng.random() < 0.4)
        t = max(t, 0)
    q, t = int(rng.integers(0, 500)), int(rng.integers(8000, 12000))
    for _ in range(n_minus):
        rows.append((q, t))
        step = int(rng.integers(1, 90))
        q, t = q + step, max(0, t - step - int(rng.choice([0, 0, 2, -2, 25, 90])) * int(rng.random() < 0.4))
    while len(rows) < m:
        if rows and rng.random() < 0.3:  # a repeat hit: the same query position again, or the same target position
            bq, bt = rows[int(rng.integers(0, len(rows)))]
            rows.append((bq, int(rng.integers(0, 12000))) if rng.random() < 0.5 else (int(rng.integers(0, 6000)), bt))
        else:
            rows.append((int(rng.integers(0, 6000)), int(rng.integers(0, 12000))))
    return group(rows[:m], qid, tid)


def group_size_cases():
    out = []
    for m in (1, 2, 3, 63, 64, 65, 66, 128, 129, 200):
        rows = random_group(np.random.default_rng([7, m]), m, 0, 1)
        out.append(("size_%d" % m, anchors_of(rows), dict(KEEP_ALL)))
        out.append(("size_%d_S0_M64" % m, anchors_of(rows), dict(KEEP_ALL, min_chain_score=0, max_chains=64)))
        # a clean diagonal of m anchors through the default filter
        out.append(("diagonal_%d" % m, anchors_of(group([(100 + 40 * i, 700 + 40 * i) for i in range(m)])), {}))
    return out


def look_back_cases():
    """X, then `decoys` anchors that precede nothing in '+', then Y on X's diagonal: X is 64 back (taken) or 65 back"""
    out = []
    for decoys in (63, 64):
        rows = [(100, 100)] + [(101 + i, 10 ** 6 - 10 * i) for i in range(decoys)] + [(1000, 1000)]
        out.append(("look_back_%d" % (decoys + 1), anchors_of(group(rows)),
                    dict(KEEP_ALL, min_chain_score=0, max_chains=64)))
    return out


def tie_cases():
    free = dict(KEEP_ALL, min_chain_score=0, max_chains=4)
    return [
        # both predecessors give 15 + 9: the nearer one, (100, 160), wins
        ("tie_equal_predecessors", anchors_of(group([(100, 100), (100, 160), (200, 230)])), free),
        # gain 0 (cost(80) = 15): best == k starts a new chain; gain 1 (cost(79) = 14) chains
        ("tie_best_equals_k", anchors_of(group([(100, 100), (200, 280)])), free),
        ("tie_best_above_k", anchors_of(group([(100, 100), (200, 279)])), free),
        # two chain ends of f = 30: the one of smaller index goes first, and alone with M = 1
        ("tie_equal_ends", anchors_of(group([(100, 100), (150, 150), (1000, 9000), (1050, 9050)])), free),
        ("tie_equal_ends_M1", anchors_of(group([(100, 100), (150, 150), (1000, 9000), (1050, 9050)])),
         dict(free, max_chains=1)),
    ]


def bound_cases():
    """pairs of anchors, one read pair each, on both sides of every bound of C3 (G = 1000, B = 100), in both
    orientations"""
    steps = [(1000, 1000), (1001, 1001), (1001, 1000), (1000, 1001), (950, 1000), (500, 600), (500, 601), (600, 500),
             (601, 500), (0, 100), (100, 0), (1, 1), (0, 0)]
    rows = []
    for n, (dq, dt) in enumerate(steps):
        rows += group([(100, 5000), (100 + dq, 5000 + dt)], 0, 1 + 2 * n)
        rows += group([(100, 5000), (100 + dq, 5000 - dt)], 0, 2 + 2 * n)
    a = anchors_of(rows)
    free = dict(KEEP_ALL, min_chain_score=0, max_chains=4, max_gap=1000)
    exact = anchors_of([r for n, (dq, dt) in enumerate([(500, 500), (500, 501), (501, 500)])
                        for r in group([(100, 5000), (100 + dq, 5000 + dt)], 0, 1 + 2 * n) +
                        group([(100, 5000), (100 + dq, 5000 - dt)], 0, 2 + 2 * n)])
    wide = anchors_of(group([(5, 2 ** 32 - 5), (2 ** 31 + 10, 2 ** 31 - 30), (2 ** 32 - 2, 1)]) +
                      group([(5, 7), (2 ** 31 + 4, 2 ** 31 + 6), (2 ** 32 - 2, 2 ** 32 - 3)], 0, 2) +
                      # target steps of -(2^32 - 6) and 2^32 - 6: 6 in 32-bit arithmetic
                      group([(5, 2 ** 32 - 5), (20, 1)], 0, 3) + group([(5, 1), (20, 2 ** 32 - 5)], 0, 4))
    return [("bounds_G1000_B100", a, dict(free, bandwidth=100)),
            ("bounds_G1_B0", a, dict(free, max_gap=1, bandwidth=0)),
            ("bounds_B0", exact, dict(free, bandwidth=0)),
            # positions at the ends of uint32: the differences must not wrap; the largest gap and band
            ("bounds_uint32", wide, dict(free, max_gap=2 ** 31 - 1, bandwidth=2 ** 31 - 1)),
            ("bounds_uint32_kmer32", wide, dict(free, kmer_size=32, max_gap=2 ** 31 - 1, bandwidth=2 ** 31 - 1))]


def orientation_cases():
    minus = group([(100 + 50 * i, 9000 - 50 * i) for i in range(12)])
    crossing = group([(600 + 50 * i, 1100 + 50 * i) for i in range(-10, 11)] +
                     [(600 + 50 * i, 1100 - 50 * i) for i in range(-10, 11) if i != 0])
    return [("pure_minus", anchors_of(minus), {}),
            ("pure_minus_keep_all", anchors_of(minus), dict(KEEP_ALL)),
            ("crossing", anchors_of(crossing), {}),
            ("crossing_keep_all", anchors_of(crossing), dict(KEEP_ALL, max_chains=64, min_chain_score=0))]


def fork_anchors():
    """a trunk of 5, branch A of 3 on its diagonal (end f = 120), branch B of 3 beside it (f = 72, 87, 102: cut at the
    trunk it scores 102 - 75 = 27), and a chain of 3 far away (f = 45)"""
    trunk = [(100 * i, 100 * i) for i in range(5)]
    a = [(500 + 100 * j, 500 + 100 * j) for j in range(3)]
    b = [(550 + 100 * j, 450 + 100 * j) for j in range(3)]
    far = [(5000 + 100 * j, 50000 + 100 * j) for j in range(3)]
    return anchors_of(group(trunk + a + b + far))


def extraction_cases():
    a = fork_anchors()
    out = []
    for s in (0, 20, 27, 28, 40):
        for m in (1, 2, 3, 64):
            out.append(("fork_S%d_M%d" % (s, m), a, dict(KEEP_ALL, min_chain_score=s, max_chains=m)))
    return out


def interleaved_diagonals():
    """two collinear diagonals of 6 anchors each that alternate in sort order; every neighbour step has |dt| of about
    8000, so the triggered overlapper sees no chain at all"""
    d1 = [(100 + 200 * i, 1000 + 200 * i) for i in range(6)]
    d2 = [(200 + 200 * i, 9000 + 200 * i) for i in range(6)]
    return anchors_of(group(d1 + d2))


def many_groups(seed=11, n_groups=300):
    """about 300 groups of 1..150 anchors; every few groups a size is chosen so that the next group starts on, one
    before or one behind a multiple of 64 or of 256; one group is a read against itself"""
    rng = np.random.default_rng(seed)
    rows, total = [], 0
    for g in range(n_groups):
        m = int(rng.integers(1, 151))
        if g % 4 == 1:
            unit = 256 if g % 8 == 1 else 64
            want = (-total) % unit + int(rng.choice([-1, 0, 1]))
            m = want if 1 <= want <= 150 else (want + unit if want < 1 else m)
        qid, tid = g // 20, g % 20 + (0 if g == 45 else 100)
        if g == 45:
            qid = tid = 2  # sorts in front of (2, 100 ...): a self group
        rows += random_group(rng, m, qid, tid)
        total += m
    return anchors_of(rows)


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def reads_with_origin(seed, genome_length=20000, n_reads=40, shortest=2000, longest=3000, error_rate=0.10):
    """(reads, origin): reads drawn from both strands of a random genome, every base then substituted, followed by an
    inserted base or deleted with probability error_rate / 3 each; origin[i] = (start, end, reversed) in the genome"""
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), genome_length)
    reads, origin = [], []
    for _ in range(n_reads):
        length = int(rng.integers(shortest, longest + 1))
        start = int(rng.integers(0, genome_length - length + 1))
        out = bytearray()
        for base in genome[start:start + length].tolist():
            u = rng.random()
            if u < error_rate / 3:
                out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            elif u < 2 * error_rate / 3:
                out.append(base)
                out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            elif u >= error_rate:
                out.append(base)
        reverse = bool(rng.random() < 0.5)
        s = bytes(out)
        reads.append((s.translate(_COMP)[::-1] if reverse else s).decode())
        origin.append((start, start + length, reverse))
    return reads, origin


def true_pairs(origin, least=1000):
    """{(i, j): strand} for i != j whose origins share at least `least` bases of the genome"""
    out = {}
    for i, (s1, e1, r1) in enumerate(origin):
        for j, (s2, e2, r2) in enumerate(origin):
            if i != j and min(e1, e2) - max(s1, s2) >= least:
                out[(i, j)] = "+" if r1 == r2 else "-"
    return out


SYNTHETIC_SEED = 5


def all_cases():
    return (group_size_cases() + look_back_cases() + tie_cases() + bound_cases() + orientation_cases() +
            extraction_cases() +
            [("interleaved_M2", interleaved_diagonals(), dict(max_chains=2)),
             ("interleaved_M1", interleaved_diagonals(), dict(max_chains=1))])
