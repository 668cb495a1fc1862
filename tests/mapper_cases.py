"""Inputs shared by the cudamapper tests and tools/bench_mapper.py: the covid read fixture and seeded synthetic reads
(a random genome, reads drawn from both strands with substitutions, insertions and deletions)."""
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
COVID = os.path.join(GOLDEN, "cudamapper_covid_reads.fasta.gz")
VECTORS = os.path.join(GOLDEN, "cudamapper_vectors.json")
COVID_NPZ = os.path.join(GOLDEN, "cudamapper_covid.npz")

# the covid goldens: the reference sample's parameters (w=5) and the CLI defaults (w=10), each with the frequency
# filter of the reference (F=1e-5) and with it off
COVID_CONFIGS = [dict(k=15, w=5, F=1e-5), dict(k=15, w=10, F=1e-5), dict(k=15, w=5, F=1.0), dict(k=15, w=10, F=1.0)]
OVERLAP_PARAMS = dict(min_residues=3, min_overlap_len=250, min_bases_per_residue=1000, min_overlap_fraction=0.8)


def overlap_bytes(overlaps):
    """The fields of OVERLAP records without their padding bytes (which carry no value)."""
    from numpy.lib import recfunctions
    return recfunctions.repack_fields(np.asarray(overlaps)).tobytes()


def read_fasta(path):
    """(names, sequences) of a FASTA file, gzipped or not; names end at the first whitespace"""
    opener = gzip.open if path.endswith(".gz") else open
    names, seqs = [], []
    with opener(path, "rt") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                seqs.append([])
            else:
                seqs[-1].append(line)
    return names, ["".join(s) for s in seqs]


def covid_reads():
    return read_fasta(COVID)


def load_vectors():
    with open(VECTORS) as f:
        return json.load(f)


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def synthetic_reads(seed, genome_length, coverage, mean_length, error_rate, min_length=1):
    """Reads of ~mean_length (uniform in [mean/2, 3 mean/2]) from a random genome of genome_length bases, half of
    them reverse-complemented, each base then mutated with probability error_rate (equal thirds substitution,
    insertion, deletion)."""
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), genome_length)
    n_reads = max(1, int(genome_length * coverage / mean_length))
    reads = []
    for _ in range(n_reads):
        length = int(rng.integers(max(min_length, mean_length // 2), mean_length * 3 // 2 + 1))
        length = min(length, genome_length)
        start = int(rng.integers(0, genome_length - length + 1))
        r = genome[start:start + length]
        u = rng.random(length)
        kind = rng.integers(0, 3, length)
        subs = rng.choice(np.frombuffer(b"ACGT", np.uint8), length)
        keep = ~((u < error_rate) & (kind == 2))
        r = np.where((u < error_rate) & (kind == 0), subs, r)
        ins = (u < error_rate) & (kind == 1)
        out = np.repeat(r, np.where(ins, 2, 1))
        out[np.cumsum(np.where(ins, 2, 1)) - 1] = np.where(ins, subs, r)  # inserted base after the original
        keep = np.repeat(keep, np.where(ins, 2, 1))
        s = out[keep].tobytes()
        if rng.random() < 0.5:
            s = s.translate(_COMP)[::-1]
        reads.append(s.decode())
    return reads


# ---- cases answered by the reference's own kernels on the CPU emulator (oracle/simt) ----------------------------------
# tests/golden/make_mapper_reference_simt_goldens.py runs them through oracle/_ref/libref_cudamapper_simt.so and writes
# REFERENCE_SIMT_NPZ / REFERENCE_SIMT_JSON; tests/test_reference_simt_mapper.py and tests/test_gpu_mapper_reference.py
# build the same inputs again from the case descriptions. Every case is (class, k, w, hash, seed): the reads, indices and
# anchors follow from those alone. k <= 16: the emulator does not reproduce the GPU's shift for k >= 17.

REFERENCE_SIMT_NPZ = os.path.join(GOLDEN, "cudamapper_reference_simt.npz")
REFERENCE_SIMT_JSON = os.path.join(GOLDEN, "cudamapper_reference_simt.json")
REFERENCE_SIMT_CHECK = os.path.join(GOLDEN, "reference_simt_mapper_check.json")
WHOLE_ARRAY_LIMIT = 300  # fixture arrays of more elements are stored as length + sha256 (matcher inputs: always whole)


def central_step(k, w):
    """windows of one step of the reference's find_central_minimizers: 64 threads x 8 bases, held in 16 bits"""
    return ((512 - (k - 1)) - (w - 1)) & 0xffff


def _random_bases(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, np.uint8), n).tobytes()


def _revcomp(b):
    return b.translate(_COMP)[::-1]


def index_case_reads(cls, k, w, seed):
    """The reads (bytes) of an index case."""
    rng = np.random.default_rng([seed, k, w])
    s, one = central_step(k, w), k + w - 1  # bases of a read with one window
    if cls == "multi_step":  # several central steps
        return [_random_bases(rng, int(n)) for n in (600, 5000, int(rng.integers(600, 5000)), int(rng.integers(600, 5000)))]
    if cls == "step_boundary":  # a step boundary at the only, the last and the first window of a step
        return [_random_bases(rng, one - 1 + n) for n in (1, s - 1, s, s + 1, 2 * s + 1)]
    if cls == "stale_carry":  # k + w = 66: minimizers that persist across the step boundary, and low-complexity stretches
        return [_random_bases(rng, 2 * s + 300), _random_bases(rng, 3 * s + 7),
                _random_bases(rng, s - 40) + b"A" * 200 + _random_bases(rng, 300),
                _random_bases(rng, 200) + b"ACG" * 400 + _random_bases(rng, 300),
                _random_bases(rng, s + 10, b"AC") + _random_bases(rng, 2 * s)]
    if cls == "w1":
        return [_random_bases(rng, n) for n in (k, k + 1, 300, 1200)]
    if cls == "end_steps":  # w - 1 against the 64 - (k - 1) windows of a front-end / back-end step
        return [_random_bases(rng, n) for n in (one, one + 1, one + 70, 2 * one + 3, 1500)]
    if cls == "exact_length":  # exactly one and two windows
        return [_random_bases(rng, one), _random_bases(rng, one + 1), _random_bases(rng, one), _random_bases(rng, one + 1)]
    if cls == "short_among_long":  # reads below k + w - 1 are skipped, later ids shift
        return [_random_bases(rng, n) for n in (one - 1, 700, 1, one - 1, one, 0, 900, k, one + 5, one - 2)]
    if cls == "ties":  # homopolymers, tandem repeats of period 1..6, reads equal to their reverse complement
        reads = [bytes([c]) * 700 for c in b"ACGT"]
        reads += [_random_bases(rng, p) * (900 // p) for p in range(1, 7)]
        half = _random_bases(rng, 400)
        reads += [half + _revcomp(half), b"ACGT" * 200, b"AT" * 350, _random_bases(rng, 50) + b"GC" * 300]
        return reads
    if cls == "non_acgt":  # N, lower case, IUPAC letters, bytes >= 0x80
        reads = []
        for alphabet in (b"ACGTN", b"acgtACGT", b"ACGTRYKMSWBDHVN", bytes(range(0x80, 0x100)) + b"ACGT", bytes(range(256))):
            reads.append(_random_bases(rng, 900, alphabet))
        r = bytearray(_random_bases(rng, 1400))
        for at in rng.integers(0, len(r), 40):
            r[int(at)] = int(rng.integers(0, 256))
        return reads + [bytes(r)]
    if cls == "k16":  # the sign-extended top code: k-mers that start with T (forward) or end with A (reverse)
        return [_random_bases(rng, 1200), b"T" * 100 + _random_bases(rng, 600, b"TG") + b"A" * 100, _random_bases(rng, 700, b"TA")]
    if cls in ("filter", "all_filtered"):  # representation counts 1, 2, 3, ...: i copies of the i-th random block
        blocks = [_random_bases(rng, 60) for _ in range(9)]
        return [b"".join(blocks[i] for _ in range(i + 1)) + _random_bases(rng, 40) for i in range(9)] + [b"A" * 300, b"AC" * 200]
    raise ValueError(cls)


def _index_cases():
    cases = []

    def add(cls, k, w, seed, F=1.0, first_read_id=0):
        for h in (True, False):
            cases.append(dict(stage="index", cls=cls, k=k, w=w, hash=h, seed=seed, F=F, first_read_id=first_read_id))

    for i, (k, w) in enumerate([(15, 10), (12, 5), (16, 8)]):
        add("multi_step", k, w, 100 + i)
    for i, (k, w) in enumerate([(15, 10), (15, 5), (16, 50), (9, 3)]):
        add("step_boundary", k, w, 110 + i)
    for i, (k, w) in enumerate([(15, 51), (16, 50), (6, 60)]):
        add("stale_carry", k, w, 120 + i)
    for i, k in enumerate([15, 16, 4]):
        add("w1", k, 1, 130 + i)
    for i, (k, w) in enumerate([(15, 50), (15, 51), (15, 52), (10, 55), (10, 56), (10, 57), (4, 100), (16, 120)]):
        add("end_steps", k, w, 140 + i)  # w - 1 below, at and above 64 - (k - 1); two and three end steps
    for i, (k, w) in enumerate([(15, 10), (16, 50), (4, 1), (5, 70)]):
        add("exact_length", k, w, 150 + i)
    for i, (k, w) in enumerate([(15, 10), (12, 30)]):
        add("short_among_long", k, w, 160 + i, first_read_id=7 * i)
    for i, (k, w) in enumerate([(4, 8), (6, 10), (15, 10), (16, 5), (2, 3), (15, 51)]):
        add("ties", k, w, 170 + i)
    for i, (k, w) in enumerate([(15, 10), (8, 4), (16, 50)]):
        add("non_acgt", k, w, 180 + i)
    for i, w in enumerate([10, 1, 50]):
        add("k16", 16, w, 190 + i)
    return cases


def filter_parameters(reads, k, w, h):
    """filtering_parameter values whose threshold (floor(n F + 0.001)) equals the count of some representation while
    another representation has one element less, from the unfiltered oracle index of the reads"""
    import oracle_mapper as O
    idx = O.index(reads, k, w, h, 1.0)
    n = len(idx["representations"])
    counts = set(np.diff(idx["first_occurrence_of_representations"].astype(np.int64)).tolist())
    out = []
    for c in sorted(counts):
        if c >= 2 and c - 1 in counts:
            F = c / n
            assert int(n * F + 0.001) == c
            out.append(F)
    return out[:2] + out[-2:]


def reference_simt_index_cases():
    cases = _index_cases()
    for i, (k, w) in enumerate([(15, 10), (8, 5)]):
        for h in (True, False):
            reads = index_case_reads("filter", k, w, 200 + i)
            for F in sorted(set(filter_parameters(reads, k, w, h))):
                cases.append(dict(stage="index", cls="filter", k=k, w=w, hash=h, seed=200 + i, F=F, first_read_id=3))
            cases.append(dict(stage="index", cls="all_filtered", k=k, w=w, hash=h, seed=200 + i, F=1e-9, first_read_id=0))
    for n, c in enumerate(cases):
        c["name"] = "index_%03d_%s_k%d_w%d_%s" % (n, c["cls"], c["k"], c["w"], "hashed" if c["hash"] else "plain")
    return cases


def hand_index(read_ids, positions, representations, first_read_id, number_of_reads, longest):
    """An index dict (tests/oracle_mapper.index) from elements already grouped by ascending representation."""
    rep = np.asarray(representations, np.uint64)
    uq, first = np.unique(rep, return_index=True)
    assert np.all(np.diff(rep.astype(np.int64)) >= 0)
    return dict(representations=rep, read_ids=np.asarray(read_ids, np.uint32), positions_in_reads=np.asarray(positions, np.uint32),
                directions=np.zeros(len(rep), np.uint8), unique_representations=uq,
                first_occurrence_of_representations=np.append(first, len(rep)).astype(np.uint32) if len(rep) else np.zeros(0, np.uint32),
                number_of_reads=number_of_reads, smallest_read_id=first_read_id if number_of_reads else 0,
                largest_read_id=first_read_id + number_of_reads - 1 if number_of_reads else 0,
                number_of_basepairs_in_longest_read=longest)


MATCHER_CLASSES = ["self", "disjoint", "query_empty", "target_empty", "first_read_ids", "block_300x300", "wide_position_key"]


def matcher_case_inputs(cls, k, w, h, seed):
    """(query, target): each either dict(reads=..., first_read_id=...) -- an index to build -- or dict(index=...) built by hand"""
    rng = np.random.default_rng([seed, k, w])
    reads = synthetic_reads(seed, 2000, 3, 700, 0.03)
    half = len(reads) // 2
    if cls == "self":
        return dict(reads=reads, first_read_id=0), None
    if cls == "disjoint":
        return dict(reads=["A" * 300, "AC" * 200], first_read_id=0), dict(reads=["C" * 300, "G" * 250], first_read_id=2)
    if cls == "query_empty":
        return dict(reads=["ACGT", "AC"], first_read_id=0), dict(reads=reads[:half], first_read_id=2)
    if cls == "target_empty":
        return dict(reads=reads[:half], first_read_id=0), dict(reads=["ACGT", ""], first_read_id=half)
    if cls == "first_read_ids":
        return dict(reads=reads[:half], first_read_id=5), dict(reads=reads[half:], first_read_id=100)
    if cls == "block_300x300":  # one representation shared 300 x 300 times among others: 90 000 anchors with equal keys
        def side(first):
            rid = np.sort(rng.integers(first, first + 4, 300))
            pos = rng.integers(0, 5000, 300)
            extra = 40
            rep = np.concatenate([np.full(extra // 2, 5), np.full(300, 77), np.full(extra // 2, 90 + first)])
            rid = np.concatenate([np.sort(rng.integers(first, first + 4, extra // 2)), rid, np.sort(rng.integers(first, first + 4, extra // 2))])
            pos = np.concatenate([rng.integers(0, 5000, extra // 2), pos, rng.integers(0, 5000, extra // 2)])
            return dict(index=hand_index(rid, pos, rep, first, 4, 5000))
        return side(0), side(4)
    if cls == "wide_position_key":  # query position x longest target read + target position needs more than 32 bits
        def side(first, longest):
            n = 200
            rep = np.sort(rng.integers(0, 40, n))
            return dict(index=hand_index(rng.integers(first, first + 3, n), rng.integers(0, longest - 20, n), rep, first, 3, longest))
        return side(0, 70000), side(3, 66000)
    raise ValueError(cls)


def reference_simt_matcher_cases():
    cases = []
    for i, cls in enumerate(MATCHER_CLASSES):
        for h in (True, False):
            if cls in ("block_300x300", "wide_position_key") and not h:
                continue  # built by hand: no representation is computed
            cases.append(dict(stage="matcher", cls=cls, k=15, w=10, hash=h, seed=300 + i))
    for n, c in enumerate(cases):
        c["name"] = "matcher_%02d_%s_%s" % (n, c["cls"], "hashed" if c["hash"] else "plain")
    return cases


# the reference's defaults and values that put overlaps on both sides of every condition of the filter
OVERLAPPER_FILTERS = [
    dict(min_residues=3, min_overlap_len=250, min_bases_per_residue=1000, min_overlap_fraction=0.8),
    dict(min_residues=4, min_overlap_len=300, min_bases_per_residue=100, min_overlap_fraction=0.9),
    dict(min_residues=6, min_overlap_len=0, min_bases_per_residue=75, min_overlap_fraction=0.5),
    dict(min_residues=0, min_overlap_len=447, min_bases_per_residue=149, min_overlap_fraction=0.99),
    dict(min_residues=20, min_overlap_len=50, min_bases_per_residue=50, min_overlap_fraction=0.9),
]


def overlapper_case_anchors(seed, n):
    """Sorted anchors on few read pairs whose neighbour steps straddle the chain thresholds (150 in query and |target|), whose
    chains have 2, 3, 4 and more anchors, whose chain starts straddle the fusion threshold (||dq| - |dt|| of 300), with
    rising and falling targets and self pairs."""
    rng = np.random.default_rng(seed)
    out = []
    pairs = sorted(set((int(q), int(t)) for q, t in rng.integers(0, 5, (12, 2))))
    per_pair = max(1, n // len(pairs))
    for q, t in pairs:
        qp, tp = int(rng.integers(0, 300)), int(rng.integers(200000, 300000))
        sign = int(rng.choice([1, -1]))
        m = 0
        while m < per_pair:
            length = int(rng.choice([1, 2, 3, 3, 4, 4, 5, 9, 30]))
            for i in range(length):
                out.append((q, t, qp, tp))
                m += 1
                if i + 1 < length and length == 30:  # a dense chain: few bases per residue
                    qp += int(rng.choice([1, 10, 40]))
                    tp = max(0, tp + sign * int(rng.choice([1, 10, 40])))
                elif i + 1 < length:  # inside a chain
                    qp += int(rng.choice([1, 40, 100, 148, 149]))
                    tp = max(0, tp + sign * int(rng.choice([0, 3, 60, 120, 148, 149])))
            # the step to the next chain: breaks it by the query step, the target step or both; the fusion distance follows
            dq = int(rng.choice([150, 151, 200, 448, 449, 450, 451, 700]))
            dt = int(rng.choice([0, 149, 150, 151, dq - 301, dq - 300, dq - 299, dq - 298, dq + 298, dq + 299, dq + 300, dq + 301, 5000]))
            if dq < 150 and abs(dt) < 150:
                dt = 150
            qp += dq
            tp = max(0, tp + sign * dt)
            if rng.random() < 0.08:
                sign = -sign
    a = np.array(out, dtype=[("query_read_id", "<u4"), ("target_read_id", "<u4"), ("query_position_in_read", "<u4"),
                             ("target_position_in_read", "<u4")])
    return a[np.lexsort((a["target_position_in_read"], a["query_position_in_read"], a["target_read_id"], a["query_read_id"]))]


def unsorted_overlapper_anchors():
    """a query step backwards inside a read pair (the reference asks for sorted anchors only in a debug build)"""
    return np.array([(0, 1, 100, 500), (0, 1, 120, 480), (0, 1, 140, 460), (0, 1, 90, 440), (0, 1, 110, 420), (0, 1, 130, 400),
                     (0, 1, 135, 380), (2, 2, 0, 0), (2, 2, 100, 100), (2, 2, 200, 200), (2, 2, 349, 349)],
                    dtype=[("query_read_id", "<u4"), ("target_read_id", "<u4"), ("query_position_in_read", "<u4"),
                           ("target_position_in_read", "<u4")])


def reference_simt_overlapper_cases():
    cases = []
    for i, (seed, n) in enumerate([(400, 3000), (401, 4000), (402, 2500), (403, 60)]):
        for all_to_all in (True, False):
            for f, filt in enumerate(OVERLAPPER_FILTERS):
                cases.append(dict(stage="overlapper", cls="thresholds", seed=seed, n=n, all_to_all=all_to_all, filter=f))
    for all_to_all in (True, False):
        cases.append(dict(stage="overlapper", cls="query_step_backwards", seed=0, n=11, all_to_all=all_to_all, filter=2))
    for n, c in enumerate(cases):
        c["name"] = "overlapper_%02d_%s_seed%d_%s_filter%d" % (n, c["cls"], c["seed"], "all" if c["all_to_all"] else "qt", c["filter"])
    return cases


def overlapper_case_input(case):
    return unsorted_overlapper_anchors() if case["cls"] == "query_step_backwards" else overlapper_case_anchors(case["seed"], case["n"])


def map_case_reads(case):
    """(queries, targets or None) of an end-to-end case: reads of a small genome, both strands, 3 % errors"""
    reads = synthetic_reads(case["seed"], 4000, 5, 1500, 0.03)
    half = len(reads) // 2
    return (reads[:half], reads[half:]) if case["targets"] else (reads, None)


def reference_simt_map_cases():
    """index -> matcher -> overlapper chained, as map_reads does: hashed, both indices numbered from 0"""
    cases = []
    for i, (k, w, F) in enumerate([(15, 10, 1.0), (15, 51, 1.0), (16, 50, 1.0), (15, 5, 0.01)]):
        for targets in (False, True):
            cases.append(dict(stage="map", cls="end_to_end", k=k, w=w, hash=True, seed=500 + i, F=F, targets=targets, filter=0))
    for n, c in enumerate(cases):
        c["name"] = "map_%02d_k%d_w%d_%s" % (n, c["k"], c["w"], "query_vs_target" if c["targets"] else "all_vs_all")
    return cases


def reference_simt_cases():
    return reference_simt_index_cases() + reference_simt_matcher_cases() + reference_simt_overlapper_cases() + reference_simt_map_cases()


def fixture_put(out, key, array, whole=False):
    """length and sha256 of an array always (out["__meta__"]), the array itself when it is small (or `whole`)"""
    import hashlib
    a = np.ascontiguousarray(array)
    out.setdefault("__meta__", {})[key] = [len(a), hashlib.sha256(a.tobytes()).hexdigest()]
    if whole or len(a) <= WHOLE_ARRAY_LIMIT:
        out[key] = a


class Fixture:
    """the npz written by make_mapper_reference_simt_goldens.py: arrays by key, and one JSON entry with the length and
    digest of every array (stored whole or not) and the cases' scalars"""

    def __init__(self, path=None):
        self.npz = np.load(path or REFERENCE_SIMT_NPZ)
        self.meta = json.loads(str(self.npz["__meta__"]))
        self.files = set(self.npz.files)

    def __getitem__(self, key):
        return self.npz[key]


def fixture_check(fx, key, array, where=""):
    """`array` is what the fixture holds under `key`: the values where they are stored, length and digest always"""
    import hashlib
    a = np.ascontiguousarray(array)
    if key in fx.files:
        assert a.dtype == fx[key].dtype, (where, key, a.dtype, fx[key].dtype)
        np.testing.assert_array_equal(a, fx[key], err_msg="%s %s" % (where, key))
    n, digest = fx.meta[key]
    assert len(a) == n, (where, key, len(a), n)
    assert hashlib.sha256(a.tobytes()).hexdigest() == digest, (where, key, "sha256")


INDEX_ARRAY_NAMES = ("representations", "read_ids", "positions_in_reads", "directions", "unique_representations",
                     "first_occurrence_of_representations")
INDEX_SCALAR_NAMES = ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read")


def fixture_put_index(out, prefix, idx, whole=False):
    for name in INDEX_ARRAY_NAMES:
        fixture_put(out, prefix + name, idx[name], whole)
    out.setdefault("__meta__", {})[prefix + "scalars"] = [int(idx[name]) for name in INDEX_SCALAR_NAMES]


def fixture_check_index(fx, prefix, idx, where="", skip=()):
    for name in INDEX_ARRAY_NAMES:
        if name not in skip:
            fixture_check(fx, prefix + name, idx[name], where)
    assert [int(idx[name]) for name in INDEX_SCALAR_NAMES] == fx.meta[prefix + "scalars"], (where, "scalars")


def fixture_index(fx, prefix):
    """an index dict from a fixture that holds its arrays whole"""
    idx = {name: fx[prefix + name] for name in INDEX_ARRAY_NAMES}
    idx.update(zip(INDEX_SCALAR_NAMES, fx.meta[prefix + "scalars"]))
    return idx
