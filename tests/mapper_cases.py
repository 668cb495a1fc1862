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
