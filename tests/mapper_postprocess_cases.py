"""Fixtures shared by the cudamapper post-processing tests: the reference's hand-transcribed cases
(cudamapper_postprocess_vectors.json) and what its functions returned on seeded inputs
(cudamapper_postprocess_reference.npz); tests/golden/make_mapper_postprocess_*.py write them."""
import json
import os

import numpy as np

import mapper_cases as MC
from oracle_mapper import OVERLAP

VECTORS = os.path.join(MC.GOLDEN, "cudamapper_postprocess_vectors.json")
REFERENCE = os.path.join(MC.GOLDEN, "cudamapper_postprocess_reference.npz")
CASES = ["fuse", "rescue", "mapped"]
RESCUE_CASES = ["rescue", "mapped"]  # the overlaps of "fuse" lie on no reads


def load_vectors():
    with open(VECTORS) as f:
        return json.load(f)


def load_reference():
    with np.load(REFERENCE) as z:
        return {k: z[k] for k in z.files}


def reads_of(golden, case):
    """(query reads, target reads) of a recorded case, as lists of bytes"""
    nq, nt = (int(x) for x in golden[case + "_n_reads"])
    q = bytes(golden[case + "_queries"]).split(b"\n") if nq else []
    t = bytes(golden[case + "_targets"]).split(b"\n") if nt else []
    assert (len(q), len(t)) == (nq, nt)
    return q, t


def overlaps_from_dicts(records):
    out = np.zeros(len(records), OVERLAP)
    for o, r in zip(out, records):
        for k, v in r.items():
            o[k] = ord(v) if k == "relative_strand" else v
    return out


def fasta_reads(name):
    return MC.read_fasta(os.path.join(MC.GOLDEN, "cudamapper_data", name))[1]
