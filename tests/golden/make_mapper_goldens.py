#!/usr/bin/env python3
"""Writes tests/golden/cudamapper_covid.npz with the plain-C oracle (tests/oracle_mapper.c): all-vs-all overlaps of the
covid read fixture for every config of mapper_cases.COVID_CONFIGS (the reference sample's k=15 w=5 and the CLI's
k=15 w=10, each with F=1e-5 and with the filter off), hashed representations, r=3 l=250 b=1000 z=0.8, before any
post-processing; with them the index size and anchor count of each config. Overlap arrays above 1000 records are
kept as their count and the sha256 of their bytes (the file stays small); smaller ones are kept whole as well."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mapper_cases as MC  # noqa: E402
import oracle_mapper as O  # noqa: E402


def main():
    reads = MC.covid_reads()[1]
    out = {}
    for cfg in MC.COVID_CONFIGS:
        key = "w%d_F%g" % (cfg["w"], cfg["F"])
        idx = O.index(reads, cfg["k"], cfg["w"], True, cfg["F"])
        a = O.anchors(idx, idx)
        o = O.overlaps(a, True, **MC.OVERLAP_PARAMS)
        if len(o) <= 1000:
            out[key + "_overlaps"] = o
        out[key + "_n_overlaps"] = np.int64(len(o))
        out[key + "_overlaps_sha256"] = np.array(hashlib.sha256(MC.overlap_bytes(o)).hexdigest())
        out[key + "_n_anchors"] = np.int64(len(a))
        out[key + "_n_elements"] = np.int64(len(idx["representations"]))
        print(key, len(idx["representations"]), len(a), len(o))
    np.savez_compressed(MC.COVID_NPZ, **out)


if __name__ == "__main__":
    main()
