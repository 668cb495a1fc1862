"""One-off check of tests/golden/cudamapper_covid.npz (written by the oracle, make_mapper_goldens.py) against the REFERENCE's
own cudamapper kernels on the CPU emulator (oracle/_ref/libref_cudamapper_simt.so): the four COVID_CONFIGS through the
reference's IndexGPU, MatcherGPU and OverlapperTriggered, compared in element count, anchor count and the overlaps'
sha256. Records what it checked in tests/golden/reference_simt_mapper_check.json (tests/test_reference_simt_mapper.py
reads it). usage: python tests/golden/check_mapper_goldens_against_reference.py"""
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mapper_cases as MC  # noqa: E402
import ref_cudamapper as R  # noqa: E402


def main():
    assert R.available(), "build oracle/_ref/libref_cudamapper_simt.so first (make -C oracle all, with the reference checkout)"
    reads = MC.covid_reads()[1]
    golden = np.load(MC.COVID_NPZ)
    configs = []
    for cfg in MC.COVID_CONFIGS:
        t0 = time.time()
        key = "w%d_F%g" % (cfg["w"], cfg["F"])
        idx = R.index(reads, cfg["k"], cfg["w"], True, cfg["F"])
        a = R.anchors(idx, idx)
        o = R.overlaps(a, True, **MC.OVERLAP_PARAMS)
        got = dict(n_elements=len(idx["representations"]), n_anchors=len(a), n_overlaps=len(o),
                   overlaps_sha256=hashlib.sha256(MC.overlap_bytes(o)).hexdigest())
        want = dict(n_elements=int(golden[key + "_n_elements"]), n_anchors=int(golden[key + "_n_anchors"]),
                    n_overlaps=int(golden[key + "_n_overlaps"]), overlaps_sha256=str(golden[key + "_overlaps_sha256"]))
        configs.append(dict(cfg, agrees=got == want, seconds=round(time.time() - t0, 1), **got))
        print(key, "agrees" if got == want else "DIFFERS: reference %s, golden %s" % (got, want), configs[-1]["seconds"], "s")
    with open(MC.REFERENCE_SIMT_CHECK, "w") as f:
        json.dump(dict(what="cudamapper_covid.npz against the reference's kernels on oracle/simt: all 3000 reads, all four configs",
                       configs=configs), f, indent=1)
        f.write("\n")
    assert all(c["agrees"] for c in configs)


if __name__ == "__main__":
    main()
