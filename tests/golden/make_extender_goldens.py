"""Regenerates tests/golden/cudaextender_sample.npz from the reference checkout's cudaextender data: the sample sequence
(encoded), its seed pairs, the 1 337 expected scored segment pairs and the parameters of the reference's end-to-end test
(score matrix, X-drop 910, score threshold 3000, entropy on). Skips when the reference checkout is absent.

    python tests/golden/make_extender_goldens.py [reference_root]
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_extender as X  # noqa: E402

OUT = os.path.join(HERE, "cudaextender_sample.npz")


def main(ref):
    data = os.path.join(ref, "cudaextender", "data")
    if not os.path.isdir(data):
        print("reference cudaextender data not present at %s: nothing to do" % data)
        return 0
    with open(os.path.join(data, "sample.fa")) as f:
        seq = "".join(l.strip() for l in f if not l.startswith(">"))
    seeds = np.loadtxt(os.path.join(data, "sample_seed_pairs.csv"), delimiter=",", dtype=np.int64).reshape(-1, 2)
    expected = np.loadtxt(os.path.join(data, "sample_scored_segment_pairs.csv"), delimiter=",", dtype=np.int64).reshape(-1, 4)
    # the parameters of the end-to-end test, read as numbers out of the test's text
    with open(os.path.join(ref, "cudaextender", "tests", "Test_CudaextenderEnd2End.cu")) as f:
        text = f.read()
    body = re.search(r"score_matrix\[NUC2\]\s*=\s*\{([^}]*)\}", text).group(1)
    matrix = np.array([int(v) for v in body.replace("\n", " ").split(",")], np.int32)
    assert matrix.size == 64
    xdrop = int(re.search(r"xdrop_threshold\s*=\s*(-?\d+)", text).group(1))
    thr = int(re.search(r"score_threshold\s*=\s*(-?\d+)", text).group(1))
    no_entropy = re.search(r"no_entropy\s*=\s*(true|false)", text).group(1) == "true"
    encoded = X.encode(seq)
    # seeds delta-encoded along the file's order (they are nearly sorted): compresses ~4x better
    deltas = np.diff(seeds, axis=0, prepend=np.zeros((1, 2), np.int64)).astype(np.int32)
    np.savez_compressed(OUT, sequence=encoded, seed_deltas=deltas, expected=expected.astype(np.int32),
                        score_matrix=matrix, xdrop=np.int32(xdrop), score_threshold=np.int32(thr),
                        no_entropy=np.bool_(no_entropy))
    got = X.rows(X.extend(encoded, encoded, matrix, xdrop, thr, no_entropy, seeds))
    print("wrote %s: %d bp, %d seeds, %d expected rows; oracle %s" % (
        OUT, encoded.size, len(seeds), len(expected), "agrees" if got == [tuple(r) for r in expected.tolist()] else "DIFFERS"))
    return 0


def load(path=OUT):
    """dict(sequence int8, seeds [N,2] target/query int64, expected [K,4] target/query/length/score, score_matrix,
    xdrop, score_threshold, no_entropy)"""
    z = np.load(path)
    return dict(sequence=z["sequence"], seeds=np.cumsum(z["seed_deltas"].astype(np.int64), axis=0),
                expected=z["expected"], score_matrix=z["score_matrix"], xdrop=int(z["xdrop"]),
                score_threshold=int(z["score_threshold"]), no_entropy=bool(z["no_entropy"]))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GW_REFERENCE", "/root/reference")))
