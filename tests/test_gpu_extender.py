"""cudaextender on the GPU (libcudaextender.so): the reference's end-to-end known answer through Python (host and
device pointers) and through the C++ sample, the device compact / sort / unique step on hand-built segment lists, a
fixed-seed random sweep against the CPU oracle, and the Extender's life cycle."""
import os
import subprocess

import numpy as np
import pytest

import extender_cases as K
import oracle_extender as X

pytestmark = pytest.mark.gpu


def _ext(matrix, xdrop, no_entropy, **kw):
    from genomeworks_amd import cudaextender
    return cudaextender.UngappedXDropExtender(matrix, xdrop, no_entropy, **kw)


def _rows(segments):
    return X.rows(segments)


@pytest.fixture(scope="module")
def sample():
    return K.load_sample()


def test_sample_host_api_equals_golden(sample):
    e = _ext(sample["score_matrix"], sample["xdrop"], sample["no_entropy"])
    got = e.extend(sample["sequence"], sample["sequence"], sample["score_threshold"], sample["seeds"])
    assert _rows(got) == sample["expected"]


def test_sample_device_api_equals_golden(sample):
    import torch
    e = _ext(sample["score_matrix"], sample["xdrop"], sample["no_entropy"])
    seq = torch.from_numpy(sample["sequence"]).cuda()
    seeds = torch.from_numpy(sample["seeds"].astype(np.int32)).cuda()
    got = e.extend(seq, seq, sample["score_threshold"], seeds)
    assert _rows(got) == sample["expected"]


def test_sample_chunked_equals_oracle(sample):
    """Chunks are sorted and de-duplicated on their own, then appended (the oracle states the same)."""
    e = _ext(sample["score_matrix"], sample["xdrop"], sample["no_entropy"])
    e.set_chunk_size(50000)
    args = (sample["sequence"], sample["sequence"], sample["score_matrix"], sample["xdrop"], sample["score_threshold"],
            sample["no_entropy"], sample["seeds"])
    got = e.extend(sample["sequence"], sample["sequence"], sample["score_threshold"], sample["seeds"])
    assert _rows(got) == X.rows(X.extend(*args, chunk=50000))


@pytest.mark.parametrize("mode", ["host", "device"])
def test_cpp_sample_equals_golden(sample, tmp_path, mode):
    from test_extender_headers import build_sample
    exe = build_sample(tmp_path)
    letters = np.array(list("ACGTaNX&"))
    seq = "".join(letters[sample["sequence"]])
    fa = tmp_path / "sample.fa"
    fa.write_text(">chr1\n" + "\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + "\n")
    csv = tmp_path / "seeds.csv"
    csv.write_text("".join("%d,%d\n" % (t, q) for t, q in sample["seeds"]))
    mat = tmp_path / "scores.txt"
    mat.write_text(" ".join(str(int(v)) for v in sample["score_matrix"]) + "\n")
    cmd = [exe, "-p", "-m", str(mat), "-x", str(sample["xdrop"]), "-t", str(sample["score_threshold"])]
    cmd += (["-d"] if mode == "device" else []) + [str(fa), str(fa), str(csv)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(v) for v in line.split(",")) for line in r.stdout.split()]
    assert got == sample["expected"]


@pytest.mark.parametrize("case", K.extend_cases(), ids=lambda c: c[0])
def test_known_answers(case):
    name, T, Q, M, xdrop, thr, no_entropy, seeds, expected = case
    e = _ext(M, xdrop, no_entropy)
    from genomeworks_amd.cudaextender import encode_sequence
    assert _rows(e.extend(encode_sequence(Q), encode_sequence(T), thr, seeds)) == expected


@pytest.mark.parametrize("case", K.sort_unique_cases(), ids=lambda c: c[0])
def test_device_sort_unique_hook(case):
    from genomeworks_amd.cudaextender import sort_unique_device
    name, segs, keep, expected = case
    arr = np.array([(q, t, l, s) for (t, q, l, s) in segs], X.SEGMENT)
    assert _rows(sort_unique_device(arr, keep)) == expected


def test_device_sort_unique_random_against_oracle():
    rng = np.random.default_rng(5)
    n = 30000
    t = rng.integers(0, 3000, n)
    q = np.clip(t + rng.integers(-20, 21, n), 0, None)  # few diagonals: many overlaps
    segs = np.zeros(n, X.SEGMENT)
    segs["target"], segs["query"] = t, q
    segs["length"] = rng.integers(-1, 200, n)
    segs["score"] = rng.integers(0, 5000, n)
    keep = rng.random(n) < 0.8
    from genomeworks_amd.cudaextender import sort_unique_device
    assert _rows(sort_unique_device(segs, keep)) == X.rows(X.sort_unique(segs[keep]))


def _random_matrix(rng):
    m = rng.integers(-150, -20, 64).astype(np.int32)
    for b in range(4):
        m[9 * b] = rng.integers(60, 120)
    m[32:40] = m[40:48] = -1000
    m[4::8] = m[5::8] = -1000
    m[56:64] = m[7::8] = -9000
    return m


def _mutate(rng, s, rate):
    s = s.copy()
    hit = rng.random(s.size) < rate
    s[hit] = rng.integers(0, 4, hit.sum())
    return s


def test_random_sweep_against_oracle():
    """Fixed-seed sweep: several matrices and X from 50 to 5000, entropy on and off, |Q| != |T|, seeds on negative
    diagonals and at both edges, a 20 kbp identical run (an extension over 300 tiles), zero seeds, all-negative
    neighbourhoods and N/L/X/E symbols."""
    from genomeworks_amd import cudaextender
    rng = np.random.default_rng(20261016)
    checked = 0
    for it in range(24):
        M = _random_matrix(rng) if it % 3 else K.load_sample()["score_matrix"]
        xdrop = int(rng.choice([50, 200, 910, 2000, 5000]))
        no_entropy = bool(it % 2)
        tlen = int(rng.integers(500, 6000))
        T = rng.integers(0, 4, tlen).astype(np.int8)
        # query: a mutated copy of a window of T, shifted, plus random flanks (|Q| != |T|)
        a = int(rng.integers(0, tlen // 2))
        Q = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 300))).astype(np.int8),
                            _mutate(rng, T[a:], float(rng.choice([0.0, 0.02, 0.1, 0.3])))])
        if it % 4 == 1:  # special symbols sprinkled in
            for arr in (T, Q):
                idx = rng.integers(0, arr.size, arr.size // 50)
                arr[idx] = rng.integers(4, 8, idx.size)
        if it % 6 == 5:  # all-negative neighbourhood: every column mismatches
            Q = ((T[: Q.size] + 1) % 4).astype(np.int8) if Q.size <= T.size else ((np.resize(T, Q.size) + 1) % 4).astype(np.int8)
        n = 0 if it == 7 else int(rng.integers(1, 3000))
        st = rng.integers(0, tlen, n)
        sq = rng.integers(0, Q.size, n)
        edges = np.array([[0, 0], [tlen - 1, Q.size - 1], [0, Q.size - 1], [tlen - 1, 0], [tlen, 0], [0, Q.size]])
        seeds = np.concatenate([np.stack([st, sq], 1), edges]) if n else np.zeros((0, 2), np.int64)
        thr = int(rng.choice([0, 300, 1000, 3000]))
        e = cudaextender.UngappedXDropExtender(M, xdrop, no_entropy)
        got = _rows(e.extend(Q, T, thr, seeds))
        want = X.rows(X.extend(T, Q, M, xdrop, thr, no_entropy, seeds))
        assert got == want, "iteration %d: %d rows vs %d" % (it, len(got), len(want))
        checked += len(want)
    # a 20 kbp identical run: one extension of > 300 tiles each way
    run = np.random.default_rng(1).integers(0, 4, 20000).astype(np.int8)
    M = K.matrix()
    seeds = [(10000, 10000), (0, 0), (19999, 19999), (5, 7)]
    for no_entropy in (False, True):
        e = cudaextender.UngappedXDropExtender(M, 100, no_entropy)
        got = _rows(e.extend(run, run, 1000, seeds))
        assert got == X.rows(X.extend(run, run, M, 100, 1000, no_entropy, seeds))
        assert got[0] == (0, 0, 19999, 200000)
    assert checked > 100


def test_life_cycle():
    import torch
    from genomeworks_amd import cudaextender as CE
    s = K.load_sample()
    seq, M = s["sequence"], s["score_matrix"]
    stream = torch.cuda.Stream()
    e = CE.UngappedXDropExtender(M, s["xdrop"], s["no_entropy"], stream=stream)
    # sync / results before any host-pointer extend
    assert e.sync() == CE.invalid_operation
    with pytest.raises(CE.ExtenderError):
        e.get_scored_segment_pairs()
    # two extend calls on one extender: each result stands alone
    first = _rows(e.extend(seq, seq, s["score_threshold"], s["seeds"][:40000]))
    second = _rows(e.extend(seq, seq, s["score_threshold"], s["seeds"]))
    assert second == s["expected"]
    assert first == X.rows(X.extend(seq, seq, M, s["xdrop"], s["score_threshold"], False, s["seeds"][:40000]))
    # reset drops the host results
    e.reset()
    assert e.sync() == CE.invalid_operation
    # zero seeds: success, no rows
    assert len(e.extend(seq, seq, s["score_threshold"], np.zeros((0, 2), np.int64))) == 0
    # invalid input: null pointers, negative lengths
    assert e.extend_async_device(0, 10, 0, 10, 100, 0, 1, 0, 0) == CE.invalid_input
    q = torch.from_numpy(seq).cuda()
    out = torch.empty((4, 4), dtype=torch.int32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    sd = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    assert e.extend_async_device(q.data_ptr(), -1, q.data_ptr(), 10, 100, sd.data_ptr(), 1, out.data_ptr(),
                                 cnt.data_ptr()) == CE.invalid_input
    assert e.extend_async_device(q.data_ptr(), 10, q.data_ptr(), 10, 100, sd.data_ptr(), -1, out.data_ptr(),
                                 cnt.data_ptr()) == CE.invalid_input
    assert e.extend_async_device(q.data_ptr(), 10, q.data_ptr(), 10, 100, sd.data_ptr(), 1, out.data_ptr(),
                                 0) == CE.invalid_input
    # unsupported matrix size / extension type are rejected at creation
    with pytest.raises(CE.ExtenderError):
        CE.UngappedXDropExtender(M[:63], 910, False)
    with pytest.raises(CE.ExtenderError):
        CE.UngappedXDropExtender(M, 910, False, extension_type=1)
    del e
    torch.cuda.synchronize()
