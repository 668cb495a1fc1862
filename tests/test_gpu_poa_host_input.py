"""cudapoa with the reads left in the pinned staging block (the graph-build kernel fetches them over the link when it stages
a read in LDS, 16 bytes per lane) against the same batch with GW_POA_HOST_INPUT=0 (the reads uploaded, as before) and
against the CPU oracle: consensus, coverage and status agree byte for byte. The switch is read per call, so both arms run
in this process; Batch.last_generate_read_host says which arm a generate_poa() took.

Shapes: read lengths at the edges of the 4-byte padding, the 16-byte fetch and the 1 KB wave-wide request, the longest read
as the last read of the last window (its read-ahead runs into the zeroed slack), a window of one read, bytes outside ACGT,
explicit base weights, a fill of 8 windows followed by reset() and another fill of 4 with nothing fetched in between,
generate_poa() followed by relaunch(), 1100 windows for the persistent grid, a batch whose gap score needs 32-bit scores
(its traceback is the lane-0 walk, which must find the read in LDS as well), and a full-band batch, whose kernel keeps the
copy path."""
import numpy as np
import pytest

import oracle_poa as O

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def _read(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).astype(np.uint8))


def _mutated(rng, read, n):
    """a copy of `read` with a few substitutions, cut or extended to n bases"""
    out = bytearray(read)
    for _ in range(max(1, len(out) // 20)):
        out[int(rng.integers(len(out)))] = b"ACGT"[int(rng.integers(4))]
    if n <= len(out):
        return bytes(out[:n])
    return bytes(out) + _read(rng, n - len(out))


def _edge_windows(seed):
    rng = np.random.default_rng(seed)
    windows = []
    for n in EDGE_LENGTHS:
        backbone = _read(rng, n)
        windows.append([backbone, _mutated(rng, backbone, n), _mutated(rng, backbone, n + 1), _mutated(rng, backbone, max(1, n - 1))])
    windows.append([_read(rng, 100)])  # a window of one read
    odd = _read(rng, 90, b"ACGTNnacgt-*")  # bytes outside ACGT
    windows.append([odd, _mutated(rng, odd, 90), _read(rng, 77, b"ACGTN")])
    # the backbone lengths as later reads of one window, where the staging loop meets them
    windows.append([_read(rng, 40)] + [_read(rng, n) for n in EDGE_LENGTHS[:9]])
    long_one = _read(rng, 1000)
    windows.append([long_one, _mutated(rng, long_one, 1010), _mutated(rng, long_one, 1024)])  # the longest read last of all
    return windows


def _oracle(cfg_args, windows, weights=None, **scores):
    cfg = O.make_cfg(*cfg_args, **scores)
    O.lib().poa_cfg_select_types(cfg)
    out = []
    with O.Workspace(cfg) as ws:
        for i, w in enumerate(windows):
            ref = ws.process(w, None if weights is None else weights[i])
            if ref["status"] == 0:
                out.append((ref["consensus"], [int(v) for v in ref["coverage"]], 0))
            else:
                out.append(("", [], ref["status"]))
    return out


def _fill(batch, windows, weights=None):
    for i, w in enumerate(windows):
        status, per_read = batch.add_poa_group(list(w), None if weights is None else weights[i])
        assert status == 0 and all(s == 0 for s in per_read), (i, status, per_read)


def _results(batch):
    cons, cov, status = batch.get_consensus()
    return [(c, list(v), s) for c, v, s in zip(cons, cov, status)]


def _both_arms(monkeypatch, run, expect_host=True):
    """run(batch-making closure) under host input and under GW_POA_HOST_INPUT=0; returns the two results"""
    monkeypatch.delenv("GW_POA_HOST_INPUT", raising=False)
    got_host, used = run()
    assert used == expect_host
    monkeypatch.setenv("GW_POA_HOST_INPUT", "0")
    got_copy, used = run()
    assert used is False
    monkeypatch.delenv("GW_POA_HOST_INPUT", raising=False)
    return got_host, got_copy


def _batch(max_seq, max_reads, mode, mem=1 << 30, **scores):
    from genomeworks_amd import cudapoa
    return cudapoa.CudaPoaBatch.from_batch_config(max_seq, max_reads, 256, mode, mem, **scores)


def _agree(got_host, got_copy, want):
    assert len(got_host) == len(got_copy) == len(want)
    bad = [i for i in range(len(want)) if not (got_host[i] == got_copy[i] == want[i])]
    assert not bad, (bad[:10], got_host[bad[0]], got_copy[bad[0]], want[bad[0]])


def test_edge_lengths_one_read_window_odd_bytes_and_the_longest_read_last(monkeypatch):
    windows = _edge_windows(11)
    assert len(windows[-1][-1]) == 1024 == max(len(r) for w in windows for r in w)

    def run():
        batch = _batch(1024, 10, "static_band")
        _fill(batch, windows)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run), _oracle((1024, 10, 256, 1), windows))


def test_adaptive_band(monkeypatch):
    windows = _edge_windows(12)[9:]

    def run():
        batch = _batch(1024, 10, "adaptive_band")
        _fill(batch, windows)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run), _oracle((1024, 10, 256, 2), windows))


@pytest.mark.parametrize("mode", ["static_band", "adaptive_band"])
def test_32_bit_scores(monkeypatch, mode):
    """gap -16 with 3072 graph rows: the scores leave int16 (ids stay 16-bit, the tables stay in LDS), the score tile of the
    lane-parallel traceback does not fit the ring, and the walk is lane 0's, read character by read character"""
    windows = _edge_windows(19)[9:]
    want = _oracle((1024, 10, 256, 1 if mode == "static_band" else 2), windows, gap=-16)
    cfg = O.make_cfg(1024, 10, 256, 1, gap=-16)
    O.lib().poa_cfg_select_types(cfg)
    assert cfg.score32 == 1

    def run():
        batch = _batch(1024, 10, mode, gap_score=-16)
        _fill(batch, windows)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run), want)


def test_explicit_base_weights(monkeypatch):
    rng = np.random.default_rng(13)
    windows = _edge_windows(13)[7:12]
    weights = [[None if k == 1 else rng.integers(1, 50, len(r)).astype(np.int8) for k, r in enumerate(w)] for w in windows]

    def run():
        batch = _batch(1024, 10, "static_band")
        _fill(batch, windows, weights)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run), _oracle((1024, 10, 256, 1), windows, weights))


def test_reset_and_a_different_fill_behind_a_launch_nobody_fetched(monkeypatch):
    first, second = _edge_windows(14)[4:12], _edge_windows(15)[8:12]

    def run():
        batch = _batch(1024, 10, "static_band")
        _fill(batch, first)
        batch.generate_poa()
        batch.reset()
        _fill(batch, second)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run), _oracle((1024, 10, 256, 1), second))


def test_generate_then_relaunch(monkeypatch):
    windows = _edge_windows(16)[6:]

    def run():
        batch = _batch(1024, 10, "static_band")
        _fill(batch, windows)
        batch.generate_poa()
        used = batch.last_generate_read_host
        batch.relaunch()
        batch.relaunch()
        return _results(batch), used

    _agree(*_both_arms(monkeypatch, run), _oracle((1024, 10, 256, 1), windows))


def test_1100_windows_on_the_persistent_grid(monkeypatch):
    rng = np.random.default_rng(17)
    windows = []
    for _ in range(1100):
        backbone = _read(rng, 16)
        windows.append([backbone, _mutated(rng, backbone, 16)])

    def run():
        batch = _batch(256, 2, "static_band", 4 << 30)
        assert batch.max_poas >= 1100
        _fill(batch, windows)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run), _oracle((256, 2, 256, 1), windows))


def test_a_full_band_batch_keeps_the_copy_path(monkeypatch):
    windows = [[r[:250] for r in w] for w in _edge_windows(18)[5:]]

    def run():
        batch = _batch(256, 10, "full_band")
        _fill(batch, windows)
        batch.generate_poa()
        return _results(batch), batch.last_generate_read_host

    _agree(*_both_arms(monkeypatch, run, expect_host=False), _oracle((256, 10, 256, 0), windows))
