"""The incremental Kahn order of the LDS kernels (topsort_kahn_incr_lds) keeps the queue's front in registers, does an
ordinary step in one LDS round trip and starts a replayed block's loads next to it. The decisions are those of
oracle/topsort_incr_model.inc; these tests drive model and kernel through every branch of that phase: ordinary steps,
blocks, the element-wise queue compare, nodes with more than three out-edges, queue lengths past the 4-bit field and
a queue longer than the 64 lanes of the register window.

Inputs come from a seeded pure-Python generator (a backbone plus substitution / insertion / deletion per base), so the
CPU half needs nothing but the C oracle."""
import random

import pytest

import oracle_poa as O
from genomeworks_amd import debug_flags as D

BAND = {"full_band": 0, "static_band": 1, "adaptive_band": 2, "static_band_traceback": 3}
BASES = "ACGT"


def _backbone(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _edited(rng, backbone, rate):
    """One read: every base is substituted, followed by an insertion, or deleted with probability rate / 3 each."""
    out = []
    for c in backbone:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice(BASES))
        elif x < 2 * rate / 3:
            out.append(c + "".join(rng.choice(BASES) for _ in range(rng.randrange(1, 4))))
        elif x < rate:
            continue
        else:
            out.append(c)
    return "".join(out)


def high_degree_windows(n=8, seed=99):
    """Many reads that each carry a different base, insertion or deletion at the same six backbone positions (nodes with
    more than three and more than six out-edges, wide queues); every second window with reads cut at both ends."""
    rng = random.Random(seed)
    windows = []
    for k in range(n):
        backbone = _backbone(rng, rng.choice([200, 400]))
        reads = [backbone]
        hot = sorted(rng.sample(range(20, len(backbone) - 20), 6))
        for _ in range(rng.choice([12, 24, 31])):
            s = list(backbone)
            for h in hot:
                kind = rng.randrange(4)
                if kind == 0:
                    s[h] = rng.choice(BASES)
                elif kind == 1:
                    s[h] = s[h] + _backbone(rng, rng.randrange(1, 12))
                elif kind == 2:
                    for d in range(rng.randrange(1, 9)):
                        s[h + d] = ""
            t = "".join(s)
            a, b = rng.randrange(0, 8), rng.randrange(0, 8)
            reads.append(t[a:len(t) - b] if k % 2 else t)
        windows.append(reads)
    return windows


def small_windows(n=16, seed=4242):
    """40-300 bp, 3-17 reads, 2-25 % edits; every second window with reads that begin and end differently."""
    rng = random.Random(seed)
    windows = []
    for k in range(n):
        backbone = _backbone(rng, rng.randrange(40, 301))
        rate = rng.uniform(0.02, 0.25)
        reads = [backbone] + [_edited(rng, backbone, rate) for _ in range(rng.randrange(2, 17))]
        if k % 2:
            reads = [("GATTACA"[: rng.randrange(8)] + r)[rng.randrange(5):len(r) + 7 - rng.randrange(5)] for r in reads]
        windows.append(reads)
    return windows


def branch_window(backbone_len, reads, insert_len, seed):
    """`reads` reads that each carry a different insertion of `insert_len` bases behind one backbone position: as many
    parallel branches in the graph, and a Kahn queue as long while they are walked."""
    rng = random.Random(seed)
    backbone = _backbone(rng, backbone_len)
    at = backbone_len // 2
    seen, out = set(), [backbone]
    while len(out) <= reads:
        ins = _backbone(rng, insert_len)
        if ins[0] in (backbone[at],) or ins in seen:  # the branch must leave the backbone at its first base
            continue
        seen.add(ins)
        out.append(backbone[:at] + ins + backbone[at:])
    return out


def _keep(windows):
    kept = [[r for r in w if 0 < len(r) < 1024] for w in windows]
    assert all(len(k) == len(w) and len(k) >= 2 for k, w in zip(kept, windows))  # nothing is left out
    return kept


def source_window(backbone_len, reads, seed):
    """Read r is the backbone behind a prefix of r bases, the longest read first: r - 1 times A behind a first base (C, G,
    T in turn) that matches nothing within two gaps' reach. It becomes a node beside the prefix path, without in-edges,
    and no later read runs through it: close to `reads` source nodes (the GPU test counts them), all of them in the Kahn
    queue when the sort starts."""
    rng = random.Random(seed)
    backbone = _backbone(rng, backbone_len)
    return [backbone] + ["CGT"[r % 3] + "A" * (r - 1) + backbone for r in range(reads, 0, -1)]


SETS = {
    # name: (windows, reads per window of the batch, device memory)
    "short_reads": (lambda: _keep(high_degree_windows() + small_windows() + [branch_window(300, 20, 30, 7)]), 32, 8 << 30),
    # BatchConfig-style 200 reads per window: 80 sources, a queue longer than the register window (and than the 4-bit field)
    "many_reads": (lambda: _keep([source_window(60, 80, 11)]), 200, 16 << 30),
}
_WINDOWS = {}


def windows_of(name):
    if name not in _WINDOWS:
        _WINDOWS[name] = SETS[name][0]()
    return [list(w) for w in _WINDOWS[name]]


def oracle_cfg(band_mode, max_seqs):
    cfg = O.make_cfg(1024, max_seqs, 256, BAND[band_mode])
    cfg.max_nodes_per_graph = 3072
    cfg.matrix_sequence_dimension = 1024 if band_mode == "full_band" else 264 if band_mode.startswith("static") else 528
    cfg.max_banded_pred_distance = 512
    O.lib().poa_cfg_select_types(cfg)
    return cfg


@pytest.mark.parametrize("which", ["high_degree", "small"])
def test_model_takes_every_branch_of_phase_2(which):
    windows = _keep(high_degree_windows() if which == "high_degree" else small_windows())
    with O.topsort_model(0) as tm:
        for mode in (1, 2):
            with O.Workspace(O.make_cfg(1024, 32, 256, mode)) as ws:
                for w in windows:
                    assert ws.process(w)["status"] == 0
        st = tm.stats()
    print(which, {k: st[k] for k in ("real_steps", "blocks", "sync_checks", "wide_steps", "mismatch", "empty_blocks")})
    assert st["mismatch"] == 0 and st["empty_blocks"] == 0, st
    assert st["real_steps"] > 0 and st["blocks"] > 0 and st["sync_checks"] > 0 and st["wide_steps"] > 0, st


def _run_gpu(windows, band_mode, max_seqs, mem, min_sources=0):
    from genomeworks_amd import cudapoa
    kw = {"matrix_sequence_dimension": 1024} if band_mode == "full_band" else {}
    b = cudapoa.CudaPoaBatch(max_seqs, 1024, mem, output_type="consensus", band_mode=band_mode, alignment_band_width=256,
                             max_nodes_per_graph=3072, **kw)
    for w in windows:
        st, seq_st = b.add_poa_group(w)
        assert st == 0 and all(s == 0 for s in seq_st)
    b.generate_poa()
    out = b.get_consensus(), b.total_cells()
    if min_sources:  # the queue of the last read's sort starts with the graph's sources
        graphs, _ = b.get_graphs()
        assert all(sum(1 for _, d in g.in_degree() if d == 0) >= min_sources for g in graphs)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("band_mode", list(BAND))
def test_kernel_equals_full_resort_and_oracle(monkeypatch, band_mode, which):
    """Production (incremental order) against the full re-sort after every read (GWHIP_DEBUG bit 21, the reference's
    schedule), and both against the oracle: consensus, coverage, status and cell count of every window."""
    windows = windows_of(which)
    _, max_seqs, mem = SETS[which]
    monkeypatch.delenv("GWHIP_DEBUG", raising=False)
    prod = _run_gpu(windows, band_mode, max_seqs, mem, min_sources=65 if which == "many_reads" else 0)
    monkeypatch.setenv("GWHIP_DEBUG", D.env_value(D.kDbgTopsortFullResort))
    full = _run_gpu(windows, band_mode, max_seqs, mem)
    monkeypatch.delenv("GWHIP_DEBUG", raising=False)
    assert prod == full
    (cons, cov, status), cells = prod
    cells_ref, compared = 0, 0
    with O.Workspace(oracle_cfg(band_mode, max_seqs)) as ws:
        for i, w in enumerate(windows):
            ref = ws.process(w)
            cells_ref += ref["cells"]
            assert status[i] == ref["status"] == 0, (i, status[i], ref["status"])
            assert cons[i] == ref["consensus"], i
            assert cov[i] == list(ref["coverage"]), i
            compared += 1
    assert compared == len(windows)
    assert cells == cells_ref
