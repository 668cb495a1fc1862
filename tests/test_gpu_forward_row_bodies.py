"""The row bodies of the packed forward pass (poa_forward_moves.h: one straight-line body per descriptor kind, operands
ready-made per block of 63 rows, poa_forward_row_operands.h) on a small window set that reaches every body in both
phases, against the oracle and against the general routine.

The set (seeds below, chosen on the CPU with the oracle's row hook, the way tools/row_distance_stats.py observes the
rows): 36 windows of 200-420 bases and 6-12 reads in the six divergence classes of
test_kernel_shortcuts_equal_the_plain_schedule scaled to the length, every fourth with ragged starts, and four
config-3 windows cut to their first 6 reads. At band 256 the oracle's rows hold, over the set, in the phase of band
start 0 / of the moved band: 45 168 / 50 757 rows on the previous row, 0 / 6 528 on the previous row with the band moved a
quad (a band that starts at column 0 has not moved, so that kind cannot occur in the first phase), 1 611 / 2 381 with one,
3 916 / 5 093 with two, 309 / 303 with three and 19 / 12 with four to six predecessors within 7 rows, 327 / 255 for the
general routine (a read shorter than 255 bases takes the generic pass at band 256: the first-phase rows of those reads, 15 561
of the 51 350, do not reach these bodies; a band that has moved belongs to a longer read). 11 of the rows with four to six predecessors lie at row indices above 256 (windows 3, 9 and 22: the side
table of predecessors 3..5 has wrapped there), and with phases of 200-1 075 rows and blocks of 63 nearly every phase ends
inside a block."""
import random

import pytest

import oracle_poa as O
from genomeworks_amd import debug_flags as D
from test_gpu_poa import config3, oracle_cfg, run_gpu

pytestmark = pytest.mark.gpu

CLASSES = ((0, 0, 0), (5, 2, 2), (40, 20, 20), (90, 40, 40), (10, 60, 5), (10, 5, 60))  # per 1000 bases
SEEDS = tuple(range(9100, 9136))
SHAPE_SEED = 63
CONFIG3_FIRST, CONFIG3_COUNT = 1000, 4
CONFIGS = tuple((mode, width) for width in (256, 128) for mode in ("static_band", "adaptive_band"))
ARMS = (("ring_through_general", D.env_value(D.kDbgRingToGeneral)),
        ("everything_general", D.env_value(D.kDbgRingToGeneral, D.kDbgRegistersToGeneral, D.kDbgManyPredsToGeneral)))
# descriptor kinds (poa_forward_row_operands.h)
KINDS = {0: "previous row", 1: "previous row, band moved", 2: "one from the ring", 3: "two from the ring", 4: "general",
         5: "three from the ring", 6: "four to six from the ring"}


@pytest.fixture(scope="module")
def windows():
    from genomeworks_amd import synthetic
    rng = random.Random(SHAPE_SEED)
    out = []
    for k, seed in enumerate(SEEDS):
        blen = rng.randrange(200, 421)
        reads = rng.randrange(6, 13)
        mut, ins, dele = (max(1, round(c * blen / 1000)) if c else 0 for c in CLASSES[k % 6])
        w = [r.decode() for r in synthetic.generate_window(seed, blen, reads, mut, ins, dele)]
        if k % 4 == 0:
            w = [("GATTACA"[: rng.randrange(8)] + r)[rng.randrange(5):] for r in w]
        out.append([r for r in w if 0 < len(r) < 1024])
    out += [w[:6] for w in config3(CONFIG3_COUNT, CONFIG3_FIRST)]
    return out


@pytest.fixture(scope="module")
def production(windows):
    """consensus, coverage, status and cell count of the production instantiation, per (band mode, width)"""
    import os
    assert "GWHIP_DEBUG" not in os.environ
    out = {}
    for mode, width in CONFIGS:
        b = run_gpu(windows, mode, band_width=width, mem=2 << 30)
        out[mode, width] = (b.get_consensus(), b.total_cells())
    return out


@pytest.mark.parametrize("mode,width", CONFIGS)
def test_every_window_equals_the_oracle(windows, production, mode, width):
    (cons, cov, status), cells = production[mode, width]
    cells_ref = 0
    with O.Workspace(oracle_cfg(mode, band_width=width)) as ws:
        for i, w in enumerate(windows):
            ref = ws.process(w)
            cells_ref += ref["cells"]
            assert status[i] == ref["status"] == 0, (i, status[i], ref["status"])
            assert cons[i] == ref["consensus"], "window %d consensus differs" % i
            assert cov[i] == list(ref["coverage"]), "window %d coverage differs" % i
        assert ws.overflow_events() == 0
    assert cells == cells_ref


@pytest.mark.parametrize("arm,flag", ARMS)
def test_row_bodies_equal_the_general_routine(monkeypatch, windows, production, arm, flag):
    monkeypatch.setenv("GWHIP_DEBUG", flag)
    for mode, width in CONFIGS:
        b = run_gpu(windows, mode, band_width=width, mem=2 << 30)
        assert (b.get_consensus(), b.total_cells()) == production[mode, width], (arm, mode, width)


def test_every_descriptor_kind_runs_in_both_phases(monkeypatch, windows):
    """The per-kind row counters (GWHIP_DEBUG bits 28-30 = descriptor kind + 1 with bits 13 and 12: a counted row adds 2^32 in
    the phase of band start 0 and 2^48 in the moved phase to its window's "other" counter) at band 256: every body has run in
    both phases, except that a row whose band starts at column 0 cannot have moved its band (kind 1 in the first phase is
    0 by construction); the moved-phase counts add up to the moved-phase rows of the set."""
    b = run_gpu(windows, "static_band", band_width=256, mem=2 << 30)
    rows = {}
    for kind in KINDS:
        monkeypatch.setenv("GWHIP_DEBUG", D.env_value(D.kDbgKindFine, D.kDbgKindCount, row_kind=kind))
        per_window = [w["other"] for w in b.profile_phases_per_window()]
        rows[kind] = (sum((v >> 32) & 0xffff for v in per_window), sum(v >> 48 for v in per_window))
    monkeypatch.delenv("GWHIP_DEBUG")
    print("rows per descriptor kind (band start 0, moved band):", {KINDS[k]: v for k, v in rows.items()})
    for kind, (first, moved) in rows.items():
        assert moved >= 1, (KINDS[kind], rows)
        assert (first == 0) if kind == 1 else (first >= 1), (KINDS[kind], rows)
    # one DP row per graph node and read: 65 329 rows with a moved band in the oracle's forward passes (module docstring), all of
    # them in reads long enough for the packed pass; a read whose walk needs a score row that was kept out of HBM runs its
    # forward pass a second time
    moved_total = sum(moved for _, moved in rows.values())
    assert 65329 <= moved_total <= 2 * 65329, moved_total
