"""Where the packed forward pass takes a row's predecessor rows from (poa_pred_rows.h: table word, side table of predecessors
3..5, HBM edge list for what is left over) in mark_score_rows, the general row and the walk's recomputed step, on a window set
built for the rows that tell the three sources apart (tests/pred_rows_windows.py; the counts below are asserted on the CPU by
tests/test_pred_rows_windows.py from the oracle's row hook).

The set: 24 windows of 300-700 bases and 10-16 reads, graphs of 392-772 rows. At band 256 the oracle's rows hold, in the phase of
band start 0 / of the moved band: 185 / 340 rows with four, 48 / 167 with five and 26 / 59 with six predecessors all within 7
rows; 39 / 17 rows with more than six predecessors; 156 / 726 rows with a predecessor more than 7 rows up; 90 / 76 rows with
four to six predecessors that lose their side-table slot to a row 256 further down in the same pass. One read of every window
brings 70-90 new nodes at once; at one position three reads in turn bring a second, third and fourth base (new nodes aligned to a
node that has none, one, two aligned nodes: all four bases in one MSA column in 15 of the windows); reads end ragged, and the
backbone and three reads end in four different bases of one MSA column (four sinks; the last of those reads met three sinks
that mismatch its last base alike). The same CPU test asserts these from the oracle's MSA."""
import pytest

import oracle_poa as O
import pred_rows_windows as P
from genomeworks_amd import debug_flags as D
from test_gpu_poa import oracle_cfg, run_gpu

pytestmark = pytest.mark.gpu

CONFIGS = tuple((mode, width) for width in (256, 128) for mode in ("static_band", "adaptive_band"))
# GWHIP_DEBUG (debug instantiation): bit 25 every score row is stored, bit 23 every recomputed step of the walk reruns the
# forward pass with every row stored -- a predecessor that lost its mark would show as a walk over a row that was never written
ARMS = (("every_score_row_stored", D.env_value(D.kDbgEveryRowStoresScores)), ("every_recomputed_step_reruns", D.env_value(D.kDbgRerunEveryStep)))


@pytest.fixture(scope="module")
def windows():
    return P.build_windows()


@pytest.fixture(scope="module")
def production(windows):
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


@pytest.mark.parametrize("mode,width", CONFIGS)
def test_the_msa_equals_the_oracle(windows, mode, width):
    """The merge seen whole: every node, its aligned nodes and its column, for every read."""
    b = run_gpu(windows, mode, band_width=width, mem=2 << 30, output_type="msa")
    msa, status = b.get_msa()
    with O.Workspace(oracle_cfg(mode, band_width=width, output_mask=2)) as ws:
        for i, w in enumerate(windows):
            ref = ws.process(w)
            assert status[i] == ref["status"] == 0, (i, status[i], ref["status"])
            assert msa[i] == ref["msa"], "window %d MSA differs" % i


@pytest.mark.parametrize("arm,flag", ARMS)
def test_selective_score_rows_equal_every_row_stored(monkeypatch, windows, production, arm, flag):
    monkeypatch.setenv("GWHIP_DEBUG", flag)
    for mode, width in CONFIGS:
        b = run_gpu(windows, mode, band_width=width, mem=2 << 30)
        assert (b.get_consensus(), b.total_cells()) == production[mode, width], (arm, mode, width)


# reruns of the forward pass over the set per (band mode, width), counted on the parent of the change that took the predecessor
# rows from LDS (the same kernels with only the exact counter added): a row or a predecessor that lost its score-row mark would
# give the right result more slowly, through a rerun, and show here alone
PARENT_RERUNS = {("static_band", 256): 0, ("adaptive_band", 256): 0, ("static_band", 128): 24, ("adaptive_band", 128): 26}


def test_reruns_of_the_forward_pass_equal_the_parents(monkeypatch, windows):
    """GWHIP_DEBUG bit 24 with bit 13 adds 2^40 per rerun (a walk that met a cell it must recompute in a row kept out of HBM) to
    a window's "other" counter, above the clock ticks it otherwise holds: the exact number of reruns over the set, printed and
    equal to the parent's."""
    monkeypatch.setenv("GWHIP_DEBUG", D.env_value(D.kDbgCountReruns, D.kDbgKindFine))
    reruns = {}
    for mode, width in CONFIGS:
        b = run_gpu(windows, mode, band_width=width, mem=2 << 30)
        per_window = [w["other"] for w in b.profile_phases_per_window()]
        assert all((v & ((1 << 40) - 1)) < (1 << 36) for v in per_window)  # the ticks stay far below the count's unit
        reruns[mode, width] = sum(v >> 40 for v in per_window)
    monkeypatch.delenv("GWHIP_DEBUG")
    print("reruns of the forward pass over the set:", reruns)
    assert reruns == PARENT_RERUNS
