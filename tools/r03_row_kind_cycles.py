#!/usr/bin/env python3
"""Cycles per DP row of each row kind of the metric kernel's forward pass (needs a GPU; debug instantiation with s_memtime
around the rows of ONE kind per launch, GWHIP_DEBUG bits 28-30 and 12): poa_forward_moves.h.

"kinds": the TABLE kinds of classify_kinds (3 = every multi-predecessor ring row; its selector carries bit 30, which sends
rows with 4..6 predecessors to the general routine). "descriptor_kinds" (bit 13, builds that have the descriptor kinds of
poa_forward_row_operands.h; pass --table-kinds-only for older ones): table kind 3 split into two / three / four to six
predecessors, nothing demoted, row counts exact and per phase (band start 0 / moved)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genomeworks_amd import cudapoa, synthetic

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 1024
windows = [[r.decode() for r in synthetic.generate_window(1000 + w)] for w in range(n)]
b = cudapoa.CudaPoaBatch(32, 1024, 8 << 30, band_mode="static_band", alignment_band_width=256, max_nodes_per_graph=3072)
for w in windows:
    assert b.add_poa_group(w)[0] == 0
b.generate_poa()
b.get_consensus_native()


def debug_env(flags):
    os.environ["GWHIP_DEBUG"] = str(flags - (1 << 32) if flags >= (1 << 31) else flags)


def other(flags):
    debug_env(flags)
    v = b.profile_phases()
    os.environ.pop("GWHIP_DEBUG", None)
    return v


def other_per_window(flags):
    debug_env(flags)
    v = [w["other"] for w in b.profile_phases_per_window()]
    os.environ.pop("GWHIP_DEBUG", None)
    return v


base = other(1 << 31)
res = {"windows": n, "baseline_ticks_per_window": base, "kinds": {}}
names = ["0 previous row, band not moved", "1 previous row, band moved one quad", "2 one predecessor from the ring", "3 2..6 predecessors from the ring", "4 general"]
for k in range(5):
    cyc = other(((k + 1) << 28))
    cnt = other(((k + 1) << 28) | (1 << 12))
    rows = cnt["other"] - base["other"]
    ticks = cyc["other"] - base["other"]
    res["kinds"][names[k]] = {"rows_per_window": round(rows, 1), "ticks_per_window": round(ticks), "ticks_per_row": round(ticks / max(rows, 1e-9), 1),
                              "forward_ticks_with_timers": round(cyc["nw_forward"])}
if "--table-kinds-only" not in sys.argv:
    FINE = 1 << 13
    base_fine = other(FINE)
    dnames = ["0 previous row, band not moved", "1 previous row, band moved one quad", "2 one predecessor from the ring",
              "3 two predecessors from the ring", "4 general", "5 three predecessors from the ring", "6 four to six predecessors from the ring"]
    res["descriptor_kinds"] = {}
    for k in range(7):
        cyc = other(((k + 1) << 28) | FINE)
        counted = other_per_window(((k + 1) << 28) | FINE | (1 << 12))
        # a counted row adds 2^32 (band start 0) or 2^48 (moved band) to the window's "other" ticks, which stay below 2^32
        rows0 = sum((v >> 32) & 0xffff for v in counted) / n
        rows1 = sum(v >> 48 for v in counted) / n
        ticks = cyc["other"] - base_fine["other"]
        res["descriptor_kinds"][dnames[k]] = {"rows_per_window": round(rows0 + rows1, 1), "rows_per_window_band_start_0": round(rows0, 1),
                                              "rows_per_window_moved_band": round(rows1, 1), "ticks_per_window": round(ticks),
                                              "ticks_per_row": round(ticks / max(rows0 + rows1, 1e-9), 1),
                                              "forward_ticks_with_timers": round(cyc["nw_forward"])}
print(json.dumps(res))
