#!/usr/bin/env python3
"""What mark_score_rows of the packed forward pass used to wait for on the config-3 windows (CPU, oracle): per window, the 64-row
chunks that hold a row with more than three predecessors, the dependent HBM round trips of those chunks when predecessors 3 and
up come from the edge list, and the rows the side table of predecessors 3..5 cannot serve. usage: pred_chunk_stats.py [windows]"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genomeworks_amd import synthetic  # noqa: E402

os.makedirs(os.path.join(ROOT, "tools", "bin"), exist_ok=True)
out = os.path.join(ROOT, "tools", "bin", "libpcs.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-o", out, os.path.join(ROOT, "tools", "pred_chunk_stats.c")], check=True)
import oracle_poa as O  # noqa: E402
L = C.CDLL(out)
L.pcs_get.argtypes = [C.c_void_p]
# the counting hook (C: one call per DP row) into the stock oracle's observer slot, as tests/pred_rows_windows.py does in Python
slot = C.c_void_p.in_dll(O.lib(), "poa_oracle_row_hook")
slot.value = C.cast(L.pcs_hook, C.c_void_p).value
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
with O.Workspace(O.make_cfg(1024, 32, 256, 1)) as ws:
    for w in range(n):
        assert ws.process([x.decode() for x in synthetic.generate_window(1000 + w)])["status"] == 0
slot.value = None
t = np.zeros(8, np.int64)
L.pcs_get(t.ctypes.data)
names = ("passes", "rows", "chunks", "chunks_with_a_row_of_more_than_3_predecessors", "dependent_round_trips_from_the_edge_list",
         "rows_with_4_to_6_predecessors", "rows_with_more_than_6_predecessors", "rows_that_lost_their_side_table_slot")
print(json.dumps({"windows": n, "band_width": 256, "per_window": {k: round(float(v) / n, 2) for k, v in zip(names, t)},
                  "round_trips_per_pass": round(float(t[4]) / max(int(t[0]), 1), 2)}, indent=1))
