"""Where a row's predecessor rows come from (genomeworks_amd/csrc/poa_pred_rows.h: the table word, the side table of
predecessors 3..5, the hit rule) against the plain statement, on the CPU: a stand-alone program, built once plain and once
with the sanitizers (no GPU needed)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 40 * (1 + 3 + 200 + 256 + 257 + 700 + 2048 + 4095)  # rounds x graph sizes of the program


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_predecessor_rows_equal_the_plain_statement(tmp_path, flags):
    exe = str(tmp_path / "pred_rows_check")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "pred_rows_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = r.stdout.split()
    assert out[0] == "ok" and int(out[1]) == ROWS, r.stdout
    # the cases the decode has to tell apart all occurred: entries that hit, slots lost to a later row, rows with 7+ predecessors
    hits, lost, wide = (int(x) for x in out[2:5])
    assert hits > 10000 and lost > 10000 and wide > 1000, r.stdout
