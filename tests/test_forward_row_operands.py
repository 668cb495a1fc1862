"""The row operands of the packed forward pass (genomeworks_amd/csrc/poa_forward_row_operands.h) against the plain
per-row decode, on the CPU: a stand-alone program built with the sanitizers (no GPU needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_operands_equal_the_plain_decode_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "forward_row_operands_sanitized")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "forward_row_operands_sanitized.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    # 5 table kinds x 6 counts x 7^3 distances x 32 rows x 8 band starts x 4 flag pairs
    assert r.stdout.split() == ["ok", str(5 * 6 * 343 * 32 * 8 * 4)]
