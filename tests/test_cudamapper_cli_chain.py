"""The cudamapper tool's --chain options: argument handling only, which ends before any device work. No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "genomeworks_amd", "bin", "cudamapper")
CHAIN_OPTIONS = ("--chain-max-gap", "--chain-bandwidth", "--chain-min-score", "--chain-max-chains")


def run_tool(args):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=60)


@pytest.fixture
def fasta(tmp_path):
    path = tmp_path / "reads.fasta"
    path.write_text(">a\nACGT\n")
    return str(path)


@pytest.mark.parametrize("option", CHAIN_OPTIONS)
def test_chain_values_are_refused_without_chain(fasta, option):
    run = run_tool([option, "3", fasta, fasta])
    assert run.returncode != 0 and run.stdout == ""
    assert "cudamapper: %s needs --chain" % option in run.stderr


@pytest.mark.parametrize("args", [["--chain-max-gap", "0"], ["--chain-max-gap", "-5"], ["--chain-bandwidth", "-1"],
                                  ["--chain-min-score", "-1"], ["--chain-max-chains", "0"],
                                  ["--chain-max-chains", "65"], ["--chain-max-chains", "many"]])
def test_chain_values_out_of_range_are_refused(fasta, args):
    run = run_tool(["--chain"] + args + [fasta, fasta])
    assert run.returncode != 0 and run.stdout == ""
    assert "cudamapper:" in run.stderr and ("--chain-" in run.stderr or args[1] == "many")


def test_chain_options_are_in_the_help():
    run = run_tool(["--help"])
    for option in ("--chain ",) + CHAIN_OPTIONS:
        assert option in run.stdout, option
    for default in ("[5000]", "[500]", "[40]", "[4]"):
        assert default in run.stdout
