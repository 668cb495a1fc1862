"""The host Alignment classes against the reference's own vectors (cudaaligner/tests/Test_AlignmentImpl.cpp:36-204,
extracted into tests/golden/cudaaligner_vectors.json): CIGAR (basic / extended), format_alignment, getters -- for
AlignmentImpl and for the PackedAlignment views that sync_alignments() of the banded aligner hands out."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from genomeworks_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("aln") / "alignment_impl_driver")
    lib = os.path.join(ROOT, "genomeworks_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "genomeworks_amd", "host"), "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "alignment_impl_driver.cpp"), "-L", lib, "-lgenomeworks_amd", "-lgwhip",
                    "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROCM, "lib"),
                    "-pthread"], check=True)
    return exe


def run(driver, cases):
    text = "".join("%s %s %s %d\n" % (c["query"] or "-", c["target"] or "-", "".join(str(s) for s in c["alignment"]) or "-",
                                        1 if c["is_optimal"] else 0) for c in cases)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout
    return [line.split("\t") for line in out.split("\n") if line]


def test_reference_vectors(driver):
    with open(os.path.join(ROOT, "tests", "golden", "cudaaligner_vectors.json")) as f:
        cases = json.load(f)["alignment_impl"]
    rows = run(driver, cases)
    assert rows[0] == ["initial", "1", "1"]      # StatusType::uninitialized, AlignmentType::unset
    assert rows[1] == ["after_set", "0", "0"]    # success, global_alignment
    rows = rows[3:]
    per_case = 4  # AlignmentImpl, PackedAlignment(runs), runs, PackedAlignment(states)
    assert len(rows) == per_case * len(cases)
    for k, c in enumerate(cases):
        impl, packed_runs, runs, packed_states = rows[per_case * k:per_case * k + per_case]
        states = "".join(str(s) for s in c["alignment"])
        ed = sum(1 for s in c["alignment"] if s != 0)
        for got in (impl, packed_states):
            assert got[1:5] == [c["query"], c["target"], states, "1" if c["is_optimal"] else "0"], got[0]
            assert got[7] == c["cigar_basic"] and got[8] == c["cigar_extended"] and int(got[9]) == ed, got[0]
            assert got[10:13] == c["formatted"], got[0]
        # run-length form (what the banded aligner produces): same CIGARs and distance; per-position states are not held
        assert packed_runs[1:3] == [c["query"], c["target"]] and packed_runs[3] == ""
        assert packed_runs[7] == c["cigar_basic"] and packed_runs[8] == c["cigar_extended"] and int(packed_runs[9]) == ed
        # its runs, forward order, re-expand to the states
        expanded = "".join(op * int(n) for n, op in (r.split("x") for r in runs[1].split(",") if r))
        assert expanded == states


def test_line_wrapped_output_and_empty_alignment(driver):
    rows = run(driver, [dict(query="ACGTA", target="ACTA", alignment=[0, 0, 3, 0, 0], is_optimal=True),
                        dict(query="", target="", alignment=[], is_optimal=True)])[3:]
    impl = rows[0]
    # operator<< with linebreak_after = 3: query / pairing / target in blocks of three columns
    assert impl[13] == "ACG/|| /AC-/TA/||/TA//"
    empty = rows[4]
    assert empty[0] == "AlignmentImpl" and empty[7] == "" and empty[8] == "" and empty[9] == "0"


def test_reversed_states_helper_equals_a_plain_reverse_loop(driver):
    """gwhost::reverse_bytes (host_common.hpp), which turns the kernels' back-to-front paths around for AlignerGlobal and
    AlignerSemiglobal: lengths 0, 1, 7, 8, 9, 15, 16, 17 and 1000 against a plain loop, guard bytes around the range."""
    assert run(driver, [])[2] == ["reverse_bytes", "ok"]


def test_banded_pipeline_submits_the_recorded_calls(tmp_path):
    """The banded aligner's three-stream pipeline replayed on the CPU (tests/cpp/banded_pipeline_replay_driver.cpp: recording
    stand-ins for the HIP runtime and the kernels' entry points, defined in the executable so that they take precedence over
    the libraries'): create_aligner, 640 x add_alignment, align_all, relaunch, sync_alignments and a second batch with another
    chunk count on the same object, for one chunk, five chunks, and seven chunks with a mirror of three runs. Every HIP call --
    stream by role, copy sizes and offsets, events by role and chunk -- equals tests/golden/banded_pipeline_calls*.txt, recorded
    from the commit before the host classes' streams, events and pinned buffers were restructured."""
    from genomeworks_amd import build
    build.build_host()
    exe = str(tmp_path / "banded_pipeline_replay_driver")
    lib = os.path.join(ROOT, "genomeworks_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "genomeworks_amd", "host"), "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "banded_pipeline_replay_driver.cpp"), "-rdynamic", "-L", lib,
                    "-lgenomeworks_amd", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + lib,
                    "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-pthread"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GW_ALIGNER_")}
    # (the second run: the second chunk's workspace does not fit, align_all() drains its streams and throws, and the same object
    # is reset and takes a whole batch)
    for args, golden in (([], "banded_pipeline_calls.txt"), (["--fail-alloc"], "banded_pipeline_calls_alloc_failure.txt")):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        with open(os.path.join(ROOT, "tests", "golden", golden)) as f:
            want = f.read().split("\n")
        got = out.stdout.split("\n")
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        assert got == want, "%s: first difference at line %d:\n  got  %r\n  want %r" % (
            golden, first + 1, got[first] if first < len(got) else None, want[first] if first < len(want) else None)


def test_worker_pool_runs_every_task_once(tmp_path):
    """gwhost::parallel_tasks (the pool behind the un-reversal of get_consensus()): tests/cpp/parallel_tasks_driver.cpp."""
    from genomeworks_amd import build
    build.build_host()
    exe = str(tmp_path / "parallel_tasks_driver")
    lib = os.path.join(ROOT, "genomeworks_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "genomeworks_amd", "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "parallel_tasks_driver.cpp"), "-L", lib, "-lgenomeworks_amd", "-lgwhip",
                    "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROCM, "lib"),
                    "-pthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_two_bases_per_byte_round_trip(tmp_path):
    """The banded aligner's upload format (genomeworks_amd/host/base_packing.hpp) against a restatement of the device-side
    expansion: tests/cpp/base_packing_driver.cpp."""
    exe = str(tmp_path / "base_packing_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "genomeworks_amd", "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "base_packing_driver.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_chunk_order_on_host_threads_equals_a_plain_stable_sort(tmp_path):
    """The banded aligner's processing order and workspace sizing in pieces on pool threads (genomeworks_amd/host/chunk_order.hpp)
    against one stable sort and one sizing call per chunk: tests/cpp/chunk_order_driver.cpp."""
    from genomeworks_amd import build
    build.build_all()
    exe = str(tmp_path / "chunk_order_driver")
    lib = os.path.join(ROOT, "genomeworks_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "genomeworks_amd", "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "chunk_order_driver.cpp"), "-L", lib, "-lgenomeworks_amd", "-lgwhip",
                    "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROCM, "lib"),
                    "-pthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
