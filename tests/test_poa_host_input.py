"""PoaBatch with the reads left in the pinned staging block, on the CPU (tests/cpp/poa_host_input_driver.cpp: the host
sources under test and recording stand-ins for every HIP and kernel-library entry point they call, with a
hipHostGetDevicePointer that succeeds). With host input generate_poa() makes no sequence copy, the launch gets the pinned
address, the read-ahead slack is zero in the host buffer, reset() and a refill behind a launch wait for the launch's event
before the block is touched, the first relaunch uploads once with the device pointer and the second uploads nothing, and
the destructor has synchronised before the block is freed. With the query failing, with GW_POA_HOST_INPUT=0 and with a
full-band configuration the calls are the ones made before there was host input. The driver checks itself; it is built
plain and, as the same stand-alone program, under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HOST = os.path.join(ROOT, "genomeworks_amd", "host")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "poa_host_input_driver.cpp")] + [
    os.path.join(HOST, f) for f in ("cudapoa_batch.cpp", "runtime.cpp", "logging.cpp", "device_pool.cpp")]


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_host_input_calls_and_lifetime(tmp_path, sanitized):
    exe = str(tmp_path / "poa_host_input_driver")
    # (the sanitizers' runtimes linked statically: the program does not depend on what else the process has loaded)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
             "-static-libubsan"] if sanitized else []
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                    "-pthread"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", os.path.join(ROCM, "include"),
                                           "-o", exe] + SOURCES, check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("GW_POA_HOST_INPUT", "GW_PINNED_CACHE_BYTES")}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    failed = [l for l in out.stdout.split("\n") if l.startswith("FAIL")]
    assert out.returncode == 0 and not failed, out.stdout[-4000:]
    assert out.stdout.count("\nok  ") >= 35 and "0 checks failed" in out.stdout


def test_the_library_query_names_the_lds_table_kernels_of_the_score_matrix_bands():
    """gwhip_poa_reads_host_sequences (a host function, no GPU needed) on the edges of its rule: 16-bit ids, at most 3072 graph
    rows and 2032 bases per read -- the kernels with their tables in LDS -- in the static and the adaptive band; any score
    type. The driver's stand-in above follows the same rule."""
    import ctypes as C
    from genomeworks_amd import _native
    L = _native.gwhip()
    L.gwhip_poa_reads_host_sequences.argtypes = [C.POINTER(_native.PoaConfig)]
    L.gwhip_poa_reads_host_sequences.restype = C.c_int32

    def ask(nodes=3072, seq=1024, mode=1, score32=0, size32=0):
        cfg = _native.PoaConfig()
        cfg.max_sequence_size, cfg.max_consensus_size, cfg.max_nodes_per_graph = seq, 2 * seq, nodes
        cfg.matrix_sequence_dimension, cfg.alignment_band_width, cfg.max_sequences_per_poa = 264, 256, 32
        cfg.band_mode, cfg.max_banded_pred_distance = mode, 512
        cfg.gap_score, cfg.mismatch_score, cfg.match_score, cfg.output_mask = -8, -6, 8, 1
        cfg.score32, cfg.size32 = score32, size32
        return L.gwhip_poa_reads_host_sequences(C.byref(cfg))

    assert [ask(mode=m) for m in range(5)] == [0, 1, 1, 0, 0]  # full, static, adaptive, and the two traceback-buffer modes
    assert ask(nodes=3072) == 1 and ask(nodes=3073) == 0
    assert ask(seq=2032) == 1 and ask(seq=2033) == 0
    assert ask(score32=1) == 1 and ask(score32=1, size32=1) == 0
    assert L.gwhip_poa_reads_host_sequences(None) == 0
