"""The cudapoa host path replayed on the CPU (tests/cpp/poa_host_replay_driver.cpp: recording stand-ins for the HIP runtime
and for the POA entry points of the kernel library, defined in the executable so that they take precedence over the
libraries'): one PoaBatch through its whole life, process_windows_multi_device with one worker and with four, and
process_windows_size_classes with a gated class, a class of two fills, a class whose Batch cannot be created and a class
whose fill leaves the batch empty. Every call -- stream, copy sizes and offsets, events, the arguments of every launch --
and every returned value equals tests/golden/poa_host_replay.txt, recorded from the commit before PoaBatch and the two
drivers were folded onto shared helpers. With one thread per worker the text is compared per stream (size classes) or by
window only (four workers on the shared cursor); the driver says how."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_poa_host_path_makes_the_recorded_calls(tmp_path):
    from genomeworks_amd import build
    build.build_host()
    exe = str(tmp_path / "poa_host_replay_driver")
    lib = os.path.join(ROOT, "genomeworks_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "genomeworks_amd", "host"), "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "poa_host_replay_driver.cpp"), "-rdynamic", "-L", lib,
                    "-lgenomeworks_amd", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + lib,
                    "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-pthread"], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    # a warning of the library names its source line: "[WARN /path/to/cudapoa_batch.cpp:123]" is compared as "[WARN cudapoa_batch.cpp]"
    got = re.sub(r"\[([A-Z]+) [^\] ]*/([^/ ]+):\d+\]", r"[\1 \2]", out.stdout).split("\n")
    with open(os.path.join(ROOT, "tests", "golden", "poa_host_replay.txt")) as f:
        want = f.read().split("\n")
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, "first difference at line %d:\n  got  %r\n  want %r" % (
        first + 1, got[first] if first < len(got) else None, want[first] if first < len(want) else None)
    # the scenarios are what they say they are
    text = out.stdout
    assert "hipStreamWaitEvent stream#2 waits for event#1" in text                      # the third class is gated on the second
    first_class = text[text.index("== consensus\nno exception"):].split("-- stream#0\n")[1].split("-- stream#1\n")[0]
    assert re.findall(r"gwhip_poa_generate on stream#0: (\d+) windows", first_class) == ["8", "4"]  # two fills
    assert first_class.count("hipEventRecord event#0 on stream#0") == 2                  # its event is recorded behind each
    assert "exception: Requires at least 3110544168 bytes" in text                      # rethrown once the workers were joined
    assert "D2H 12096 bytes" in text and text.count("Kernel Error: Node count exceeded") == 4
