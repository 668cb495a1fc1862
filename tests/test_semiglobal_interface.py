"""The public surface of the infix / prefix alignment types without a GPU: a caller's translation unit compiles against
include/ and links against the libraries (tests/cpp/semiglobal_interface_driver.cpp), the new C symbols are exported,
and the Python constructor refuses what it must before it touches a device. With a GPU, the same driver goes through
the C++ factories."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from genomeworks_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("semiglobal") / "semiglobal_interface_driver")
    cmd = ["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "cpp", "semiglobal_interface_driver.cpp"),
           "-L", LIB, "-lgenomeworks_amd", "-lgwsemiglobal", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
           "-Wl,-rpath," + LIB, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_enumerators_accessors_and_entry_points_compile_and_link(driver):
    r = subprocess.run([driver], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) == (0, "ok"), r.stderr


@pytest.mark.gpu
def test_cpp_factories_on_the_gpu(driver):
    r = subprocess.run([driver, "gpu"], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) == (0, "ok"), r.stderr


def test_new_c_symbols_are_exported():
    host = C.CDLL(os.path.join(LIB, "libgenomeworks_amd.so"), mode=C.RTLD_GLOBAL)
    for name in ("gw_aligner_create_typed", "gw_alignment_target_range", "gw_alignment_type", "gw_aligner_stage_ms"):
        assert hasattr(host, name), name
    kernels = C.CDLL(os.path.join(LIB, "libgwsemiglobal.so"), mode=C.RTLD_GLOBAL)
    for name in ("gwhip_semiglobal_ends", "gwhip_semiglobal_gather", "gwhip_semiglobal_workspace_bytes",
                 "gwhip_semiglobal_last_error"):
        assert hasattr(kernels, name), name


def test_source_digest_ignores_the_new_kernels():
    """The stamped kernel set is csrc/ and include/gwhip.h: the new library lives outside both."""
    from genomeworks_amd import build
    assert not any(s.startswith("csrc/") for s in build.SEMIGLOBAL_KERNEL_SRCS)
    with open(os.path.join(ROOT, "include", "gwhip.h")) as f:
        assert "semiglobal" not in f.read()


def test_python_constructor_refusals_need_no_device():
    from genomeworks_amd import cudaaligner
    for kw in (dict(alignment_type="infix", max_bandwidth=64), dict(alignment_type="prefix", algorithm="ukkonen"),
               dict(alignment_type="local")):
        with pytest.raises(RuntimeError):
            cudaaligner.CudaAlignerBatch(10, 10, 1, **kw)
