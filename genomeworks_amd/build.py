"""In-tree build of the native libraries (hipcc for gfx950, no GPU needed).

  genomeworks_amd/lib/libgwhip.so            hand-written HIP kernels + the thin C-ABI (include/gwhip.h)
  genomeworks_amd/lib/libgwsemiglobal.so     cudaaligner's infix / prefix types: the ends scan and the slice gather
                                             (include/gwhip_semiglobal.h), linked against libgwhip.so
  genomeworks_amd/lib/libgwaffine.so         the affine-gap global aligner: forward pass and traceback inside a diagonal band
                                             (include/gwhip_affine.h), on its own
  genomeworks_amd/lib/libgwhip_poa_hooks.so  test-only hook of the production POA merge (include/gwhip_poa_hooks.h)
  genomeworks_amd/lib/libgenomeworks_amd.so  host C++ (Batch / Aligner, allocator, C API include/gw_capi.h)
  genomeworks_amd/lib/libcudaextender.so     cudaextender: HIP kernels (include/gwhip_extender.h) + Extender
                                             (cudaextender/extender.hpp, C API include/gw_extender_capi.h)
  genomeworks_amd/lib/libcudamapper.so       cudamapper: HIP kernels (include/gwhip_mapper.h) + Index / Matcher
                                             handles and the batched driver (C API include/gw_mapper_capi.h)
  genomeworks_amd/bin/cudamapper             the cudamapper tool over libcudamapper.so (mapper/cudamapper_main.cpp)

Called by __graft_entry__.build(); also usable as `python -m genomeworks_amd.build`.
"""
import hashlib
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB = os.path.join(PKG, "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")

KERNEL_SRCS = ["csrc/gwhip_poa.hip", "csrc/gwhip_poa_part0.hip", "csrc/gwhip_poa_part1.hip", "csrc/gwhip_poa_part2.hip",
               "csrc/gwhip_poa_part3.hip", "csrc/gwhip_poa_part4.hip", "csrc/gwhip_poa_part5.hip", "csrc/gwhip_poa_part6.hip", "csrc/gwhip_poa_part7.hip", "csrc/gwhip_poa_hooks.hip", "csrc/gwhip_myers.hip", "csrc/gwhip_ukkonen.hip"]
HOST_SRCS = ["host/capi.cpp", "host/cudapoa_batch.cpp", "host/cudapoa_utils.cpp", "host/cudaaligner.cpp", "host/aligner_global.cpp", "host/device_pool.cpp",
             "host/aligner_semiglobal.cpp", "host/aligner_affine.cpp", "host/alignment_impl.cpp", "host/runtime.cpp", "host/logging.cpp", "host/overlap_alignment.cpp", "host/multi_device.cpp",
             "host/fasta_parser.cpp"]
# cudaextender lives apart from csrc/ so that kernel_source_digest() (the stamped POA / aligner kernel set) ignores it
EXTENDER_KERNEL_SRCS = ["extender/gwx_ungapped_xdrop.hip"]
EXTENDER_HOST_SRCS = ["extender/extender.cpp"]
# the infix / prefix alignment types of cudaaligner likewise (the host class is in host/)
SEMIGLOBAL_KERNEL_SRCS = ["semiglobal/gws_ends.hip"]
# the affine-gap global aligner likewise (the host class is in host/)
AFFINE_KERNEL_SRCS = ["affine/gwaffine.hip"]
# the test-only hook of the production POA merge likewise (include/gwhip_poa_hooks.h)
POA_HOOKS_KERNEL_SRCS = ["poa_hooks/gwhip_poa_merge_hook.hip"]
# cudamapper likewise
MAPPER_KERNEL_SRCS = ["mapper/gwm_mapper.hip", "mapper/gwm_postprocess.hip", "mapper/gwm_align.hip",
                      "mapper/gwm_segments.hip", "mapper/gwm_pileup.hip", "mapper/gwm_variants.hip",
                      "mapper/gwm_qualities.hip", "mapper/gwm_index_cache.hip", "mapper/gwm_chain.hip",
                      "mapper/gwm_anchored.hip"]
MAPPER_HOST_SRCS = ["mapper/mapper.cpp", "mapper/gwm_driver.cpp", "mapper/gwm_index_batcher.cpp",
                    "mapper/gwm_windows.cpp"]

# no fast-math, no FMA contraction: band placement is IEEE fp32
KERNEL_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off",
                "-fhip-fp32-correctly-rounded-divide-sqrt"]
# experiments (same-box A/B of compiler options, tools/ab_headline.sh): extra hipcc flags for the kernel translation units
KERNEL_FLAGS += [f for f in os.environ.get("GW_KERNEL_EXTRA_FLAGS", "").split() if f]
HOST_FLAGS = ["-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-parameter",
              "-D__HIP_PLATFORM_AMD__", "-pthread"]


def _digest(paths, extra):
    h = hashlib.sha256(repr(extra).encode())
    for p in sorted(paths):
        with open(p, "rb") as f:
            h.update(p.encode())
            h.update(f.read())
    return h.hexdigest()


def kernel_source_digest():
    """sha256 over the device sources (csrc/*.hip, *.h) and include/gwhip.h by repo-relative name and content: what a measurement
    session stamps into its PMC profile and bench.py recomputes at run time, so counters taken on other kernels are never
    attached to a line (the GPU box has no .git to ask)."""
    h = hashlib.sha256()
    base = os.path.join(PKG, "csrc")
    paths = [os.path.join(base, f) for f in os.listdir(base) if f.endswith((".hip", ".h"))] + [os.path.join(ROOT, "include", "gwhip.h")]
    for p in sorted(paths):
        with open(p, "rb") as f:
            h.update(os.path.relpath(p, ROOT).encode())
            h.update(f.read())
    return h.hexdigest()


def _deps(subdir, exts):
    out = []
    for base in (os.path.join(PKG, subdir), os.path.join(ROOT, "include")):
        for d, _, fs in os.walk(base):
            out += [os.path.join(d, f) for f in fs if f.endswith(exts)]
    return out


def _run(cmd):
    print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def _stale(target, stamp_value):
    stamp = target + ".stamp"
    if not os.path.exists(target) or not os.path.exists(stamp):
        return True
    with open(stamp) as f:
        return f.read().strip() != stamp_value


def _mark(target, stamp_value):
    with open(target + ".stamp", "w") as f:
        f.write(stamp_value)


def _local_includes(src):
    """Headers of csrc/ that `src` includes, transitively (plus include/gwhip.h): an object is rebuilt when its own
    source or one of these changes -- the POA translation unit takes minutes, the aligner ones seconds."""
    import re
    seen, todo = set(), [src]
    while todo:
        f = todo.pop()
        with open(f) as fh:
            for name in re.findall(r'#include\s+"([^"]+)"', fh.read()):
                path = os.path.normpath(os.path.join(os.path.dirname(f), name))
                if os.path.exists(path) and path not in seen:
                    seen.add(path)
                    todo.append(path)
    return sorted(seen)


INCLUDE = ["-I", os.path.join(ROOT, "include")]
HIPCC_OBJECT = [HIPCC] + KERNEL_FLAGS + INCLUDE
GXX_OBJECT = ["g++"] + HOST_FLAGS + INCLUDE + ["-I", os.path.join(ROCM, "include")]


def _build_library(name, jobs, link_args, force):
    """lib/<name> from `jobs`, a list of (compiler command without source and output, source, signature): every source
    is compiled to lib/<its name>.o, in parallel, when its stamped signature is not the job's (or on `force`), and the
    objects are linked when one was compiled or their signatures are not the ones the library was linked from."""
    os.makedirs(LIB, exist_ok=True)
    target = os.path.join(LIB, name)
    objs, procs = [], []
    for compiler, src, sig in jobs:
        o = os.path.join(LIB, os.path.basename(src) + ".o")
        objs.append(o)
        if force or _stale(o, sig):
            cmd = compiler + ["-c", src, "-o", o]
            print("[build]", " ".join(cmd), flush=True)
            procs.append((subprocess.Popen(cmd), o, sig))
    for p, o, sig in procs:
        if p.wait() != 0:
            raise RuntimeError("building %s failed" % name)
        _mark(o, sig)
    link_sig = _digest([], [sig for compiler, src, sig in jobs])
    if force or procs or _stale(target, link_sig):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target] + objs + link_args)
        _mark(target, link_sig)
    return target, link_sig


def build_kernels(force=False):
    srcs = [os.path.join(PKG, s) for s in KERNEL_SRCS if os.path.exists(os.path.join(PKG, s))]
    return _build_library("libgwhip.so", [(HIPCC_OBJECT, s, _digest([s] + _local_includes(s), KERNEL_FLAGS))
                                          for s in srcs], [], force)[0]


def build_host(force=False):
    os.makedirs(LIB, exist_ok=True)
    target = os.path.join(LIB, "libgenomeworks_amd.so")
    srcs = [os.path.join(PKG, s) for s in HOST_SRCS if os.path.exists(os.path.join(PKG, s))]
    # the host library links libgwhip.so, libgwsemiglobal.so and libgwaffine.so. Called alone in a fresh tree, this builds
    # the first; the other two are brought up to date every time (one small translation unit each, incremental), and a
    # relink follows them
    if not os.path.exists(os.path.join(LIB, "libgwhip.so")):
        build_kernels()
    with open(build_semiglobal() + ".stamp") as f:
        semiglobal_sig = f.read().strip()
    with open(build_affine() + ".stamp") as f:
        affine_sig = f.read().strip()
    sig = _digest(_deps("host", (".cpp", ".h", ".hpp")), [HOST_FLAGS, semiglobal_sig, affine_sig])
    if force or _stale(target, sig):
        cmd = ["g++"] + HOST_FLAGS + ["-shared", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROCM, "include"),
                                     "-o", target] + srcs + [
            "-L", LIB, "-lgwaffine", "-lgwsemiglobal", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
            "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
        _run(cmd)
        _mark(target, sig)
    return target


def build_semiglobal(force=False):
    """libgwsemiglobal.so: the ends scan and the slice gather of the infix / prefix alignment types (hipcc, gfx950),
    linked against libgwhip.so, whose default aligner takes the gathered slices (built before this)."""
    header = os.path.join(ROOT, "include", "gwhip_semiglobal.h")
    jobs = [(HIPCC_OBJECT, src, _digest([src, header], KERNEL_FLAGS))
            for src in (os.path.join(PKG, s) for s in SEMIGLOBAL_KERNEL_SRCS)]
    return _build_library("libgwsemiglobal.so", jobs, ["-L", LIB, "-lgwhip", "-Wl,-rpath,$ORIGIN"], force)[0]


def build_affine(force=False):
    """libgwaffine.so: the affine-gap global aligner (hipcc, gfx950); it links nothing of the project."""
    header = os.path.join(ROOT, "include", "gwhip_affine.h")
    jobs = [(HIPCC_OBJECT, src, _digest([src, header] + _local_includes(src), KERNEL_FLAGS))
            for src in (os.path.join(PKG, s) for s in AFFINE_KERNEL_SRCS)]
    return _build_library("libgwaffine.so", jobs, [], force)[0]


def build_poa_hooks(force=False):
    """libgwhip_poa_hooks.so: test-only entry points onto device routines of csrc/ (hipcc, gfx950); nothing links it."""
    header = os.path.join(ROOT, "include", "gwhip_poa_hooks.h")
    jobs = [(HIPCC_OBJECT, src, _digest([src, header] + _local_includes(src), KERNEL_FLAGS))
            for src in (os.path.join(PKG, s) for s in POA_HOOKS_KERNEL_SRCS)]
    return _build_library("libgwhip_poa_hooks.so", jobs, [], force)[0]


def build_extender(force=False):
    """libcudaextender.so: the extension kernel + rocPRIM compaction / sort (hipcc, gfx950) and the Extender host
    classes (g++), linked against libgenomeworks_amd.so for the allocator and logging."""
    header = os.path.join(ROOT, "include", "gwhip_extender.h")
    host_sig = _digest(_deps("extender", (".cpp", ".h", ".hpp")), HOST_FLAGS)
    jobs = [(HIPCC_OBJECT, src, _digest([src, header], KERNEL_FLAGS))
            for src in (os.path.join(PKG, s) for s in EXTENDER_KERNEL_SRCS)]
    jobs += [(GXX_OBJECT, os.path.join(PKG, s), host_sig) for s in EXTENDER_HOST_SRCS]
    return _build_library("libcudaextender.so", jobs, ["-L", LIB, "-lgenomeworks_amd", "-Wl,-rpath,$ORIGIN"], force)[0]


def build_mapper(force=False):
    """libcudamapper.so: the sketch / index / matcher / overlapper / post-processing / overlap alignment / window
    segment / pileup / variant kernels with their rocPRIM scans, selects and sorts (hipcc, gfx950), linked against libgwhip.so for the
    aligner, and the Index / Matcher handles, the index batcher, the batched driver and the host rules of polishing and read correction
    behind the C API (g++);
    then bin/cudamapper, which links it and libgenomeworks_amd.so (built before this)."""
    headers = [os.path.join(ROOT, "include", "gwhip_mapper.h"), os.path.join(ROOT, "include", "gwhip.h"),
               os.path.join(ROOT, "include", "gwhip_affine.h")]
    host_sig = _digest(_deps("mapper", (".cpp", ".h", ".hpp")), HOST_FLAGS)
    jobs = [(HIPCC_OBJECT, src, _digest([src] + headers + _local_includes(src), KERNEL_FLAGS))
            for src in (os.path.join(PKG, s) for s in MAPPER_KERNEL_SRCS)]
    jobs += [(GXX_OBJECT, os.path.join(PKG, s), host_sig) for s in MAPPER_HOST_SRCS]
    # gwm_align.hip calls the default aligner of libgwhip.so and the affine-gap aligner of libgwaffine.so (built before this)
    target, link_sig = _build_library("libcudamapper.so", jobs, ["-L", LIB, "-lgwaffine", "-lgwhip", "-Wl,-rpath,$ORIGIN"], force)
    # the cudamapper tool: a thin main over the C API, the FASTA reader and PAF writer of libgenomeworks_amd.so
    _build_tool("cudamapper", os.path.join(PKG, "mapper", "cudamapper_main.cpp"), ["-lcudamapper"],
                _digest(_deps("host", (".hpp",)), [host_sig, link_sig]), force)
    return target


def _build_tool(name, src, more_libs, sig, force):
    """bin/<name> from one main source, linked against `more_libs` of lib/, libgenomeworks_amd.so, libgwhip.so and the
    HIP runtime, when its stamped signature is not `sig` (or on `force`)."""
    os.makedirs(os.path.join(PKG, "bin"), exist_ok=True)
    target = os.path.join(PKG, "bin", name)
    if force or _stale(target, sig):
        _run(["g++"] + [f for f in HOST_FLAGS if f != "-fPIC"] + INCLUDE +
             ["-I", os.path.join(ROCM, "include"), "-o", target, src, "-L", LIB] + more_libs +
             ["-lgenomeworks_amd", "-lgwaffine", "-lgwsemiglobal", "-lgwhip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath,$ORIGIN/../lib",
              "-Wl,-rpath," + os.path.join(ROCM, "lib")])
        _mark(target, sig)
    return target


def build_cli(force=False):
    """The command-line tools -> genomeworks_amd/bin/: `cudapoa` (reference: cudapoa/src/main.cpp) and
    `align_overlaps` (the alignment stage of cudamapper, cudamapper/src/main.cu:54-187)."""
    sig = _digest(_deps("host", (".cpp", ".h", ".hpp")), HOST_FLAGS)
    for tool, main_src in (("align_overlaps", "align_overlaps_main.cpp"), ("cudapoa", "cudapoa_main.cpp")):
        target = _build_tool(tool, os.path.join(PKG, "host", main_src), [], sig, force)
    return target


def build_bindings(force=False):
    """The Cython package `genomeworks` (pygenomeworks/, API of the reference's pygenomeworks): three extension modules
    built in-tree against include/ and libgenomeworks_amd.so. Returns the package's parent directory (for sys.path)."""
    pkg = os.path.join(ROOT, "pygenomeworks")
    srcs = []
    for d, _, fs in os.walk(os.path.join(pkg, "genomeworks")):
        srcs += [os.path.join(d, f) for f in fs if f.endswith((".pyx", ".pxd"))]
    srcs += [os.path.join(pkg, "setup.py")] + _deps("host", (".hpp",))
    sig = _digest(srcs, "cython")
    target = os.path.join(pkg, "genomeworks", "bindings")  # stamp only
    import glob
    built = all(glob.glob(os.path.join(pkg, "genomeworks", m, m + ".*.so")) for m in ("cuda", "cudapoa", "cudaaligner"))
    stamp = target + ".stamp"
    fresh = built and os.path.exists(stamp) and open(stamp).read().strip() == sig
    if force or not fresh:
        _run_in(pkg, [sys.executable, "setup.py", "-q", "build_ext", "--inplace", "--force"])
        with open(stamp, "w") as f:
            f.write(sig)
    return pkg


def _run_in(cwd, cmd):
    print("[build] (in %s)" % cwd, " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=cwd, stdout=subprocess.DEVNULL)


def build_all(force=False):
    k = build_kernels(force)
    build_semiglobal(force)
    build_affine(force)
    build_poa_hooks(force)
    h = build_host(force)
    build_extender(force)
    build_mapper(force)
    build_cli(force)
    build_bindings(force)
    return k, h


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
