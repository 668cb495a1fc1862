"""The registry of GWHIP_DEBUG (genomeworks_amd/csrc/poa_debug_flags.h) and the list of the kernel library's environment
switches (gwhip_switches.h) stay the only place where a number or a name is spelt out: the Python names equal the header's,
no device source tests a literal bit, no launch file reads the environment itself, and INTEGRATION.md lists the switches the
header reads. Source text only; no GPU and no build is needed."""
import glob
import os
import re

from genomeworks_amd import debug_flags as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genomeworks_amd", "csrc")


def read(path):
    with open(path) as f:
        return f.read()


def header_constants():
    """name -> value of every kDbg... constant of poa_debug_flags.h: the X(kind, name, bits) lines of the table and the
    `constexpr int32_t name = value` definitions of the fields' shifts, masks and values."""
    text = read(os.path.join(CSRC, "poa_debug_flags.h"))
    found = re.findall(r"\bX\(\s*(?:AB|ABL|PROF)\s*,\s*(kDbg\w+)\s*,\s*([0-9 <]+?)\s*\)", text)
    for line in re.findall(r"^constexpr int32_t (kDbg[^;(]*);", text, re.M):
        found += re.findall(r"(kDbg\w+)\s*=\s*([0-9 <]+)", line)
    out = {}
    for name, expr in found:
        assert name not in out, name
        assert re.fullmatch(r"\d+( << \d+)?", expr.strip()), (name, expr)
        out[name] = eval(expr)
    return out


def test_python_names_equal_the_header_name_by_name():
    header = header_constants()
    python = {k: v for k, v in vars(D).items() if k.startswith("kDbg") and isinstance(v, int)}
    assert len(header) > 70  # the table and the field values were found at all
    assert sorted(header) == sorted(python)
    for name in header:
        assert header[name] == python[name], name
    assert all(0 < v < 1 << 31 for v in header.values())
    for kind in range(7):
        assert D.kDbgRowKindSelect(kind) == (kind + 1) << header["kDbgRowKindShift"]
        assert int(D.env_value(D.kDbgKindFine, D.kDbgKindCount, row_kind=kind)) == ((kind + 1) << 28) | (1 << 13) | (1 << 12)
    assert D.env_value(D.kDbgRingToGeneral, D.kDbgRegistersToGeneral, D.kDbgManyPredsToGeneral) == str((1 << 9) | (1 << 11) | (1 << 30))
    assert D.env_value(tb=D.kDbgTbStepCycles, skew=D.kDbgSkewPolls) == str((4 << 22) | (9 << 12))


# a flag word or a selector taken from it, followed by & or >> and a number, or compared with one
LITERAL_TESTS = (re.compile(r"\b(?:\w*dbg|\w*debug_flags)\s*(?:&|>>)\s*\(?\s*(?:0x)?\d"),
                 re.compile(r"\b(?:sksel|psel|tsel|prof_sel)\s*[=!]=\s*\d"),
                 re.compile(r"\bprof_mark\(\s*\d"))


def literal_tests(text):
    hits = []
    for number, line in enumerate(text.splitlines(), 1):
        code = line.split("//")[0]
        if any(p.search(code) for p in LITERAL_TESTS):
            hits.append((number, line.strip()))
    return hits


def test_the_search_for_literal_tests_finds_the_forms_the_sources_used_to_have():
    for line in ("if (!(dbg & 256)) x();", "f((dbg & (1 << 25)) != 0);", "const int32_t psel = prof_acc ? (dbg >> 22) & 7 : 0;",
                 "const int32_t sksel = PROF ? (A.dbg >> 12) & 15 : 0;", "g((a.debug_flags & 16) != 0);", "if (sksel == 9) skacc++;",
                 "if (!(debug_flags & (1 << 21)))", "prof_mark(3);", "const uint64_t t = tsel == 1 ? clock64() : 0;"):
        assert literal_tests(line), line
    for line in ("if (!(dbg & kDbgNoPackedPasses)) x();", "if (sksel == kDbgSkewPolls) skacc++;", "// bit 8: dbg & 256",
                 "const int32_t tsel = prof_acc ? (dbg >> kDbgTopsortShift) & kDbgTopsortMask : 0;", "if (ksel >= 0 && lane == 0) y();"):
        assert not literal_tests(line), line


def test_no_device_source_tests_a_literal_bit_of_the_flag_word():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) +
                   glob.glob(os.path.join(ROOT, "genomeworks_amd", "poa_hooks", "*")) + [os.path.join(ROOT, "tools", "microbench_rows.hip")])
    assert len(paths) > 25
    hits = {os.path.relpath(p, ROOT): literal_tests(read(p)) for p in paths}
    assert {p: h for p, h in hits.items() if h} == {}


def test_launch_files_leave_the_environment_to_the_switches_header():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        assert "getenv" not in read(path), path
    header = read(os.path.join(CSRC, "gwhip_switches.h"))
    read_by_the_code = set(re.findall(r'"(GWHIP_[A-Z_]+)"', header))
    in_the_header_table = set(re.findall(r"^//   (GWHIP_[A-Z_]+) ", header, re.M))
    in_integration_md = set(re.findall(r"^\s*\| `(GWHIP_[A-Z_]+)` \|", read(os.path.join(ROOT, "INTEGRATION.md")), re.M))
    assert len(read_by_the_code) == 12
    assert read_by_the_code == in_the_header_table
    assert read_by_the_code == in_integration_md
