"""The affine-gap global aligner without a GPU: the oracle against the stated cases and
against a second formulation, the shared rules header under the sanitizers, the libraries' exported symbols, and the
refusals that need no device."""
import ctypes as C
import os
import random
import subprocess

import pytest

import affine_cases as cases
import oracle_affine as O
import oracle_aligner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")


@pytest.mark.parametrize("q,t,scores,B,states,cost,optimal", cases.LITERAL)
def test_literal_cases(q, t, scores, B, states, cost, optimal):
    r = O.align(q, t, *scores, B)
    assert r["cost"] == cost and r["optimal"] == optimal
    if states is not None:
        assert r["states"] == states
    assert O.cost_of(r["states"], *scores) == cost
    O.replay(r["states"], q, t)


def test_unit_costs_scatter_the_gap_that_affine_costs_keep_whole():
    # the issue's smallest example: two gap runs at distance 3 under unit costs, one run and a mismatch under (4, 6, 2)
    unit = oracle_aligner.hirschberg("CGCGGA", "CGG")
    assert unit["edit_distance"] == 3 and unit["cigar"] == "2M1D1M2D"
    assert O.cigar(O.align("CGCGGA", "CGG", 4, 6, 2, 8)["states"]) == "1M3D2M"
    assert O.cost_of([0, 0, 3, 0, 3, 3], 4, 6, 2) == 18


def test_band_geometry():
    assert O.band(10, 10, 0) == (0, 0, 1)
    assert O.band(10, 14, 3) == (-3, 7, 11)
    assert O.band(14, 10, 3) == (-7, 3, 11)
    assert O.align("A" * 10, "A" * 10, 4, 6, 2, 1023)["cost"] == 0
    assert O.align("A" * 10, "A" * 11, 4, 6, 2, 1023)["cost"] == 8
    assert O.align("A" * 10, "A" * 10, 4, 6, 2, 1024) == dict(states=None, cost=-1, optimal=False)  # W = 2049


@pytest.fixture(scope="module")
def fuzz():
    """1 200 seeded pairs of 0-40 bases with a score set and a band each, aligned once in the band and once in full"""
    r = random.Random(7)
    out = []
    for q, t in cases.pairs(11, 1200, 40, max_error=0.5):
        scores, B = r.choice(cases.SCORE_SETS), r.choice([0, 1, 2, 5, 40])
        out.append((q, t, scores, B, O.align(q, t, *scores, B), O.align(q, t, *scores, 100)))
    return out


def test_the_two_formulations_agree(fuzz):
    seen = set()
    for q, t, scores, B, banded, full in fuzz:
        seen.add(scores)
        assert full["cost"] == O.gotoh_cost(q, t, *scores), (q, t, scores)
        for r in (banded, full):
            assert O.cost_of(r["states"], *scores) == r["cost"], (q, t, scores, B)
            O.replay(r["states"], q, t)
        assert banded["cost"] >= full["cost"]
    assert seen == set(cases.SCORE_SETS)


def test_unit_scores_in_a_full_band_give_the_edit_distance(fuzz):
    checked = 0
    for q, t, scores, B, banded, full in fuzz:
        if scores == (1, 0, 1) and (q or t):
            assert full["cost"] == oracle_aligner.hirschberg(q, t)["edit_distance"], (q, t)
            checked += 1
    assert checked > 100


def test_the_flag_means_the_full_band_cost(fuzz):
    flagged = worse = 0
    for q, t, scores, B, banded, full in fuzz:
        if banded["optimal"]:
            flagged += 1
            assert banded["cost"] == full["cost"], (q, t, scores, B)
        elif banded["cost"] > full["cost"]:
            worse += 1
    assert flagged > 500 and worse >= 1


def _sanitized_cases():
    """cases for the stand-alone program: the literal ones, seeded ones over the score sets, and the lane-block and
    capacity edges W = 63, 64, 65, 2048, 2049"""
    out = [(q, t, s, B) for q, t, s, B, _, _, _ in cases.LITERAL]
    r = random.Random(3)
    for q, t in cases.pairs(5, 150, 60, max_error=0.4):
        out.append((q, t, r.choice(cases.SCORE_SETS), r.choice([0, 1, 3, 8, 33])))
    for W, difference, B in ((63, 0, 31), (64, 1, 31), (64, -1, 31), (65, 0, 32), (65, 2, 31)):
        out.append(cases.pair_with_band(W + difference, 90, difference, 0.25) + (cases.DEFAULT, B))
        assert O.band(90, 90 + difference, B)[2] == W
    out.append(cases.pair_with_band(21, 40, 1) + (cases.DEFAULT, 1023))   # W = 2048
    out.append(cases.pair_with_band(22, 40, -1) + ((2, 3, 1), 1023))      # W = 2048
    out.append(cases.pair_with_band(23, 40, 0) + (cases.DEFAULT, 1024))   # W = 2049: no result
    out.append(cases.pair_with_band(24, 40, 2) + (cases.DEFAULT, 1023))   # W = 2049: no result
    return out


def test_shared_header_under_the_sanitizers(tmp_path):
    exe, listing = str(tmp_path / "affine_cells_sanitized"), str(tmp_path / "cases.txt")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "genomeworks_amd", "affine"), os.path.join(ROOT, "tests", "cpp", "affine_cells_sanitized.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    todo = _sanitized_cases()
    with open(listing, "w") as f:
        for q, t, (x, o, e), B in todo:
            f.write("%s %s %d %d %d %d\n" % (q or "-", t or "-", x, o, e, B))
    r = subprocess.run([exe, listing], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo)
    no_result = 0
    for line, (q, t, scores, B) in zip(lines, todo):
        want = O.align(q, t, *scores, B)
        cost, optimal, length, states = line.split()
        if want["states"] is None:
            no_result += 1
            assert (cost, optimal, length, states) == ("-1", "0", "0", "-"), (line, q, t, scores, B)
            continue
        got = [] if states == "-" else [int(c) for c in states]
        assert (int(cost), bool(int(optimal)), int(length), got) == (want["cost"], want["optimal"], len(want["states"]), want["states"]), \
            (line, q, t, scores, B)
    assert no_result == 2


def _exported(library):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, library)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}


def test_exported_symbols():
    affine = _exported("libgwaffine.so")
    assert {"gwhip_affine_workspace_bytes", "gwhip_affine_align", "gwhip_affine_align_events", "gwhip_affine_last_error"} <= affine
    assert not any(s.startswith(("gwhip_hirschberg", "gwhip_myers", "gwhip_poa")) for s in affine)  # on its own
    host = _exported("libgenomeworks_amd.so")
    assert {"gw_aligner_create_affine", "gw_alignment_cost"} <= host
    assert any("create_aligner_affine" in s for s in host) and any("get_alignment_cost" in s for s in host)
    mapper = _exported("libcudamapper.so")
    assert {"gwm_align_overlaps_scored", "gwm_overlap_variants_scored", "gwm_align_bytes_needed_scored",
            "gw_mapper_align_overlaps_scored", "gw_mapper_overlap_variants_scored",
            "gwm_align_overlaps", "gwm_overlap_variants", "gwm_align_bytes_needed"} <= mapper
    from genomeworks_amd import build as B
    assert B.AFFINE_KERNEL_SRCS == ["affine/gwaffine.hip"]
    assert all(not s.startswith("affine/") for s in B.KERNEL_SRCS + B.HOST_SRCS)  # outside the stamped kernel set


class _Args(C.Structure):
    _fields_ = [("n_alignments", C.c_int32), ("sequences", C.c_void_p), ("sequence_starts", C.c_void_p),
                ("sequence_starts_host", C.POINTER(C.c_int64)), ("mismatch", C.c_int32), ("gap_open", C.c_int32),
                ("gap_extend", C.c_int32), ("band", C.c_int32), ("results", C.c_void_p), ("result_lengths", C.c_void_p),
                ("costs", C.c_void_p), ("optimal", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


def test_kernel_level_sizes_and_refusals_without_a_device():
    L = C.CDLL(os.path.join(LIB, "libgwaffine.so"))
    L.gwhip_affine_workspace_bytes.restype = C.c_size_t
    L.gwhip_affine_workspace_bytes.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_int32]
    L.gwhip_affine_align.argtypes = [C.POINTER(_Args), C.c_void_p]
    L.gwhip_affine_last_error.restype = C.c_char_p
    starts = (C.c_int64 * 5)(0, 100, 210, 215, 515)  # (100, 110) and (5, 300)
    # offsets, then (n + m + 1) rows of roundup4((W + 2) / 2) bytes a pair, each part rounded up to 256
    def part(n, m, B):
        W = abs(m - n) + 2 * B + 1
        return ((n + m + 1) * ((((W + 2) // 2) + 3) & ~3) + 255) & ~255
    assert L.gwhip_affine_workspace_bytes(2, starts, 16) == 256 + part(100, 110, 16) + part(5, 300, 16)
    assert L.gwhip_affine_workspace_bytes(2, starts, 1024) == 256  # neither pair is aligned: W > 2048
    # nothing below reaches a device: every call is refused on the host
    fake = 0x1000
    def call(**over):
        a = _Args(2, fake, fake, starts, 4, 6, 2, 16, fake, fake, fake, fake, fake, 1 << 30)
        for k, v in over.items():
            setattr(a, k, v)
        return L.gwhip_affine_align(C.byref(a), None), L.gwhip_affine_last_error().decode()
    for bad in (dict(mismatch=0), dict(mismatch=256), dict(gap_open=-1), dict(gap_open=256), dict(gap_extend=0),
                dict(gap_extend=256), dict(band=-1), dict(n_alignments=-1)):
        rc, text = call(**bad)
        assert rc != 0 and "gwhip_affine_align" in text, bad
    rc, text = call(workspace_bytes=L.gwhip_affine_workspace_bytes(2, starts, 16) - 1)
    assert rc != 0 and "workspace" in text
    rc, text = call(results=None)
    assert rc != 0 and "null" in text
    assert call(n_alignments=0)[0] == 0  # an empty batch launches nothing


def test_python_refusals_without_a_device():
    from genomeworks_amd import cudaaligner, cudamapper
    for keyword in ("mismatch", "gap_open", "gap_extend", "band_width"):
        with pytest.raises(RuntimeError, match=keyword):
            cudaaligner.CudaAlignerBatch(100, 100, 10, **{keyword: 3})
        with pytest.raises(RuntimeError, match=keyword):
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="ukkonen", **{keyword: 3})
    with pytest.raises(RuntimeError):
        cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", alignment_type="infix")
    for bad in (dict(mismatch=0), dict(mismatch=256), dict(gap_open=-1), dict(gap_open=256), dict(gap_extend=0),
                dict(gap_extend=256), dict(band_width=-1)):
        with pytest.raises(RuntimeError, match="outside|non-negative"):
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", **bad)
    for bad in ((0, 6, 2, 64), (256, 6, 2, 64), (4, -1, 2, 64), (4, 256, 2, 64), (4, 6, 0, 64), (4, 6, 256, 64),
                (4, 6, 2, -1), (4, 6, 2), dict(mismatch=0), dict(gap=3)):
        with pytest.raises(ValueError):
            cudamapper._scoring_args(bad)
    assert cudamapper._scoring_args(None) is None
    assert list(cudamapper._scoring_args(dict(band=64))) == [4, 6, 2, 64]
    assert list(cudamapper._scoring_args((1, 0, 1, 7))) == [1, 0, 1, 7]
    # host arithmetic: the budget of one overlap grows with the band and with the slices
    narrow, wide = cudamapper.align_bytes_needed_scored(800, 800, 16), cudamapper.align_bytes_needed_scored(800, 800, 256)
    assert 1601 * 16 < narrow < wide and wide > 1601 * 256
