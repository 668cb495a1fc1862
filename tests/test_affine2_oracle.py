"""The two-piece affine-gap global aligner without a GPU: the oracle against the stated
cases, its three formulations against one another and against the one-piece oracle, the rules header under the
sanitizers, the libraries' exported symbols, and the refusals that need no device."""
import ctypes as C
import os
import random
import subprocess

import pytest

import affine2_cases as cases
import oracle_affine as O1
import oracle_affine2 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")


@pytest.mark.parametrize("q,t,scores,B,cost,longest,optimal", cases.LITERAL)
def test_literal_cases(q, t, scores, B, cost, longest, optimal):
    r = O.align(q, t, *scores, B)
    assert r["cost"] == cost and r["optimal"] == optimal
    assert O.cost_of(r["states"], *scores) == cost
    if longest is not None:
        assert O.runs(r["states"]) == [longest]  # one run, nothing scattered
    O.replay(r["states"], q, t)


def test_the_second_piece_is_what_makes_the_long_run_cheap():
    q, t = cases.LITERAL[0][:2]
    assert O1.align(q, t, *cases.ONE_PIECE, 40)["cost"] == 94   # 4 + 3 * 30
    assert O.align(q, t, *cases.DEFAULT, 40)["cost"] == 84      # 24 + 2 * 30
    q, t = cases.LITERAL[2][:2]
    assert O1.align(q, t, *cases.ONE_PIECE, 40)["cost"] == 64 == O.align(q, t, *cases.DEFAULT, 40)["cost"]
    assert [O.g(L, 4, 3, 24, 2) for L in (1, 19, 20, 21)] == [7, 61, 64, 66]  # the pieces cross at L = 20


def test_a_tie_between_the_pieces_goes_to_the_first():
    # 20 inserted bases: 4 + 3 * 20 == 24 + 2 * 20. H takes E1 before E2, so the walk is in E1: the same states as the
    # one-piece aligner's, which has nothing else
    q, t = cases.LITERAL[2][:2]
    assert O.align(q, t, *cases.DEFAULT, 40)["states"] == O1.align(q, t, *cases.ONE_PIECE, 40)["states"]


def test_capacity():
    assert O.align("A" * 10, "A" * 11, *cases.DEFAULT, 511)["cost"] == 7                              # W = 1024
    assert O.align("A" * 10, "A" * 10, *cases.DEFAULT, 512) == dict(states=None, cost=-1, optimal=False)  # W = 1025


def test_the_bound_with_one_piece_is_the_one_piece_bound():
    for n, m, o, e, B in ((10, 10, 6, 2, 0), (5, 300, 0, 1, 7), (300, 5, 255, 255, 200)):
        assert O.bound(n, m, o, e, o, e, B) == O1.bound(n, m, 1, o, e, B)


@pytest.fixture(scope="module")
def fuzz():
    """per score set 60 seeded pairs of 0-25 bases, aligned in a band each and in full, with the two other formulations"""
    r = random.Random(17)
    out = []
    for k, scores in enumerate(cases.SCORE_SETS):
        for q, t in cases.pairs(100 + k, 60, 25, max_error=0.5):
            B = r.choice([0, 1, 2, 5])
            out.append((q, t, scores, B, O.align(q, t, *scores, B), O.align(q, t, *scores, 100)))
    return out


def test_the_three_formulations_agree(fuzz):
    for q, t, scores, B, banded, full in fuzz:
        assert full["cost"] == O.five_matrix_cost(q, t, *scores) == O.general_gap_cost(q, t, *scores), (q, t, scores)
        for r in (banded, full):
            assert O.cost_of(r["states"], *scores) == r["cost"], (q, t, scores, B)
            O.replay(r["states"], q, t)
        assert banded["cost"] >= full["cost"]


def test_the_flag_means_the_full_matrix_cost(fuzz):
    flagged = worse = 0
    for q, t, scores, B, banded, full in fuzz:
        if banded["optimal"]:
            flagged += 1
            assert banded["cost"] == full["cost"], (q, t, scores, B)
        elif banded["cost"] > full["cost"]:
            worse += 1
    assert flagged > 150 and worse >= 1


def test_a_dominated_or_identical_second_piece_is_the_one_piece_aligner(fuzz):
    checked = 0
    for q, t, scores, B, banded, full in fuzz:
        if scores in (cases.DOMINATED, cases.IDENTICAL):
            assert banded == O1.align(q, t, *scores[:3], B) and full == O1.align(q, t, *scores[:3], 100), (q, t, scores, B)
            checked += 1
    assert checked == 120


def _sanitized_cases():
    """cases for the stand-alone program: the literal ones, seeded ones over the score sets, and the lane-block and
    capacity edges W = 63, 64, 65, 1024, 1025"""
    out = [(q, t, s, B) for q, t, s, B, _, _, _ in cases.LITERAL]
    r = random.Random(3)
    for q, t in cases.spliced_pairs(5, 150, 60, max_error=0.4):
        out.append((q, t, r.choice(cases.SCORE_SETS), r.choice([0, 1, 3, 8, 33])))
    for W, difference, B in ((63, 0, 31), (64, 1, 31), (64, -1, 31), (65, 0, 32), (65, 2, 31)):
        out.append(cases.pair_with_band(W + difference, 90, difference, 0.25) + (cases.DEFAULT, B))
        assert O.band(90, 90 + difference, B)[2] == W
    out.append(cases.pair_with_band(21, 40, 1) + (cases.DEFAULT, 511))            # W = 1024
    out.append(cases.pair_with_band(22, 40, -1) + ((2, 255, 1, 0, 3), 511))       # W = 1024
    out.append(cases.pair_with_band(23, 40, 0) + (cases.DEFAULT, 512))            # W = 1025: no result
    out.append(cases.pair_with_band(24, 40, 2) + (cases.DEFAULT, 511))            # W = 1025: no result
    return out


def test_rules_header_under_the_sanitizers(tmp_path):
    exe, listing = str(tmp_path / "affine2_cells_sanitized"), str(tmp_path / "cases.txt")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "genomeworks_amd", "affine"), os.path.join(ROOT, "tests", "cpp", "affine2_cells_sanitized.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    todo = _sanitized_cases()
    with open(listing, "w") as f:
        for q, t, scores, B in todo:
            f.write("%s %s %d %d %d %d %d %d\n" % ((q or "-", t or "-") + tuple(scores) + (B,)))
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
    assert {"gwhip_affine2_workspace_bytes", "gwhip_affine2_align", "gwhip_affine2_align_events"} <= _exported("libgwaffine.so")
    host = _exported("libgenomeworks_amd.so")
    assert "gw_aligner_create_affine2" in host
    assert sum("create_aligner_affine" in s and "TwoPieceScoring" in s for s in host) == 2
    assert {"gwm_align_overlaps_scored2", "gwm_overlap_variants_scored2", "gw_mapper_align_overlaps_scored2",
            "gw_mapper_overlap_variants_scored2"} <= _exported("libcudamapper.so")


class _Args2(C.Structure):
    _fields_ = [("n_alignments", C.c_int32), ("sequences", C.c_void_p), ("sequence_starts", C.c_void_p),
                ("sequence_starts_host", C.POINTER(C.c_int64)), ("mismatch", C.c_int32), ("gap_open", C.c_int32),
                ("gap_extend", C.c_int32), ("gap_open2", C.c_int32), ("gap_extend2", C.c_int32), ("band", C.c_int32),
                ("results", C.c_void_p), ("result_lengths", C.c_void_p), ("costs", C.c_void_p), ("optimal", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


def _part(n, m, B):
    """bytes of one aligned pair's bit matrix: (n + m + 1) rows of roundup4((W + 2) / 2), rounded up to 256"""
    W = abs(m - n) + 2 * B + 1
    return ((n + m + 1) * ((((W + 2) // 2) + 3) & ~3) + 255) & ~255


def test_kernel_level_sizes_and_refusals_without_a_device():
    L = C.CDLL(os.path.join(LIB, "libgwaffine.so"))
    for f in (L.gwhip_affine_workspace_bytes, L.gwhip_affine2_workspace_bytes):
        f.restype = C.c_size_t
        f.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_int32]
    L.gwhip_affine2_align.argtypes = [C.POINTER(_Args2), C.c_void_p]
    L.gwhip_affine_last_error.restype = C.c_char_p
    assert C.sizeof(_Args2) == 104  # gwhip_affine_args (96 bytes) and two int32 more
    starts = (C.c_int64 * 5)(0, 100, 210, 215, 515)  # (100, 110) and (5, 300)
    assert L.gwhip_affine2_workspace_bytes(2, starts, 16) == 256 + _part(100, 110, 16) + _part(5, 300, 16)
    # the capacity: W = |m - n| + 2 B + 1 = 1024 counts, 1025 does not (the one-piece aligner counts both)
    edge = (C.c_int64 * 5)(0, 100, 201, 301, 401)  # (100, 101) and (100, 100)
    assert L.gwhip_affine2_workspace_bytes(2, edge, 511) == 256 + _part(100, 101, 511) + _part(100, 100, 511)
    assert L.gwhip_affine2_workspace_bytes(2, edge, 512) == 256
    assert L.gwhip_affine_workspace_bytes(2, edge, 512) == 256 + _part(100, 101, 512) + _part(100, 100, 512)
    wide = (C.c_int64 * 3)(0, 100, 202)  # (100, 102) at B = 511: W = 1025
    assert L.gwhip_affine2_workspace_bytes(1, wide, 511) == 256
    # nothing below reaches a device: every call is refused on the host
    fake = 0x1000

    def call(**over):
        a = _Args2(2, fake, fake, starts, 6, 4, 3, 24, 2, 16, fake, fake, fake, fake, fake, 1 << 30)
        for k, v in over.items():
            setattr(a, k, v)
        return L.gwhip_affine2_align(C.byref(a), None), L.gwhip_affine_last_error().decode()
    for bad in (dict(mismatch=0), dict(mismatch=256), dict(gap_open=-1), dict(gap_open=256), dict(gap_extend=0),
                dict(gap_extend=256), dict(gap_open2=-1), dict(gap_open2=256), dict(gap_extend2=0), dict(gap_extend2=256),
                dict(band=-1), dict(n_alignments=-1)):
        rc, text = call(**bad)
        assert rc != 0 and "gwhip_affine2_align" in text, bad
    rc, text = call(workspace_bytes=L.gwhip_affine2_workspace_bytes(2, starts, 16) - 1)
    assert rc != 0 and "workspace" in text
    rc, text = call(results=None)
    assert rc != 0 and "null" in text
    assert call(n_alignments=0)[0] == 0  # an empty batch launches nothing


def test_python_refusals_without_a_device():
    from genomeworks_amd import cudaaligner, cudamapper
    for keyword, other in (("gap_open2", "gap_extend2"), ("gap_extend2", "gap_open2")):
        with pytest.raises(RuntimeError, match=keyword):  # alone
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", **{keyword: 3})
        for algorithm in (None, "ukkonen"):               # with another aligner
            with pytest.raises(RuntimeError, match=keyword):
                cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm=algorithm, **{keyword: 3, other: 3})
    for bad in (dict(gap_open2=-1, gap_extend2=2), dict(gap_open2=256, gap_extend2=2)):
        with pytest.raises(RuntimeError, match="gap_open2"):
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", **bad)
    for bad in (dict(gap_open2=24, gap_extend2=0), dict(gap_open2=24, gap_extend2=256)):
        with pytest.raises(RuntimeError, match="gap_extend2"):
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", **bad)
    with pytest.raises(RuntimeError, match="mismatch"):
        cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="affine", mismatch=0, gap_open2=24, gap_extend2=2)


def test_scoring_args():
    from genomeworks_amd import cudamapper
    f = cudamapper._scoring_args
    assert list(f((6, 4, 3, 24, 2, 64))) == [6, 4, 3, 24, 2, 64]
    assert list(f(dict(gap_open2=24, gap_extend2=2))) == [6, 4, 3, 24, 2, 128]
    assert list(f(dict(gap_open2=9, gap_extend2=1, mismatch=5, gap_open=0, band=7))) == [5, 0, 3, 9, 1, 7]
    for bad in ((0, 4, 3, 24, 2, 64), (6, 256, 3, 24, 2, 64), (6, 4, 0, 24, 2, 64), (6, 4, 3, -1, 2, 64),
                (6, 4, 3, 256, 2, 64), (6, 4, 3, 24, 0, 64), (6, 4, 3, 24, 256, 64), (6, 4, 3, 24, 2, -1),
                (6, 4, 3, 24, 2), (6, 4, 3, 24, 2, 64, 1), dict(gap_open2=24), dict(gap_extend2=2),
                dict(gap_open2=24, gap_extend2=2, gap_open3=1), dict(gap_open2=24, gap_extend2=0)):
        with pytest.raises(ValueError):
            f(bad)
    # the old forms mean what they meant
    assert f(None) is None
    assert list(f((1, 0, 1, 7))) == [1, 0, 1, 7]
    assert list(f(dict(band=64))) == [4, 6, 2, 64]
    assert list(f(dict())) == [4, 6, 2, 128]
    with pytest.raises(ValueError):
        f((4, 6, 2))
