"""The affine X-drop extension without a GPU: the oracle against the stated cases, its banded
formulation against the plain score-form DP, the rules header under the sanitizers, the libraries' exported symbols, the
argument struct's layout and the refusals that need no device."""
import ctypes as C
import os
import random
import subprocess

import pytest

import extend_cases as cases
import oracle_extend as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeworks_amd", "lib")


@pytest.mark.parametrize("q,t,B,X,ends,score,dropped,states", cases.LITERAL)
def test_literal_cases(q, t, B, X, ends, score, dropped, states):
    r = O.extend(q, t, *cases.DEFAULT, B, X)
    assert (r["query_end"], r["target_end"]) == ends and r["score"] == score
    if dropped is not None:
        assert r["dropped"] == dropped
    assert r["states"] == states and len(r["states"]) == len(states)
    assert O.score_of(r["states"], *cases.DEFAULT) == score


@pytest.fixture(scope="module")
def fuzz():
    """per score set 70 seeded pairs of 0-40 bases: (q, t, scores, the extension at X = -1 in a band that covers the matrix)"""
    out = []
    for k, scores in enumerate(cases.SCORE_SETS):
        for q, t in cases.pairs(300 + k, 70, 40):
            out.append((q, t, scores, O.extend(q, t, *scores, 64, -1)))
    assert len(out) >= 400
    return out


def test_the_banded_extension_finds_the_plain_maximum(fuzz):
    positive = 0
    for q, t, scores, r in fuzz:
        best, where = O.plain_best(q, t, *scores)
        assert r["score"] == best and (r["query_end"], r["target_end"]) in where, (q, t, scores)
        assert r["dropped"] == 0
        assert O.score_of(r["states"], *scores) == r["score"], (q, t, scores)
        assert O.consumed(r["states"]) == (r["query_end"], r["target_end"]), (q, t, scores)
        O.replay(r["states"], q[:r["query_end"]], t[:r["target_end"]])
        positive += r["score"] > 0
    assert positive > 300


def test_a_finite_xdrop_never_scores_more_and_says_when_it_stopped(fuzz):
    smaller = 0
    r = random.Random(5)
    for q, t, scores, free in fuzz:
        X = r.choice([0, 1, 3, 10])
        got = O.extend(q, t, *scores, 64, X)
        assert got["score"] <= free["score"], (q, t, scores, X)
        assert O.score_of(got["states"], *scores) == got["score"]
        if got["score"] < free["score"]:
            smaller += 1
            assert got["dropped"] == 1, (q, t, scores, X)
    assert smaller >= 1


def test_a_narrow_band_never_scores_more(fuzz):
    for q, t, scores, free in fuzz[::3]:
        for B in (0, 1, 3):
            got = O.extend(q, t, *scores, B, -1)
            assert got["score"] <= free["score"]
            assert all(abs(j - i) <= B for i, j in _cells(got["states"]))


def _cells(states):
    i = j = 0
    yield i, j
    for s in states:
        i += s != 2
        j += s != 3
        yield i, j


def _sanitized_cases():
    """cases for the stand-alone program: the literal ones, seeded ones over the score sets, W = 63, 65, 127, 129, 1023,
    B = 0, empty sequences, 5 against 300 bases and the reverse"""
    out = [(q, t, cases.DEFAULT, B, X) for q, t, B, X, _, _, _, _ in cases.LITERAL]
    r = random.Random(3)
    for q, t in cases.pairs(7, 120, 90):
        out.append((q, t, r.choice(cases.SCORE_SETS), r.choice([0, 1, 3, 8, 33]), r.choice([0, 5, 30, 200, -1])))
    wide = cases.pairs(8, 12, 200)
    for k, B in enumerate((31, 32, 63, 64, 511, 0)):
        for X in (20, -1):
            q, t = wide[2 * k + (X < 0)]
            out.append((q, t, cases.DEFAULT, B, X))
    short, long_ = cases.random_sequence(r, 5), cases.random_sequence(r, 300)
    for B in (0, 7, 511):
        out += [(short, short + long_, cases.DEFAULT, B, -1), (short + long_, short, cases.DEFAULT, B, 50),
                ("", long_, cases.DEFAULT, B, -1), (long_, "", (63, 64, 127, 96), B, 0), ("", "", cases.DEFAULT, B, 0)]
    return out


def test_rules_header_under_the_sanitizers(tmp_path):
    exe, listing = str(tmp_path / "extend_cells_sanitized"), str(tmp_path / "cases.txt")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "genomeworks_amd", "affine"), os.path.join(ROOT, "tests", "cpp", "extend_cells_sanitized.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    todo = _sanitized_cases()
    with open(listing, "w") as f:
        for q, t, scores, B, X in todo:
            f.write("%s %s %d %d %d %d %d %d\n" % ((q or "-", t or "-") + tuple(scores) + (B, X)))
    r = subprocess.run([exe, listing], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo)
    dropped = 0
    for line, (q, t, scores, B, X) in zip(lines, todo):
        want = O.extend(q, t, *scores, B, X)
        query_end, target_end, score, flag, length, states = line.split()
        got = [] if states == "-" else [int(c) for c in states]
        assert (int(query_end), int(target_end), int(score), int(flag), int(length), got) == \
            (want["query_end"], want["target_end"], want["score"], want["dropped"], len(want["states"]), want["states"]), \
            (line, q, t, scores, B, X)
        dropped += want["dropped"]
    assert 10 <= dropped <= len(todo) - 10


def _exported(library):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, library)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}


def test_exported_symbols():
    assert {"gwhip_extend_workspace_bytes", "gwhip_extend", "gwhip_extend_events"} <= _exported("libgwaffine.so")
    host = _exported("libgenomeworks_amd.so")
    assert {"gw_aligner_create_extension", "gw_alignment_extension"} <= host
    assert sum("create_aligner_extension" in s and "ExtensionScoring" in s for s in host) == 2
    assert any("get_alignment_extension" in s for s in host)
    assert not any("create_aligner_affine" in s and "Extension" in s for s in host)
    assert {"gwm_extend_overlaps", "gw_mapper_extend_overlaps"} <= _exported("libcudamapper.so")


class _Args(C.Structure):
    _fields_ = [("n_alignments", C.c_int32), ("sequences", C.c_void_p), ("sequence_starts", C.c_void_p),
                ("sequence_starts_host", C.POINTER(C.c_int64)), ("match", C.c_int32), ("mismatch", C.c_int32),
                ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("band", C.c_int32), ("xdrop", C.c_int32),
                ("results", C.c_void_p), ("result_lengths", C.c_void_p), ("scores", C.c_void_p), ("query_ends", C.c_void_p),
                ("target_ends", C.c_void_p), ("dropped", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class _AffineArgs(C.Structure):
    _fields_ = [("n_alignments", C.c_int32), ("sequences", C.c_void_p), ("sequence_starts", C.c_void_p),
                ("sequence_starts_host", C.POINTER(C.c_int64)), ("mismatch", C.c_int32), ("gap_open", C.c_int32),
                ("gap_extend", C.c_int32), ("band", C.c_int32), ("results", C.c_void_p), ("result_lengths", C.c_void_p),
                ("costs", C.c_void_p), ("optimal", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


def test_the_argument_structs():
    assert C.sizeof(_Args) == 120
    offsets = {name: getattr(_Args, name).offset for name, _ in _Args._fields_}
    assert offsets == dict(n_alignments=0, sequences=8, sequence_starts=16, sequence_starts_host=24, match=32, mismatch=36,
                           gap_open=40, gap_extend=44, band=48, xdrop=52, results=56, result_lengths=64, scores=72,
                           query_ends=80, target_ends=88, dropped=96, workspace=104, workspace_bytes=112)
    assert C.sizeof(_AffineArgs) == 96
    import test_affine2_oracle
    assert C.sizeof(test_affine2_oracle._Args2) == 104


def _library():
    L = C.CDLL(os.path.join(LIB, "libgwaffine.so"))
    L.gwhip_extend_workspace_bytes.restype = C.c_size_t
    L.gwhip_extend_workspace_bytes.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32]
    L.gwhip_extend.argtypes = [C.POINTER(_Args), C.c_void_p]
    L.gwhip_affine_last_error.restype = C.c_char_p
    return L


def test_workspace_bytes():
    L = _library()
    starts = (C.c_int64 * 5)(0, 100, 210, 215, 515)  # (100, 110) and (5, 300)
    for B in (0, 16, 511):
        want = 256 + O.bits_bytes(100, 110, B) + O.bits_bytes(5, 300, B)
        assert L.gwhip_extend_workspace_bytes(2, starts, B, 1) == want
        assert L.gwhip_extend_workspace_bytes(2, starts, B, 0) == 0
    # (a_max + 1) rows of roundup4((2 B + 3) / 2) bytes
    assert O.bits_bytes(100, 110, 16) == ((min(210, 216) + 1) * 20 + 255) & ~255
    assert O.bits_bytes(5, 300, 16) == ((min(305, 26) + 1) * 20 + 255) & ~255


def test_kernel_level_refusals_without_a_device():
    L = _library()
    starts = (C.c_int64 * 5)(0, 100, 210, 215, 515)
    fake = 0x1000  # nothing below reaches a device: every call is refused on the host

    def call(**over):
        a = _Args(2, fake, fake, starts, 2, 4, 4, 2, 16, 200, fake, fake, fake, fake, fake, fake, fake, 1 << 30)
        for k, v in over.items():
            setattr(a, k, v)
        return L.gwhip_extend(C.byref(a), None), L.gwhip_affine_last_error().decode()
    for bad in (dict(band=512), dict(band=-1), dict(match=64, mismatch=64), dict(match=0), dict(mismatch=-1), dict(gap_open=128),
                dict(gap_open=-1), dict(gap_extend=0), dict(match=2, gap_extend=127), dict(xdrop=-2), dict(xdrop=(1 << 20) + 1),
                dict(n_alignments=-1)):
        rc, text = call(**bad)
        assert rc != 0 and "gwhip_extend" in text, bad
    rc, text = call(workspace_bytes=L.gwhip_extend_workspace_bytes(2, starts, 16, 1) - 1)
    assert rc != 0 and "workspace" in text
    for missing in ("sequences", "sequence_starts", "scores", "query_ends", "target_ends", "dropped", "result_lengths", "workspace"):
        rc, text = call(**{missing: None})
        assert rc != 0 and "null" in text, missing
    assert call(n_alignments=0)[0] == 0  # an empty batch launches nothing
    assert call(n_alignments=0, results=None, workspace=None)[0] == 0


def test_python_refusals_without_a_device():
    from genomeworks_amd import cudaaligner
    for keyword in ("match", "xdrop"):
        for algorithm in (None, "ukkonen", "affine"):
            with pytest.raises(RuntimeError, match=keyword):
                cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm=algorithm, **{keyword: 3})
    with pytest.raises(RuntimeError, match="gap_open2"):
        cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="extend", gap_open2=24, gap_extend2=1)
    for bad, word in ((dict(band_width=512), "band_width"), (dict(match=64, mismatch=64), "mismatch"), (dict(gap_open=128), "gap_open"),
                      (dict(match=2, gap_extend=127), "gap_extend"), (dict(xdrop=-2), "xdrop"), (dict(match=0), "match")):
        with pytest.raises(RuntimeError, match=word):
            cudaaligner.CudaAlignerBatch(100, 100, 10, algorithm="extend", **bad)
    # today's refusals keep their texts
    with pytest.raises(RuntimeError, match='mismatch: only algorithm="affine" takes these'):
        cudaaligner.CudaAlignerBatch(100, 100, 10, mismatch=3)


def test_extension_args():
    from genomeworks_amd import cudamapper
    f = cudamapper._extension_args
    assert list(f(None)) == [2, 4, 4, 2, 64, 200]
    assert list(f((1, 3, 5, 2, 511, -1))) == [1, 3, 5, 2, 511, -1]
    assert list(f(dict())) == [2, 4, 4, 2, 64, 200]
    assert list(f(dict(band=7, xdrop=0, match=5))) == [5, 4, 4, 2, 7, 0]
    assert list(f((63, 64, 127, 96, 0, 1 << 20))) == [63, 64, 127, 96, 0, 1 << 20]
    for bad in ((2, 4, 4, 2, 512, 200), (2, 4, 4, 2, -1, 200), (64, 64, 4, 2, 64, 200), (0, 4, 4, 2, 64, 200),
                (2, -1, 4, 2, 64, 200), (2, 4, 128, 2, 64, 200), (2, 4, -1, 2, 64, 200), (2, 4, 4, 0, 64, 200),
                (2, 4, 4, 127, 64, 200), (2, 4, 4, 2, 64, -2), (2, 4, 4, 2, 64, (1 << 20) + 1), (2, 4, 4, 2, 64),
                (2, 4, 4, 2, 64, 200, 1), (), dict(bandwidth=64), dict(gap_open2=24), dict(band=512)):
        with pytest.raises(ValueError):
            f(bad)
    for M in (-1, (1 << 19) + 1):  # refused before the library is touched
        with pytest.raises(ValueError, match="max_extension"):
            cudamapper.extend_overlaps([], ["ACGT"], max_extension=M)


def test_the_overlap_rule_on_a_hand_made_case_of_both_strands():
    """ends from oracle_mapper_extend against ends computed by explicit slicing and reverse complementing"""
    import numpy as np

    import mapper_extend_cases as MC
    import oracle_mapper_extend as OM
    r = random.Random(8)
    target = cases.random_sequence(r, 400)
    # the query is target[100:300] between unrelated flanks; the record knows only [140, 260) of it
    flank = lambda n: cases.random_sequence(r, n)
    plus = flank(30) + target[100:300] + flank(25)
    minus = flank(20) + MC.rc(target[100:300]) + flank(35)
    records = np.zeros(2, MC.OVERLAP)
    records[0] = (0, 0, 30 + 40, 140, 30 + 160, 260, ord("+"), 5, 1)
    records[1] = (1, 0, 20 + 40, 140, 20 + 160, 260, ord("-"), 6, 0)
    extension = (2, 4, 4, 2, 16, 30)
    out, moved, scores = OM.extend_overlaps(records, [plus, minus], [target], extension, 1024)
    # '+': the tail is plus[190:] against target[260:], the head plus[:70] against target[:140], both back to front
    tail = O.extend(plus[190:], target[260:], *extension)
    head = O.extend(plus[:70][::-1], target[:140][::-1], *extension)
    # the 40 missing bases, and a base or two of a flank where it happens to match
    assert all(40 <= v <= 42 for v in (tail["query_end"], tail["target_end"], head["query_end"], head["target_end"]))
    assert tuple(out[0])[2:6] == (70 - head["query_end"], 140 - head["target_end"], 190 + tail["query_end"], 260 + tail["target_end"])
    assert list(moved[0]) == [head["query_end"], head["target_end"], tail["query_end"], tail["target_end"]]
    assert list(scores[0]) == [head["score"], tail["score"]] and min(scores[0]) >= 80
    # '-': in the strand's coordinates the target is rc(target) and the slice [400 - 260, 400 - 140)
    strand = MC.rc(target)
    tail = O.extend(minus[180:], strand[260:], *extension)
    head = O.extend(minus[:60][::-1], strand[:140][::-1], *extension)
    assert all(40 <= v <= 42 for v in (tail["query_end"], tail["target_end"], head["query_end"], head["target_end"]))
    # the tail moves te' = 260 up, which is ts = 400 - te' forward; the head moves ts' = 140 down, which is te = 400 - ts'
    assert tuple(out[1])[2:6] == (60 - head["query_end"], 400 - (260 + tail["target_end"]), 180 + tail["query_end"],
                                  400 - (140 - head["target_end"]))
    assert list(moved[1]) == [head["query_end"], head["target_end"], tail["query_end"], tail["target_end"]]
    assert minus[20:220] == MC.rc(target[100:300])  # what the extended record says
    for k in (0, 1):  # every other field is as it was
        assert (out[k]["query_read_id"], out[k]["target_read_id"], out[k]["relative_strand"], out[k]["num_residues"],
                out[k]["overlap_complete"]) == (records[k]["query_read_id"], records[k]["target_read_id"],
                                                records[k]["relative_strand"], records[k]["num_residues"], records[k]["overlap_complete"])
    # a cap below the missing 40 bases, and none at all
    assert list(OM.extend_overlaps(records, [plus, minus], [target], extension, 25)[1][0]) == [25, 25, 25, 25]
    assert list(OM.extend_overlaps(records, [plus, minus], [target], extension, 0)[1][1]) == [0, 0, 0, 0]
