#!/usr/bin/env python3
"""Writes tests/golden/cudamapper_vectors.json: known answers of GenomeWorks' cudamapper tests. Each case names the
reference test it comes from (file:line). Data only.

    python tests/golden/make_mapper_vectors.py [REFERENCE_CHECKOUT]

Minimizer, overlapper and matcher cases are transcribed below by hand. The expected index arrays of the file-based
cases of Test_CudamapperIndexGPU.cu are read from that test file in a GenomeWorks checkout (the argument, or
$GW_REFERENCE), because they run to dozens of values each; their inputs are the small FASTA fixtures in
tests/golden/cudamapper_data/.

Not covered, on purpose:
  * the index case that names ctacaag.fasta (Test_CudamapperIndexCache.cu:565): that file is not in the reference tree;
  * 10_reads.fasta / 20_reads.fasta, aagcta.fasta and catcaag.fasta alone: only the IndexBatcher, IndexCache and
    IndexDescriptor tests read them, and those classes are not part of this library.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "cudamapper_data")


def mini(source, reads, k, w, hash_, reps, rest, first_read_id=0):
    return dict(source=source, reads=reads, k=k, w=w, hash=hash_, first_read_id=first_read_id,
                representations=reps, read_ids=[r[0] for r in rest], positions_in_reads=[r[1] for r in rest],
                directions=[r[2] for r in rest])


MINIMIZERS = [
    mini("Test_CudamapperMinimizer.cpp:94", ["GATT"], 4, 1, False, [0b00001101], [(0, 0, 1)]),
    mini("Test_CudamapperMinimizer.cpp:94", ["GATT"], 4, 1, True, [304626093], [(0, 0, 0)]),
    mini("Test_CudamapperMinimizer.cpp:138", ["GATT"], 2, 3, False, [0b1000, 0b0011, 0b0000],
         [(0, 0, 0), (0, 1, 0), (0, 2, 1)]),
    mini("Test_CudamapperMinimizer.cpp:138", ["GATT"], 2, 3, True, [1023180699, 2797583197, 3255840626],
         [(0, 0, 0), (0, 1, 0), (0, 2, 0)]),
    mini("Test_CudamapperMinimizer.cpp:207", ["CCCATACC"], 2, 7, False, [0b0101, 0b0101, 0b0100, 0b0011, 0b0001, 0b0101],
         [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 5, 0), (0, 6, 0)]),
    mini("Test_CudamapperMinimizer.cpp:207", ["CCCATACC"], 2, 7, True, [2515151312, 2515151312, 1582582417, 2515151312],
         [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 6, 0)]),
    mini("Test_CudamapperMinimizer.cpp:298", ["CATCAAG", "AAGCTA"], 3, 2, False,
         [0b001110, 0b001101, 0b010000, 0b000010, 0b000010, 0b001001, 0b011100],
         [(0, 0, 1), (0, 1, 0), (0, 3, 0), (0, 4, 0), (1, 0, 0), (1, 2, 1), (1, 3, 0)]),
    mini("Test_CudamapperMinimizer.cpp:298", ["CATCAAG", "AAGCTA"], 3, 2, True,
         [549100223, 447855090, 1279515286, 1865025060, 1865025060, 4103259927, 357458314],
         [(0, 0, 0), (0, 1, 1), (0, 2, 0), (0, 4, 0), (1, 0, 0), (1, 2, 1), (1, 3, 0)]),
    # the same two reads numbered from read id 5
    mini("Test_CudamapperMinimizer.cpp:409", ["CATCAAG", "AAGCTA"], 3, 2, False,
         [0b001110, 0b001101, 0b010000, 0b000010, 0b000010, 0b001001, 0b011100],
         [(5, 0, 1), (5, 1, 0), (5, 3, 0), (5, 4, 0), (6, 0, 0), (6, 2, 1), (6, 3, 0)], first_read_id=5),
    mini("Test_CudamapperMinimizer.cpp:409", ["CATCAAG", "AAGCTA"], 3, 2, True,
         [549100223, 447855090, 1279515286, 1865025060, 1865025060, 4103259927, 357458314],
         [(5, 0, 0), (5, 1, 1), (5, 2, 0), (5, 4, 0), (6, 0, 0), (6, 2, 1), (6, 3, 0)], first_read_id=5),
]

# get_overlaps defaults of overlapper_triggered.hpp:57-63: min_residues 20, min_overlap_len 50, min_bases_per_residue 50,
# min_overlap_fraction 0.9
_DEFAULTS = dict(min_residues=20, min_overlap_len=50, min_bases_per_residue=50, min_overlap_fraction=0.9)


def ov(source, anchors, expected, **args):
    case = dict(_DEFAULTS, all_to_all=False, source=source, anchors=anchors, expected=expected)
    case.update(args)
    return case


OVERLAPPER = [
    # one anchor (fields left zero): no chain of three
    ov("Test_CudamapperOverlapperTriggered.cu:30", [(0, 0, 0, 0)], [], min_residues=0),
    ov("Test_CudamapperOverlapperTriggered.cu:57",
       [(1, 2, 100, 1000), (1, 2, 200, 1100), (1, 2, 300, 1200), (1, 2, 400, 1300)],
       [dict(query_read_id=1, target_read_id=2, query_start_position_in_read=100, query_end_position_in_read=400,
             target_start_position_in_read=1000, target_end_position_in_read=1300)],
       min_residues=0, min_overlap_len=0, min_bases_per_residue=1000),
    # four different read pairs
    ov("Test_CudamapperOverlapperTriggered.cu:110",
       [(1, 2, 100, 1000), (3, 4, 200, 1100), (5, 6, 300, 1200), (8, 9, 400, 1300)], [],
       min_residues=0, min_overlap_len=0, min_bases_per_residue=1000),
    # colinear, but 1 900 bases apart: four chains of one anchor under the header defaults
    ov("Test_CudamapperOverlapperTriggered.cu:157",
       [(1, 2, 100, 1000), (1, 2, 2000, 11000), (1, 2, 3000, 12000), (1, 2, 4000, 13000)], [], min_residues=0),
    ov("Test_CudamapperOverlapperTriggered.cu:204",
       [(1, 2, 100, 1000), (1, 2, 200, 1100), (1, 2, 300, 1200), (1, 2, 2400, 3300)],
       [dict(query_read_id=1, target_read_id=2, query_start_position_in_read=100, query_end_position_in_read=300,
             target_start_position_in_read=1000, target_end_position_in_read=1200)],
       min_residues=0, min_overlap_len=0, min_bases_per_residue=1000),
    ov("Test_CudamapperOverlapperTriggered.cu:257",
       [(1, 2, 100, 1300), (1, 2, 200, 1200), (1, 2, 300, 1100), (1, 2, 400, 1000)],
       [dict(relative_strand="-", target_start_position_in_read=1000, target_end_position_in_read=1300)],
       min_residues=0, min_overlap_len=0, min_bases_per_residue=1000),
]


def _sorted_anchors(a):
    return sorted(a)


def matcher_32bit():
    """Test_CudamapperMatcherGPU.cu:297: five query and seven target representations; query section i pairs with
    target section found[i]."""
    q_first = [0, 4, 10, 13, 18, 21]
    t_first = [0, 3, 7, 9, 13, 16, 18, 21]
    found = [-1, 1, 3, -1, 6]
    q_rid = [500 + i for i in range(21)]
    q_pos = [10 * i for i in range(21)]
    t_rid = [10000 + 100 * i for i in range(21)]
    t_pos = [1000 * i for i in range(21)]
    meta = dict(query_first_read_id=500, query_number_of_reads=20, query_longest=200,
                target_first_read_id=10000, target_number_of_reads=2000, target_longest=20000)
    return q_first, t_first, found, q_rid, q_pos, t_rid, t_pos, meta


def matcher_64bit(src):
    """Test_CudamapperMatcherGPU.cu:426: the same sections, explicit read ids and positions (target positions above
    2^31)."""
    lines = src.split("\n")
    start = next(i for i, l in enumerate(lines) if "test_generate_anchors_small_example_64_bit_positions" in l)
    body = "\n".join(lines[start:start + 215])

    def arr(name):
        return [int(v) for v in re.findall(name + r"\.push_back\((-?\d+)\)", body)]

    q_first = arr("query_starting_index_of_each_representation_h")
    t_first = arr("target_starting_index_of_each_representation_h")
    found = arr("found_target_indices_h")
    meta = dict(query_first_read_id=1000, query_number_of_reads=8000 - 1000, query_longest=100900,
                target_first_read_id=7001, target_number_of_reads=7009 - 7001, target_longest=2540000090)
    return (q_first, t_first, found, arr("query_read_ids_h"), arr("query_positions_in_read_h"), arr("target_read_ids_h"),
            arr("target_positions_in_read_h"), meta)


def matcher_case(source, parts):
    q_first, t_first, found, q_rid, q_pos, t_rid, t_pos, meta = parts
    # representations that reproduce the pairing: target section j holds 10 (j + 1); an unpaired query section gets a
    # value between its neighbours that no target section has
    t_unique = [10 * (j + 1) for j in range(len(t_first) - 1)]
    q_unique = []
    for i, j in enumerate(found):
        q_unique.append(10 * (j + 1) if j >= 0 else (q_unique[-1] + 1 if q_unique else 1))
    assert q_unique == sorted(q_unique) and all((v in t_unique) == (j >= 0) for v, j in zip(q_unique, found))
    expected = []
    for i, j in enumerate(found):
        if j < 0:
            continue
        for qi in range(q_first[i], q_first[i + 1]):
            for ti in range(t_first[j], t_first[j + 1]):
                expected.append((q_rid[qi], t_rid[ti], q_pos[qi], t_pos[ti]))
    return dict(source=source, query_unique_representations=q_unique, query_first_occurrence=q_first,
                query_read_ids=q_rid, query_positions_in_reads=q_pos, target_unique_representations=t_unique,
                target_first_occurrence=t_first, target_read_ids=t_rid, target_positions_in_reads=t_pos,
                expected_anchors=_sorted_anchors(expected), **meta)


def read_fasta(name):
    seqs = []
    with open(os.path.join(DATA, name)) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                seqs.append("")
            elif line:
                seqs[-1] += line
    return seqs


def index_cases(src):
    """The file-based cases of Test_CudamapperIndexGPU.cu (test_function(filename, first, past, ...), hash off)."""
    lines = src.split("\n")
    out = []
    for s, l in enumerate(lines):
        if not l.startswith("TEST("):
            continue
        body = "\n".join(lines[s:])
        body = body[:body.index("\n}\n")]
        if "test_function(filename" not in body:
            continue
        body_nc = re.sub(r"//[^\n]*", "", body)

        def arr(name):
            return [int(v, 0) for v in re.findall(r"\b" + name + r"\.push_back\((0b[01]+|\d+)\)", body_nc)]

        def const(name):
            return int(re.search(name + r"\s*=\s*(\d+)", body_nc).group(1))

        call = re.search(r"test_function\(filename,\s*(\d+)\s*,\s*(\d+)\s*,", body_nc)
        fp = re.search(r"filtering_parameter\s*=\s*([0-9.e-]+);", body_nc)
        dirs = re.findall(r"expected_directions_of_reads\.push_back\(SketchElement::DirectionOfRepresentation::(\w+)\)",
                          body_nc)
        out.append(dict(
            source="Test_CudamapperIndexGPU.cu:%d" % (s + 1),
            fasta=re.search(r'"/(\w+\.fasta)"', body_nc).group(1),
            first_read_id=int(call.group(1)), past_the_last_read_id=int(call.group(2)),
            k=const("minimizer_size"), w=const("window_size"),
            filtering_parameter=float(fp.group(1)) if fp else 1.0,
            representations=arr("expected_representations"),
            positions_in_reads=arr("expected_positions_in_reads"),
            read_ids=arr("expected_read_ids"),
            directions_of_reads=[0 if d == "FORWARD" else 1 for d in dirs],
            unique_representations=arr("expected_unique_representations"),
            first_occurrence_of_representations=arr("expected_first_occurrence_of_representations"),
            number_of_reads=const("expected_number_of_reads"),
            smallest_read_id=const("expected_smallest_read_id"),
            largest_read_id=const("expected_largest_read_id"),
            number_of_basepairs_in_longest_read=const("expected_number_of_basepairs_in_longest_read")))
        case = out[-1]
        case["reads"] = read_fasta(case["fasta"])[case["first_read_id"]:case["past_the_last_read_id"]]
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GW_REFERENCE")
    if not ref:
        sys.exit("usage: make_mapper_vectors.py GENOMEWORKS_CHECKOUT")
    tests = os.path.join(ref, "cudamapper", "tests")
    with open(os.path.join(tests, "Test_CudamapperIndexGPU.cu")) as f:
        indices = index_cases(f.read())
    with open(os.path.join(tests, "Test_CudamapperMatcherGPU.cu")) as f:
        msrc = f.read()
    matchers = [matcher_case("Test_CudamapperMatcherGPU.cu:297", matcher_32bit()),
                matcher_case("Test_CudamapperMatcherGPU.cu:426", matcher_64bit(msrc))]
    # whole indices of gatt.fasta (k=4 w=1): one anchor against itself, none against an empty index (k=5 > read)
    matcher_files = [dict(source="Test_CudamapperMatcherGPU.cu:638", fasta="gatt.fasta", query_k=4, target_k=4, w=1,
                          expected_count=1),
                     dict(source="Test_CudamapperMatcherGPU.cu:653", fasta="gatt.fasta", query_k=4, target_k=5, w=1,
                          expected_count=0),
                     dict(source="Test_CudamapperMatcherGPU.cu:653", fasta="gatt.fasta", query_k=5, target_k=4, w=1,
                          expected_count=0),
                     dict(source="Test_CudamapperMatcherGPU.cu:653", fasta="gatt.fasta", query_k=5, target_k=5, w=1,
                          expected_count=0)]
    for m in matcher_files:
        m["reads"] = read_fasta(m["fasta"])
    doc = dict(minimizers=MINIMIZERS, indices=indices, matcher=matchers, matcher_files=matcher_files,
               overlapper=OVERLAPPER,
               skipped=[dict(source="Test_CudamapperIndexCache.cu:565",
                             reason="names ctacaag.fasta, which is not in the reference tree")])
    with open(os.path.join(HERE, "cudamapper_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d minimizer, %d index, %d matcher, %d overlapper cases" %
          (len(MINIMIZERS), len(indices), len(matchers) + len(matcher_files), len(OVERLAPPER)))


if __name__ == "__main__":
    main()
