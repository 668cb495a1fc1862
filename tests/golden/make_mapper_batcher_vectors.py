#!/usr/bin/env python3
"""Writes tests/golden/cudamapper_batcher_vectors.json: the expected batches of GenomeWorks' index batcher tests
(cudamapper/tests/Test_CudamapperIndexBatcher.cu): the table for a query and a target set that differ, the table for one
set against itself, and the cases that must be refused. Data only, transcribed from the cited lines.

    python tests/golden/make_mapper_batcher_vectors.py

Where the reference is present (GW_REFERENCE, default /root/reference) every descriptor list of its test source is read
again and compared with the tables below, and the read lengths with its two data files, so a transcription slip fails
loudly. A host batch is (query indices, target indices, [device batches]), a device batch (query indices, target
indices), an index [first_read, number_of_reads]."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GW_REFERENCE", "/root/reference")
SOURCE = "Test_CudamapperIndexBatcher.cu"

# read lengths of the reference's 10_reads.fasta and 20_reads.fasta (SOURCE:124-164)
LENGTHS_10 = [5, 2, 2, 2, 2, 3, 7, 2, 8, 3]
LENGTHS_20 = [4, 6, 7, 4, 3, 8, 6, 3, 3, 5, 7, 3, 2, 4, 4, 2, 5, 6, 2, 4]

# SOURCE:122-533: 10_reads against 20_reads, 10 basepairs per index, Q 2, q 1, C 5, c 2
NOT_THE_SAME = [
    ([[0, 3], [3, 3]], [[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]],
     [([[0, 3]], [[0, 2], [2, 1]]),
      ([[0, 3]], [[3, 2], [5, 1]]),
      ([[0, 3]], [[6, 2]]),
      ([[3, 3]], [[0, 2], [2, 1]]),
      ([[3, 3]], [[3, 2], [5, 1]]),
      ([[3, 3]], [[6, 2]])]),
    ([[0, 3], [3, 3]], [[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]],
     [([[0, 3]], [[8, 2], [10, 2]]),
      ([[0, 3]], [[12, 3], [15, 2]]),
      ([[0, 3]], [[17, 2]]),
      ([[3, 3]], [[8, 2], [10, 2]]),
      ([[3, 3]], [[12, 3], [15, 2]]),
      ([[3, 3]], [[17, 2]])]),
    ([[0, 3], [3, 3]], [[19, 1]],
     [([[0, 3]], [[19, 1]]),
      ([[3, 3]], [[19, 1]])]),
    ([[6, 2], [8, 1]], [[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]],
     [([[6, 2]], [[0, 2], [2, 1]]),
      ([[6, 2]], [[3, 2], [5, 1]]),
      ([[6, 2]], [[6, 2]]),
      ([[8, 1]], [[0, 2], [2, 1]]),
      ([[8, 1]], [[3, 2], [5, 1]]),
      ([[8, 1]], [[6, 2]])]),
    ([[6, 2], [8, 1]], [[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]],
     [([[6, 2]], [[8, 2], [10, 2]]),
      ([[6, 2]], [[12, 3], [15, 2]]),
      ([[6, 2]], [[17, 2]]),
      ([[8, 1]], [[8, 2], [10, 2]]),
      ([[8, 1]], [[12, 3], [15, 2]]),
      ([[8, 1]], [[17, 2]])]),
    ([[6, 2], [8, 1]], [[19, 1]],
     [([[6, 2]], [[19, 1]]),
      ([[8, 1]], [[19, 1]])]),
    ([[9, 1]], [[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]],
     [([[9, 1]], [[0, 2], [2, 1]]),
      ([[9, 1]], [[3, 2], [5, 1]]),
      ([[9, 1]], [[6, 2]])]),
    ([[9, 1]], [[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]],
     [([[9, 1]], [[8, 2], [10, 2]]),
      ([[9, 1]], [[12, 3], [15, 2]]),
      ([[9, 1]], [[17, 2]])]),
    ([[9, 1]], [[19, 1]],
     [([[9, 1]], [[19, 1]])]),
]

# SOURCE:535-854: 20_reads against itself, 10 basepairs per index, Q = C = 5, q = c = 2
THE_SAME = [
    ([[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]], [[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]],
     [([[0, 2], [2, 1]], [[0, 2], [2, 1]]),
      ([[0, 2], [2, 1]], [[3, 2], [5, 1]]),
      ([[0, 2], [2, 1]], [[6, 2]]),
      ([[3, 2], [5, 1]], [[3, 2], [5, 1]]),
      ([[3, 2], [5, 1]], [[6, 2]]),
      ([[6, 2]], [[6, 2]])]),
    ([[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]], [[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]],
     [([[0, 2], [2, 1]], [[8, 2], [10, 2]]),
      ([[0, 2], [2, 1]], [[12, 3], [15, 2]]),
      ([[0, 2], [2, 1]], [[17, 2]]),
      ([[3, 2], [5, 1]], [[8, 2], [10, 2]]),
      ([[3, 2], [5, 1]], [[12, 3], [15, 2]]),
      ([[3, 2], [5, 1]], [[17, 2]]),
      ([[6, 2]], [[8, 2], [10, 2]]),
      ([[6, 2]], [[12, 3], [15, 2]]),
      ([[6, 2]], [[17, 2]])]),
    ([[0, 2], [2, 1], [3, 2], [5, 1], [6, 2]], [[19, 1]],
     [([[0, 2], [2, 1]], [[19, 1]]),
      ([[3, 2], [5, 1]], [[19, 1]]),
      ([[6, 2]], [[19, 1]])]),
    ([[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]], [[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]],
     [([[8, 2], [10, 2]], [[8, 2], [10, 2]]),
      ([[8, 2], [10, 2]], [[12, 3], [15, 2]]),
      ([[8, 2], [10, 2]], [[17, 2]]),
      ([[12, 3], [15, 2]], [[12, 3], [15, 2]]),
      ([[12, 3], [15, 2]], [[17, 2]]),
      ([[17, 2]], [[17, 2]])]),
    ([[8, 2], [10, 2], [12, 3], [15, 2], [17, 2]], [[19, 1]],
     [([[8, 2], [10, 2]], [[19, 1]]),
      ([[12, 3], [15, 2]], [[19, 1]]),
      ([[17, 2]], [[19, 1]])]),
    ([[19, 1]], [[19, 1]],
     [([[19, 1]], [[19, 1]])]),
]

CASES = [
    dict(source=SOURCE + ":122", name="query_and_target_not_the_same", query_lengths=LENGTHS_10,
         target_lengths=LENGTHS_20, same_query_and_target=False, query_basepairs_per_index=10,
         target_basepairs_per_index=10, query_indices_per_host_batch=2, query_indices_per_device_batch=1,
         target_indices_per_host_batch=5, target_indices_per_device_batch=2, expected=NOT_THE_SAME),
    dict(source=SOURCE + ":535", name="same_query_and_target", query_lengths=LENGTHS_20, target_lengths=None,
         same_query_and_target=True, query_basepairs_per_index=10, target_basepairs_per_index=10,
         query_indices_per_host_batch=5, query_indices_per_device_batch=2, target_indices_per_host_batch=5,
         target_indices_per_device_batch=2, expected=THE_SAME),
]

# SOURCE:856-925: 10_reads against itself with Q 5, q 2 and 10 basepairs per index; one argument differs per case.
# "parser" (the same set announced, two parsers given) cannot be said through an interface that names the same set by
# leaving the target out; it is kept for the record and marked so.
_BASE = dict(query_lengths=LENGTHS_10, query_basepairs_per_index=10, target_basepairs_per_index=10,
             query_indices_per_host_batch=5, query_indices_per_device_batch=2, target_indices_per_host_batch=5,
             target_indices_per_device_batch=2, expressible=True)
EXCEPTIONS = [
    dict(_BASE, source=SOURCE + ":872", name="indices_per_host_batch", target_indices_per_host_batch=100),
    dict(_BASE, source=SOURCE + ":886", name="indices_per_device_batch", target_indices_per_device_batch=100),
    dict(_BASE, source=SOURCE + ":900", name="parser", expressible=False),
    dict(_BASE, source=SOURCE + ":914", name="basepairs_per_index", target_basepairs_per_index=100),
]


def tables_of_the_reference(text):
    """every descriptor list of the source, gathered per TEST in the shape of the tables above"""
    tables = {}
    for test in re.split(r"\nTEST\(", text)[1:]:
        name = re.match(r"TestCudamapperIndexBatcher, test_generate_batches_of_indices_(\w+)\)", test).group(1)
        out = []
        for level, kind, literal in re.findall(r"(host|device)_batch_(query|target)_indices(\{.*\});", test):
            d = [[int(a), int(b)] for a, b in re.findall(r"\{(\d+), (\d+)\}", literal)]
            if level == "host" and kind == "query":
                out.append([d, None, []])
            elif level == "host":
                out[-1][1] = d
            elif kind == "query":
                out[-1][2].append([d, None])
            else:
                out[-1][2][-1][1] = d
        tables[name] = out
    return tables


def fasta_lengths(path):
    lengths = []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                lengths.append(0)
            else:
                lengths[-1] += len(line.strip())
    return lengths


def check_against_reference():
    path = os.path.join(REF, "cudamapper", "tests", SOURCE)
    if not os.path.exists(path):
        print("reference not present: the tables are written unchecked")
        return
    with open(path) as f:
        text = f.read()
    tables = tables_of_the_reference(text)
    as_lists = lambda t: json.loads(json.dumps(t))
    for case in CASES:
        if as_lists(case["expected"]) != tables[case["name"]]:
            sys.exit("the table %s differs from %s" % (case["name"], path))
    for name, lengths in (("10_reads.fasta", LENGTHS_10), ("20_reads.fasta", LENGTHS_20)):
        if fasta_lengths(os.path.join(REF, "cudamapper", "data", name)) != lengths:
            sys.exit("read lengths of %s differ" % name)
    if len(re.findall(r"ASSERT_THROW\(generate_batches_of_indices", text)) != len(EXCEPTIONS):
        sys.exit("the number of exception cases differs from %s" % path)
    for literal in ("target_indices_per_host_batch = 100;", "target_indices_per_device_batch = 100;",
                    "target_basepairs_per_index = 100;"):
        if literal not in text:
            sys.exit("literal %r not found in %s" % (literal, path))
    print("checked against", path)


if __name__ == "__main__":
    check_against_reference()
    out = os.path.join(HERE, "cudamapper_batcher_vectors.json")
    with open(out, "w") as f:
        json.dump(dict(cases=CASES, exceptions=EXCEPTIONS), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")
