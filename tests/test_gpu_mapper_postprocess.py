"""cudamapper's overlap post-processing on the GPU (fusion, end rescue, grouping into indices, the batched driver and
the cudamapper tool) against the reference-recorded fixtures and the CPU oracle (tests/oracle_mapper_postprocess.py),
record for record."""
import os
import subprocess

import numpy as np
import pytest

import mapper_cases as MC
import mapper_postprocess_cases as PC
import oracle_mapper as O
import oracle_mapper_postprocess as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "genomeworks_amd", "bin", "cudamapper")


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


@pytest.fixture(scope="module")
def golden():
    return PC.load_reference()


def same(a, b):
    return a.dtype == O.OVERLAP and np.array_equal(a, np.ascontiguousarray(b, O.OVERLAP))


# ---- fixtures ------------------------------------------------------------------------------------------------------

def test_post_process_vectors(cm):
    for case in PC.load_vectors()["post_process"]:
        o = PC.overlaps_from_dicts(case["overlaps"])
        out = cm.post_process_overlaps(o)
        assert len(out) == case["expected_count"], case["source"]
        assert same(out, P.post_process_overlaps(o)), case["source"]


def test_extension_vector(cm):
    """one round of the reference's test moves both ends; three rounds equal the oracle's"""
    for case in PC.load_vectors()["extension"]:
        o = PC.overlaps_from_dicts([case["overlap"]])
        q, t = [case["query"]], [case["target"]]
        got = cm.rescue_overlap_ends(o, q, t, case["extension"], case["required_similarity"])
        assert same(got, P.rescue_overlap_ends(o, q, t, case["extension"], case["required_similarity"]))
        e = case["expected"]  # already at the ends of both reads after the first round
        assert all(int(got[0][k]) == v for k, v in e.items()), case["source"]


def test_grouping_vectors(cm):
    for case in PC.load_vectors()["grouping"]:
        lengths = [len(s) for s in PC.fasta_reads(case["fasta"])]
        assert [list(d) for d in cm.group_reads_into_indices(lengths, case["max_basepairs_per_index"])] == \
            case["expected"], case["source"]
    rng = np.random.default_rng(3)
    for lengths, limit in ([], 10), ([11, 3], 10), ([10, 1], 10), ([4, 6, 20, 1], 10), \
            (rng.integers(1, 3000, 500).tolist(), 5000):
        assert cm.group_reads_into_indices(lengths, limit) == P.group_reads_into_indices(lengths, limit)


@pytest.mark.parametrize("case", PC.CASES)
def test_post_process_equals_reference(cm, golden, case):
    o = golden[case + "_overlaps"]
    assert same(cm.post_process_overlaps(o), golden[case + "_post"])
    assert same(cm.post_process_overlaps(o, True), golden[case + "_post_drop"])


@pytest.mark.parametrize("case", PC.RESCUE_CASES)
def test_rescue_equals_reference(cm, golden, case):
    q, t = PC.reads_of(golden, case)
    assert same(cm.rescue_overlap_ends(golden[case + "_overlaps"], q, t, 50, 0.5), golden[case + "_rescue"])
    assert same(cm.rescue_overlap_ends(golden[case + "_post"], q, t, 50, 0.5), golden[case + "_post_rescue"])


# ---- seeded random sweep -------------------------------------------------------------------------------------------

def random_fusion_overlaps(seed, n):
    """overlaps on few read pairs whose neighbours' gaps straddle every threshold of the fusion rules"""
    rng = np.random.default_rng(seed)
    o = np.zeros(n, O.OVERLAP)
    q = t = 0
    qe = te = 0
    strand = ord("+")
    for i in range(n):
        if i == 0 or rng.random() < 0.12:
            q, t = int(rng.integers(0, 6)), int(rng.integers(0, 6))
            strand = int(rng.choice([ord("+"), ord("-")]))
            qe, te = int(rng.integers(0, 5000)), int(rng.integers(3000000, 4000000))
        if rng.random() < 0.05:
            strand = int(rng.choice([ord("+"), ord("-")]))
        lq, lt = (int(x) for x in rng.integers(50, 6000, 2))
        gq = int(rng.choice([0, 1, 499, 500, 501, 800, 1000, 1001, 1250, 5000, -100]) + rng.integers(-2, 3))
        gt = int(rng.choice([0, 1, 499, 500, 501, 800, 1000, 1001, 1250, 5000, -100]) + rng.integers(-2, 3))
        qs = max(0, qe + gq)
        if strand == ord("+"):
            ts = max(0, te + gt)
            rec = (q, t, qs, ts, qs + lq, ts + lt, strand, int(rng.integers(1, 200)), int(rng.integers(0, 2)))
            te = ts + lt
        else:  # targets fall: te holds the previous target start
            t_end = max(lt, te - gt)
            rec = (q, t, qs, t_end - lt, qs + lq, t_end, strand, int(rng.integers(1, 200)), int(rng.integers(0, 2)))
            te = t_end - lt
        qe = qs + lq
        o[i] = rec
    return o


@pytest.mark.parametrize("seed,n", [(1, 3000), (2, 1), (3, 2), (4, 257), (5, 4096)])
def test_post_process_random_sweep(cm, seed, n):
    o = random_fusion_overlaps(seed, n)
    flags = P.mergable_flags(o)
    if n >= 257:
        assert 0.1 < flags.mean() < 0.9  # the sweep fuses and splits
    for drop in (False, True):
        assert same(cm.post_process_overlaps(o, drop), P.post_process_overlaps(o, drop)), (seed, drop)


def shrunk_overlaps(seed, reads, overlaps):
    """mapped overlaps with their ends pulled in by 0..120 bases, so that the flanks are similar sequence"""
    rng = np.random.default_rng(seed)
    o = overlaps.copy()
    for r in o:
        for s, e in (("query_start_position_in_read", "query_end_position_in_read"),
                     ("target_start_position_in_read", "target_end_position_in_read")):
            a, b = int(r[s]), int(r[e])
            da, db = (int(x) for x in rng.integers(0, 121, 2))
            if b - a > da + db:
                r[s], r[e] = a + da, b - db
    return o


@pytest.fixture(scope="module")
def sweep_set():
    reads = [r.encode() for r in MC.synthetic_reads(17, 40000, 12, 2500, 0.03)]
    # reads with N and with lower case: ordinary bytes for the k-mers, unchanged by the complement
    reads[3] = reads[3][:700] + b"N" * 3 + reads[3][703:]
    reads[5] = reads[5][:900].lower() + reads[5][900:]
    o = O.map_reads(reads, None, 15, 10, 1.0, **MC.OVERLAP_PARAMS)
    assert len(o) >= 2000, len(o)
    return reads, shrunk_overlaps(18, reads, o)


@pytest.mark.parametrize("extension,similarity", [(0, 0.5), (15, 0.5), (50, 0.5), (78, 0.5), (50, 0.3), (78, 1.0),
                                                  (30, 0.0), (14, 0.9)])
def test_rescue_random_sweep(cm, sweep_set, extension, similarity):
    reads, o = sweep_set
    ref = P.rescue_overlap_ends(o, reads, reads, extension, similarity)
    if 0 < extension and similarity <= 0.5:
        assert not np.array_equal(ref, o)
    assert same(cm.rescue_overlap_ends(o, reads, None, extension, similarity), ref)
    assert same(cm.rescue_overlap_ends(o, reads, reads, extension, similarity), ref)


def test_rescue_with_first_read_ids(cm, sweep_set):
    reads, o = sweep_set
    shifted = o[:300].copy()
    shifted["query_read_id"] += 1000
    shifted["target_read_id"] += 70
    ref = P.rescue_overlap_ends(shifted, reads, reads, 50, 0.5, 1000, 70)
    got = cm.rescue_overlap_ends(shifted, reads, reads, 50, 0.5, first_query_read_id=1000, first_target_read_id=70)
    assert same(got, ref)


def test_empty_input(cm):
    empty = np.zeros(0, O.OVERLAP)
    assert len(cm.post_process_overlaps(empty)) == 0 and len(cm.post_process_overlaps(empty, True)) == 0
    assert len(cm.rescue_overlap_ends(empty, ["ACGT"], None)) == 0
    assert len(cm.rescue_overlap_ends(empty, [], [])) == 0
    assert cm.group_reads_into_indices([], 100) == [(0, 0)]
    assert len(cm.map_reads_batched([], max_basepairs_per_index=100)) == 0
    assert len(cm.map_reads_batched(["ACGT"], max_basepairs_per_index=100)) == 0


def test_rescue_errors(cm):
    reads = ["ACGT" * 30, "ACGT" * 20]
    ok = PC.overlaps_from_dicts([dict(query_read_id=0, target_read_id=1, query_start_position_in_read=10,
                                      query_end_position_in_read=60, target_start_position_in_read=10,
                                      target_end_position_in_read=60, relative_strand="+")] * 3)
    assert same(cm.rescue_overlap_ends(ok, reads), P.rescue_overlap_ends(ok, reads, reads))
    for extension in (-1, 79, 1000):
        with pytest.raises(cm.MapperError):
            cm.rescue_overlap_ends(ok, reads, None, extension)
        with pytest.raises(cm.MapperError):
            cm.rescue_overlap_ends(ok[:0], reads, None, extension)
    for strand in "+-":
        for field, value in (("target_end_position_in_read", 81), ("query_end_position_in_read", 121),
                             ("target_read_id", 2), ("query_read_id", 7), ("query_start_position_in_read", 200),
                             ("target_start_position_in_read", 4000000000)):
            bad = ok.copy()
            bad["relative_strand"] = ord(strand)
            bad[1][field] = value
            with pytest.raises(ValueError):
                P.rescue_overlap_ends(bad, reads, reads)
            with pytest.raises(cm.MapperError):
                cm.rescue_overlap_ends(bad, reads)
    with pytest.raises(cm.MapperError):  # ids below the first read id of the set
        cm.rescue_overlap_ends(ok, reads, None, first_query_read_id=1)


# ---- the batched driver and the tool -------------------------------------------------------------------------------

LIMIT = 45000


@pytest.fixture(scope="module")
def batch_reads():
    reads = MC.synthetic_reads(23, 20000, 7, 2000, 0.03)
    groups = P.group_reads_into_indices([len(r) for r in reads], LIMIT)
    assert len(groups) >= 3
    return reads


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("rescue", [False, True])
def test_map_reads_batched_all_to_all(cm, batch_reads, rescue, drop):
    timings = {}
    got = cm.map_reads_batched(batch_reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT,
                               drop_fused_overlaps=drop, rescue_overlap_ends=rescue, timings=timings)
    ref = P.map_batched(batch_reads, None, 15, 10, 1.0, MC.OVERLAP_PARAMS, LIMIT, drop_fused_overlaps=drop,
                        rescue=rescue)
    assert len(ref) > 100 and timings["index_pairs"] >= 6
    assert same(got, ref)


def test_map_reads_batched_query_vs_target(cm, batch_reads):
    half = len(batch_reads) // 2
    q, t = batch_reads[:half], batch_reads[half:]
    got = cm.map_reads_batched(q, t, filtering_parameter=1.0, max_basepairs_per_index=LIMIT,
                               max_basepairs_per_target_index=30000, rescue_overlap_ends=True)
    ref = P.map_batched(q, t, 15, 10, 1.0, MC.OVERLAP_PARAMS, LIMIT, 30000, rescue=True)
    assert len(ref) > 50
    assert same(got, ref)


def test_map_reads_batched_one_index_equals_map_reads(cm, batch_reads):
    got = cm.map_reads_batched(batch_reads, filtering_parameter=1.0, max_basepairs_per_index=10**9, post_process=False)
    assert same(got, cm.map_reads(batch_reads, filtering_parameter=1.0))
    half = len(batch_reads) // 2
    got = cm.map_reads_batched(batch_reads[:half], batch_reads[half:], max_basepairs_per_index=10**9, post_process=False)
    assert same(got, cm.map_reads(batch_reads[:half], batch_reads[half:]))


def run_tool(args):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags", [[], ["-R"], ["-D", "-R"]])
def test_cudamapper_tool_prints_format_paf(cm, batch_reads, tmp_path, flags):
    names = ["read_%d" % i for i in range(len(batch_reads))]
    fasta = tmp_path / "reads.fasta"
    with open(fasta, "w") as f:
        for n, r in zip(names, batch_reads):
            f.write(">%s some description\n" % n)
            f.write("\n".join(r[i:i + 80] for i in range(0, len(r), 80)) + "\n")
    run = run_tool(["-i", str(LIMIT / 1e6)] + flags + [str(fasta), str(fasta)])
    assert run.returncode == 0, run.stderr
    # less than 0.5 Mbp of input and no -F: the tool turns the frequency filter off, as the reference does
    o = cm.map_reads_batched(batch_reads, filtering_parameter=1.0, max_basepairs_per_index=LIMIT,
                             drop_fused_overlaps="-D" in flags, rescue_overlap_ends="-R" in flags)
    lengths = [len(r) for r in batch_reads]
    assert len(o) > 100
    assert run.stdout == cm.format_paf(o, names, lengths, names, lengths, 15)
    assert run.stdout == P.format_paf(o, names, lengths, names, lengths, 15)


def test_cudamapper_tool_refuses_what_it_does_not_do(tmp_path):
    fasta = tmp_path / "reads.fasta"
    fasta.write_text(">a\nACGT\n")
    for args in (["-a", "1"], ["-d", "2"], ["-S"], ["-Q", "3"], ["-m", "4"]):
        run = run_tool(args + [str(fasta), str(fasta)])
        assert run.returncode != 0 and run.stdout == "" and "cudamapper:" in run.stderr, (args, run.stderr)
    assert "align_overlaps" in run_tool(["-a", "1", str(fasta), str(fasta)]).stderr
    import gzip
    packed = tmp_path / "reads.fasta.gz"
    with gzip.open(packed, "wt") as f:
        f.write(">a\nACGT\n")
    run = run_tool([str(packed), str(packed)])
    assert run.returncode != 0 and run.stdout == "" and "gzip" in run.stderr


def test_cudamapper_tool_warns_about_short_reads(batch_reads, tmp_path):
    fasta = tmp_path / "reads.fasta"
    with open(fasta, "w") as f:
        for i, r in enumerate(batch_reads[:6] + ["ACGTACGT"]):
            f.write(">r%d\n%s\n" % (i, r))
    run = run_tool([str(fasta), str(fasta)])
    assert run.returncode == 0, run.stderr
    assert [line for line in run.stderr.splitlines() if line.startswith("WARNING")] == [
        "WARNING: 1 reads are shorter than k + w - 1 = 24 bases; they are skipped and the read ids behind them in "
        "their index shift"]
