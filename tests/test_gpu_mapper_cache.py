"""cudamapper's index cache on the GPU: packed host copies of indices (Index.to_host / IndexHostCopy.to_device and the
kernel-level gwm_index_pack / gwm_index_unpack), the index batcher against the reference's expected batches, the cached
batched driver against the one-pair-at-a-time run and the walk of tests/oracle_mapper_batcher.py, and the tool's
-Q -q -C -c."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import mapper_cases as MC
import oracle_mapper_batcher as B
import oracle_mapper_postprocess as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOL = os.path.join(ROOT, "genomeworks_amd", "bin", "cudamapper")
ARRAYS = ("representations", "read_ids", "positions_in_reads", "directions_of_reads", "unique_representations",
          "first_occurrence_of_representations")
ATTRIBUTES = ("number_of_reads", "smallest_read_id", "largest_read_id", "number_of_basepairs_in_longest_read",
              "kmer_size", "window_size")


@pytest.fixture(scope="module")
def cm():
    from genomeworks_amd import cudamapper
    return cudamapper


# ---- round trip ----------------------------------------------------------------------------------------------------

def assert_round_trip(index, where):
    n, n_unique = len(index.representations), len(index.unique_representations)
    with index.to_host() as copy:
        # size: 8 B per element, one direction bit per element in 64-bit words, 12 B per unique representation
        assert copy.nbytes <= 8 * n + 8 * -(-n // 64) + 12 * (n_unique + 1) + 256, where
        back = copy.to_device()
        again = copy.to_device()  # a copy serves any number of restores
    for restored in (back, again):
        for name in ARRAYS:
            a, b = getattr(index, name), getattr(restored, name)
            assert a.dtype == b.dtype and a.shape == b.shape, (where, name)
            assert a.tobytes() == b.tobytes(), (where, name)
        for name in ATTRIBUTES:
            assert getattr(index, name) == getattr(restored, name), (where, name)
        restored.close()
    return n


def test_round_trip_covid(cm):
    reads = MC.covid_reads()[1]
    for hashed in (True, False):
        for F in (1e-3, 1.0):
            n = assert_round_trip(cm.Index(reads, 15, 10, hashed, F), "covid hashed=%s F=%g" % (hashed, F))
            assert n > 1000


def test_round_trip_synthetic(cm):
    reads = MC.synthetic_reads(23, 20000, 7, 2000, 0.03)
    for hashed in (True, False):
        for F in (1e-3, 1.0):
            index = cm.Index(reads, 15, 10, hashed, F)
            assert set(np.unique(index.directions_of_reads)) == {0, 1}
            assert_round_trip(index, "synthetic hashed=%s F=%g" % (hashed, F))
    index = cm.Index(reads[3:9], 15, 10, first_read_id=5)
    assert index.smallest_read_id == 5
    assert_round_trip(index, "first_read_id=5")
    # a read shorter than k + w - 1 is skipped by the index; the ids behind it shift, and the copy keeps all of that
    short = reads[:3] + ["ACGTACGT"] + reads[3:6]
    index = cm.Index(short, 15, 10)
    assert index.number_of_reads == 7 and int(index.read_ids.max()) == 5
    assert_round_trip(index, "short read")


def test_round_trip_tail_wave(cm):
    """element counts around multiples of 64: the last bitmap word is partly used"""
    reads = MC.synthetic_reads(5, 3000, 3, 600, 0.02, min_length=100)
    seen = set()
    for n_reads in range(1, len(reads) + 1):
        for k, w in ((15, 10), (11, 7)):
            index = cm.Index(reads[:n_reads], k, w)
            seen.add(assert_round_trip(index, "%d reads k=%d w=%d" % (n_reads, k, w)) % 64)
    assert len(seen - {0}) >= 3  # counts that are not multiples of 64 were among them


def test_round_trip_from_arrays_with_empty_sections(cm):
    # sections 0 and 3 hold elements, 1 and 2 and the last are empty
    index = cm.Index.from_arrays(read_ids=[0, 1, 1, 2, 3], positions_in_reads=[7, 0, 9, 4, 4],
                                 unique_representations=[3, 5, 8, 13, 21],
                                 first_occurrence_of_representations=[0, 2, 2, 2, 5, 5], first_read_id=0,
                                 number_of_reads=4, number_of_basepairs_in_longest_read=40)
    assert list(index.representations) == [3, 3, 13, 13, 13]
    assert_round_trip(index, "empty sections")
    # 130 elements in three words, an empty section first and elements that begin at a word boundary
    n = 130
    first = [0, 0, 64, 64, 129, n]
    index = cm.Index.from_arrays(np.arange(n) % 7, np.arange(n) * 3, [1, 2, 2**40, 2**63, 2**64 - 1], first, 0, 7, 500)
    assert int(index.representations[0]) == 2 and int(index.representations[129]) == 2**64 - 1
    assert_round_trip(index, "130 elements")


def test_round_trip_empty_index(cm):
    for index in (cm.Index([], 15, 10), cm.Index(["ACGT", "AC"], 15, 10, first_read_id=3)):
        assert index.number_of_reads == 0 and len(index.representations) == 0
        assert len(index.first_occurrence_of_representations) == 0
        assert_round_trip(index, "empty")


# ---- the kernel-level C-ABI: bitmap bits, and values that one bit cannot hold -----------------------------------------

class GwmIndex(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_unique", C.c_int64), ("representations", C.c_void_p), ("read_ids", C.c_void_p),
                ("positions_in_reads", C.c_void_p), ("directions", C.c_void_p), ("unique_representations", C.c_void_p),
                ("first_occurrence_of_representations", C.c_void_p), ("n_first_occurrence", C.c_int64),
                ("first_read_id", C.c_uint32), ("number_of_reads", C.c_uint32),
                ("number_of_basepairs_in_longest_read", C.c_uint32), ("stage_ms", C.c_float * 4),
                ("device_slab", C.c_void_p)]


class GwmIndexHostCopy(C.Structure):
    _fields_ = [("slab", C.c_void_p), ("bytes", C.c_int64), ("pack_ms", C.c_float)]


def device_index(torch, directions):
    """a gwm_index over torch tensors: one section, `directions` as given"""
    n = len(directions)
    t = dict(rep=torch.full((n,), 9, dtype=torch.int64, device="cuda"),
             rid=torch.arange(n, dtype=torch.int32, device="cuda") % 5,
             pos=torch.arange(n, dtype=torch.int32, device="cuda") * 2,
             dir=torch.tensor(directions, dtype=torch.uint8, device="cuda"),
             uniq=torch.tensor([9], dtype=torch.int64, device="cuda"),
             first=torch.tensor([0, n], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    x = GwmIndex(n=n, n_unique=1, representations=t["rep"].data_ptr(), read_ids=t["rid"].data_ptr(),
                 positions_in_reads=t["pos"].data_ptr(), directions=t["dir"].data_ptr(),
                 unique_representations=t["uniq"].data_ptr(), first_occurrence_of_representations=t["first"].data_ptr(),
                 n_first_occurrence=2, first_read_id=0, number_of_reads=5, number_of_basepairs_in_longest_read=2 * n)
    return x, t


def test_pack_bitmap_and_refusal_of_other_direction_values(cm):
    import torch
    from genomeworks_amd import _native
    L = _native.mapper()
    L.gwm_index_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gwm_index_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gwm_index_free.argtypes = [C.c_void_p]
    L.gwm_index_free.restype = None
    L.gwm_index_host_copy_free.argtypes = [C.c_void_p]
    L.gwm_index_host_copy_free.restype = None
    L.gwm_index_host_copy_bytes.argtypes = [C.c_void_p]
    L.gwm_index_host_copy_bytes.restype = C.c_int64
    L.gwm_last_error.restype = C.c_char_p

    n = 100  # two waves' worth of words; the second word is used up to bit 35
    directions = [1] * n
    directions[3] = directions[64] = 0
    x, keep = device_index(torch, directions)
    copy = GwmIndexHostCopy()
    assert L.gwm_index_pack(C.byref(x), None, C.byref(copy)) == 0, L.gwm_last_error()
    assert L.gwm_index_host_copy_bytes(C.byref(copy)) == copy.bytes <= 8 * n + 16 + 12 * 2 + 256
    slab = C.string_at(copy.slab, copy.bytes)
    header = np.frombuffer(slab[8:32], np.int64)
    assert list(header) == [n, 1, 2]
    at = 64 + 2 * ((4 * n + 15) // 16 * 16)  # header, read ids, positions; sections start at multiples of 16 B
    words = np.frombuffer(slab[at:at + 16], np.uint64)
    assert int(words[0]) == (2**64 - 1) ^ (1 << 3)
    assert int(words[1]) == ((1 << 36) - 1) ^ 1  # zero beyond n
    back = GwmIndex()
    assert L.gwm_index_unpack(C.byref(copy), None, C.byref(back)) == 0, L.gwm_last_error()
    torch.cuda.synchronize()
    assert back.device_slab and back.n == n and back.number_of_basepairs_in_longest_read == 2 * n
    L.gwm_index_free(C.byref(back))
    assert not back.device_slab and not back.read_ids
    L.gwm_index_host_copy_free(C.byref(copy))
    assert not copy.slab

    for value in (2, 255):
        directions = [0, 1] * 50
        directions[77] = value
        x, keep = device_index(torch, directions)
        copy = GwmIndexHostCopy()
        assert L.gwm_index_pack(C.byref(x), None, C.byref(copy)) == -1
        assert b"direction" in L.gwm_last_error() and not copy.slab and copy.bytes == 0
        assert keep["dir"].cpu().tolist() == directions  # and the index is as it was


# ---- batcher -------------------------------------------------------------------------------------------------------

def load_vectors():
    with open(os.path.join(HERE, "golden", "cudamapper_batcher_vectors.json")) as f:
        return json.load(f)


def library_arguments(case):
    same = case.get("same_query_and_target", True)
    return dict(query_lengths=case["query_lengths"], target_lengths=None if same else case["target_lengths"],
                query_indices_in_host_memory=case["query_indices_per_host_batch"],
                query_indices_in_device_memory=case["query_indices_per_device_batch"],
                target_indices_in_host_memory=case["target_indices_per_host_batch"],
                target_indices_in_device_memory=case["target_indices_per_device_batch"],
                max_basepairs_per_index=case["query_basepairs_per_index"],
                max_basepairs_per_target_index=case["target_basepairs_per_index"])


def as_lists(batches):
    return [[[list(d) for d in host[0]], [list(d) for d in host[1]],
             [[[list(d) for d in dq], [list(d) for d in dt]] for dq, dt in device]] for host, device in batches]


def test_batcher_vectors(cm):
    for case in load_vectors()["cases"]:
        got = cm.generate_batches_of_indices(**library_arguments(case))
        assert as_lists(got) == case["expected"], case["source"]
    lengths = [4, 6] * 7
    for counts in ((1, 1, 1, 1), (3, 2, 3, 2), (10, 5, 10, 5)):
        assert as_lists(cm.generate_batches_of_indices(lengths, None, *counts, max_basepairs_per_index=10)) == \
            as_lists(B.generate_batches_of_indices(lengths, None, *counts, query_basepairs_per_index=10))
    for counts in ((1, 1, 1, 1), (2, 1, 3, 2), (10, 5, 10, 5), (7, 2, 2, 1)):
        assert as_lists(cm.generate_batches_of_indices(lengths, [7, 3, 2] * 5, *counts, max_basepairs_per_index=10)) == \
            as_lists(B.generate_batches_of_indices(lengths, [7, 3, 2] * 5, *counts, query_basepairs_per_index=10))


def test_batcher_errors_write_nothing(cm):
    from genomeworks_amd import _native
    L = _native.mapper()
    cases = [c for c in load_vectors()["exceptions"] if c["expressible"]]
    assert len(cases) == 3
    for case in cases:
        with pytest.raises(cm.MapperError):
            cm.generate_batches_of_indices(**library_arguments(case))
    lengths = np.array([5] * 12, np.int64)
    targets = np.array([5] * 7, np.int64)
    for counts in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (2, 5, 2, 5), (10, 5, 1, 2)):
        with pytest.raises(cm.MapperError):
            cm.generate_batches_of_indices(lengths, targets, *counts, max_basepairs_per_index=10)
        out = np.full(4096, 0xABABABAB, np.uint32)
        rc = L.gw_mapper_generate_batches_of_indices(lengths.ctypes.data, len(lengths), targets.ctypes.data,
                                                     len(targets), 10, 10, *counts, out.ctypes.data, len(out))
        assert rc == -1 and (out == 0xABABABAB).all()
    with pytest.raises(cm.MapperError):
        cm.map_reads_batched(["ACGT" * 20] * 4, query_indices_in_host_memory=2, query_indices_in_device_memory=5)
    with pytest.raises(cm.MapperError):  # the same set: -C has to be -Q
        cm.map_reads_batched(["ACGT" * 20] * 4, query_indices_in_host_memory=4, target_indices_in_host_memory=2)


# ---- the cached driver ---------------------------------------------------------------------------------------------

ALL_TO_ALL = [(1, 1, 1, 1), (2, 1, 2, 1), (3, 2, 3, 2), (10, 5, 10, 5)]
QUERY_VS_TARGET = [(2, 1, 3, 2), (10, 5, 10, 5)]
VARIANTS = [dict(), dict(rescue_overlap_ends=True, drop_fused_overlaps=True), dict(align=True)]


@pytest.fixture(scope="module")
def batch_reads():
    return MC.synthetic_reads(23, 20000, 7, 2000, 0.03)


def keywords(counts):
    return dict(zip(("query_indices_in_host_memory", "query_indices_in_device_memory", "target_indices_in_host_memory",
                     "target_indices_in_device_memory"), counts))


def split_by_pair(overlaps, query_indices, target_indices):
    """the rows of a one-pair-at-a-time run, per index pair, in their order"""
    def index_of(read_ids, indices):
        starts = np.array([first for first, count in indices if count > 0])
        found = [(first, count) for first, count in indices if count > 0]
        return [found[i] for i in np.searchsorted(starts, read_ids, side="right") - 1]
    qi = index_of(overlaps["query_read_id"], query_indices)
    ti = index_of(overlaps["target_read_id"], target_indices)
    parts = {}
    for i, pair in enumerate(zip(qi, ti)):
        parts.setdefault(pair, []).append(i)
    for pair, rows in parts.items():
        assert rows == list(range(rows[0], rows[-1] + 1)), "a pair's records are not contiguous"
    return parts


def in_pair_order(per_pair, pairs):
    """the rows of the one-pair-at-a-time run, pair after pair in the order `pairs` gives (numpy's concatenate would
    drop the padding of the record type, so the expected records are taken by row)"""
    return np.array([i for p in pairs for i in per_pair.get(p, [])], np.int64)


def check_driver(cm, queries, targets, limit, settings):
    all_to_all = targets is None
    qd = P.group_reads_into_indices([len(r) for r in queries], limit)
    td = qd if all_to_all else P.group_reads_into_indices([len(r) for r in targets], limit)
    n_q, n_t = len([d for d in qd if d[1]]), len([d for d in td if d[1]])
    for variant in VARIANTS:
        kw = dict(filtering_parameter=1.0, max_basepairs_per_index=limit, **variant)
        align = variant.get("align", False)
        base_timings = {}
        base = cm.map_reads_batched(queries, targets, timings=base_timings, **kw)
        base_overlaps, base_cigars = base if align else (base, None)
        assert len(base_overlaps) > 50
        per_pair = split_by_pair(base_overlaps, qd, td)
        for counts in settings:
            where = "limit %d %s %s %s" % (limit, "all-to-all" if all_to_all else "query-vs-target", counts, variant)
            pairs, builds, restores = B.walk(qd, td, all_to_all, *counts)
            timings = {}
            got = cm.map_reads_batched(queries, targets, timings=timings, **keywords(counts), **kw)
            got_overlaps, got_cigars = got if align else (got, None)
            rows = in_pair_order(per_pair, pairs)
            assert sorted(rows) == list(range(len(base_overlaps))), where
            want_overlaps = base_overlaps[rows]
            assert got_overlaps.dtype == want_overlaps.dtype and np.array_equal(got_overlaps, want_overlaps), where
            if align:
                assert got_cigars == [base_cigars[i] for i in rows], where
            assert timings["index_pairs"] == base_timings["index_pairs"] == len(pairs), where
            print(where, "builds", timings["index_builds"], "restores", timings["index_restores"],
                  "pack ms %.3f unpack ms %.3f" % (timings["pack"], timings["unpack"]))
            assert (timings["index_builds"], timings["index_restores"]) == (builds, restores), where
            if counts[0] >= len(qd) and counts[2] >= len(td):
                assert timings["index_builds"] == (n_q if all_to_all else n_q + n_t), where
            if counts == (1, 1, 1, 1):
                assert np.array_equal(got_overlaps, base_overlaps), where
                off_diagonal = sum(1 for a, b in pairs if not all_to_all or a != b)
                assert timings["index_builds"] <= n_q + off_diagonal and timings["index_restores"] == 0, where
            if restores > 0:
                assert timings["unpack"] > 0 and timings["pack"] > 0, where


@pytest.mark.parametrize("limit", [45000, 15000])
def test_cached_driver_all_to_all(cm, batch_reads, limit):
    groups = P.group_reads_into_indices([len(r) for r in batch_reads], limit)
    assert len(groups) >= (3 if limit == 45000 else 6)
    check_driver(cm, batch_reads, None, limit, ALL_TO_ALL)


@pytest.mark.parametrize("limit", [45000, 15000])
def test_cached_driver_query_vs_target(cm, batch_reads, limit):
    half = len(batch_reads) // 2
    check_driver(cm, batch_reads[:half], batch_reads[half:], limit, QUERY_VS_TARGET)


def test_cached_driver_two_index_sizes_all_to_all(cm, batch_reads):
    """all against all with a target index size of its own: the batches are the whole matrix, the walk still drops the
    lower triangle, and the one-pair-at-a-time run is the oracle's map_batched"""
    kw = dict(filtering_parameter=1.0, max_basepairs_per_index=45000, max_basepairs_per_target_index=30000)
    base = cm.map_reads_batched(batch_reads, **kw)
    lengths = [len(r) for r in batch_reads]
    qd, td = P.group_reads_into_indices(lengths, 45000), P.group_reads_into_indices(lengths, 30000)
    pairs = B.walk(qd, td, True, same_indices=False)[0]
    assert pairs == B.pairs_of_map_batched(qd, td, True)
    per_pair = split_by_pair(base, qd, td)
    timings = {}
    got = cm.map_reads_batched(batch_reads, timings=timings, **keywords((3, 2, 2, 1)), **kw)
    pairs, builds, restores = B.walk(qd, td, True, 3, 2, 2, 1, same_indices=False)
    assert len(base) > 50 and np.array_equal(got, base[in_pair_order(per_pair, pairs)])
    assert (timings["index_builds"], timings["index_restores"]) == (builds, restores)


# ---- the tool ------------------------------------------------------------------------------------------------------

def run_tool(args):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def fasta(batch_reads, tmp_path_factory):
    path = tmp_path_factory.mktemp("cache") / "reads.fasta"
    with open(path, "w") as f:
        for i, r in enumerate(batch_reads):
            f.write(">read_%d\n%s\n" % (i, r))
    return str(path)


def test_tool_with_the_cache_letters(cm, batch_reads, fasta):
    names = ["read_%d" % i for i in range(len(batch_reads))]
    lengths = [len(r) for r in batch_reads]
    run = run_tool(["-i", "0.015", "-Q", "10", "-q", "5", fasta, fasta])
    assert run.returncode == 0, run.stderr
    assert "-C / --target-indices-in-host-memory not set, using -Q / --query-indices-in-host-memory value: 10" in run.stderr
    assert "-c / --target-indices-in-device-memory not set, using -q / --query-indices-in-device-memory value: 5" in run.stderr
    o = cm.map_reads_batched(batch_reads, filtering_parameter=1.0, max_basepairs_per_index=15000,
                             **keywords((10, 5, 10, 5)))
    assert len(o) > 100
    assert run.stdout == cm.format_paf(o, names, lengths, names, lengths, 15)
    plain = run_tool(["-i", "0.015", fasta, fasta])
    ones = run_tool(["-i", "0.015", "-Q", "1", "-q", "1", fasta, fasta])
    assert plain.returncode == 0 and ones.returncode == 0, plain.stderr + ones.stderr
    assert plain.stdout == ones.stdout and "not set" not in plain.stderr
    assert plain.stdout == cm.format_paf(cm.map_reads_batched(batch_reads, filtering_parameter=1.0,
                                                              max_basepairs_per_index=15000),
                                         names, lengths, names, lengths, 15)
    assert plain.stdout != run.stdout and sorted(plain.stdout.splitlines()) == sorted(run.stdout.splitlines())


def test_tool_refuses_what_the_reference_refuses(fasta, tmp_path):
    other = tmp_path / "other.fasta"
    other.write_text(">a\nACGT\n")
    for args in (["-Q", "2", "-q", "5"], ["-C", "1", "-c", "2"], ["-Q", "0", "-q", "0"], ["-q", "-1"]):
        for target in (fasta, str(other)):
            run = run_tool(args + [fasta, target])
            assert run.returncode != 0 and run.stdout == "" and "cudamapper:" in run.stderr, (args, run.stderr)
    assert "larger or equal" in run_tool(["-Q", "2", "-q", "5", fasta, fasta]).stderr
    run = run_tool(["-Q", "4", "-q", "2", "-C", "6", "-c", "2", fasta, fasta])  # the same file: -C has to be -Q
    assert run.returncode != 0 and run.stdout == "" and "cudamapper:" in run.stderr
