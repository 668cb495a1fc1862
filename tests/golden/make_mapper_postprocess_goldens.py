#!/usr/bin/env python3
"""Writes tests/golden/cudamapper_postprocess_reference.npz: what GenomeWorks' own post_process_overlaps and
rescue_overlap_ends answer on seeded inputs. Data only: the inputs and the recorded outputs.

    python tests/golden/make_mapper_postprocess_goldens.py REFERENCE_CHECKOUT

overlapper.cpp and cudamapper_utils.cpp of the checkout are host code; they are compiled with g++ into a temporary
directory against the CUDA header stubs of oracle/simt/cuda_stubs, together with the small harness below (an in-memory
FastaParser, and empty bodies for the one GPU class overlapper.cpp names). Nothing compiled is kept.

Cases (each stored as <case>_queries / _targets (newline-joined reads), <case>_overlaps and the outputs
<case>_post (post_process_overlaps), <case>_post_drop (drop_fused_overlaps), and, where the overlaps lie on the reads,
<case>_rescue (rescue_overlap_ends(50, 0.5) of the input) and <case>_post_rescue (of <case>_post)):
  fuse    hand-shaped overlaps for fusion: pairs merged by each of the three conditions alone, pairs rejected by all,
          both strands, runs of 2, 3 and more, a run that ends the array, mixed strands and read pairs;
  rescue  hand-shaped overlaps on a small read set: head and tail windows of 0, 1..14, 15..49 and 50 bases, ends that
          move in round 1 only, in all three rounds and never, similarity exactly 0.5, reads with N, an odd-length
          '-' target whose middle base lies in a window;
  mapped  the overlaps tests/oracle_mapper.py finds all-vs-all on a seeded read set of both strands.
tests/test_mapper_postprocess_oracle.py asserts the branch counts, so the fixture cannot quietly lose one."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mapper_cases as MC  # noqa: E402
import oracle_mapper as O  # noqa: E402

OUT = os.path.join(HERE, "cudamapper_postprocess_reference.npz")

HARNESS = r"""
#include <claraparabricks/genomeworks/cudamapper/overlapper.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include "overlapper_triggered.hpp"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudamapper;
OverlapperTriggered::OverlapperTriggered(DefaultDeviceAllocator a, const cudaStream_t s) : _allocator(a), _cuda_stream(s) {}
void OverlapperTriggered::get_overlaps(std::vector<Overlap>&, const device_buffer<Anchor>&, bool, int64_t, int64_t, int64_t, float) {}
struct MemoryParser : io::FastaParser
{
    std::vector<io::FastaSequence> reads;
    number_of_reads_t get_num_seqences() const override { return static_cast<number_of_reads_t>(reads.size()); }
    const io::FastaSequence& get_sequence_by_id(read_id_t i) const override { return reads.at(i); }
};
static void read_set(MemoryParser& p)
{
    size_t n; std::cin >> n;
    for (size_t i = 0; i < n; ++i) { std::string s; std::cin >> s; if (s == ".") s.clear(); p.reads.push_back({"r" + std::to_string(i), s}); }
}
static void dump(const char* tag, const std::vector<Overlap>& v)
{
    std::printf("%s %zu\n", tag, v.size());
    for (const Overlap& o : v)
        std::printf("%u %u %u %u %u %u %d %u %d\n", o.query_read_id_, o.target_read_id_, o.query_start_position_in_read_,
                    o.target_start_position_in_read_, o.query_end_position_in_read_, o.target_end_position_in_read_,
                    int(static_cast<unsigned char>(o.relative_strand)), o.num_residues_, int(o.overlap_complete));
}
int main()
{
    MemoryParser q, t;
    read_set(q); read_set(t);
    size_t n; int with_rescue; std::cin >> n >> with_rescue;
    std::vector<Overlap> in(n);
    for (Overlap& o : in)
    {
        int strand, complete;
        std::cin >> o.query_read_id_ >> o.target_read_id_ >> o.query_start_position_in_read_ >> o.target_start_position_in_read_
                 >> o.query_end_position_in_read_ >> o.target_end_position_in_read_ >> strand >> o.num_residues_ >> complete;
        o.relative_strand = static_cast<RelativeStrand>(strand);
        o.overlap_complete = complete != 0;
    }
    std::vector<Overlap> post = in, drop = in;
    Overlapper::post_process_overlaps(post, false);
    Overlapper::post_process_overlaps(drop, true);
    dump("post", post);
    dump("post_drop", drop);
    if (with_rescue)
    {
        std::vector<Overlap> r = in, pr = post;
        Overlapper::rescue_overlap_ends(r, q, t, 50, 0.5);
        Overlapper::rescue_overlap_ends(pr, q, t, 50, 0.5);
        dump("rescue", r);
        dump("post_rescue", pr);
    }
    return 0;
}
"""

FIELDS = ["query_read_id", "target_read_id", "query_start_position_in_read", "target_start_position_in_read",
          "query_end_position_in_read", "target_end_position_in_read", "relative_strand", "num_residues",
          "overlap_complete"]
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def ov(q, t, qs, qe, ts, te, strand="+", res=5, complete=1):
    return (q, t, qs, ts, qe, te, ord(strand), res, complete)


def fuse_case():
    """Overlaps for fusion only (their coordinates are free). Pair kinds, all with gaps >= 500 unless said:
    short: both gaps < 500; ratio: min / max > 0.8; relative: both gaps < 20 % of the summed lengths; none."""
    o = []
    pair = 0

    def block(strand, kinds, lengths=3000):
        """a chain of overlaps on one read pair whose consecutive pairs are of the given kinds"""
        nonlocal pair
        pair += 1
        q, t = 2 * pair, 2 * pair + 1
        qs, tpos = 1000, 100000
        recs = [(qs, qs + lengths, tpos, tpos + lengths)]
        for kind in kinds:
            qgap, tgap = {"short": (100, 499), "short0": (0, 0), "short_only": (150, 450), "ratio": (1000, 1249), "ratio_edge": (800, 1000),
                          "relative": (1000, 600), "none": (3000, 600), "none_q": (700, 100), "none_t": (100, 700),
                          "overlapping": (-200, -300)}[kind]
            pqs, pqe, pts, pte = recs[-1]
            recs.append((pqe + qgap, pqe + qgap + lengths, pte + tgap, pte + tgap + lengths))
        for i, (a, b, c, d) in enumerate(recs):
            if strand == "-":  # target coordinates fall as the query's rise
                c, d = 1000000 - d, 1000000 - c
            o.append(ov(q, t, a, b, c, d, strand, 3 + i))

    for s in "+-":
        block(s, ["short"])
        block(s, ["short_only"], lengths=300)           # neither of the other two conditions holds
        block(s, ["ratio"])
        block(s, ["relative"])
        block(s, ["none"])
        block(s, ["ratio_edge"], lengths=300)          # float(800) / float(1000) lies above the double 0.8: fuses
        block(s, ["none_q"], lengths=1000)
        block(s, ["none_t"], lengths=1000)
        block(s, ["short", "short"])                    # run of 3
        block(s, ["short", "ratio", "relative", "short0"])   # run of 5
        block(s, ["short", "none", "ratio"])            # two runs on one read pair
        block(s, ["overlapping"])                       # second starts before the first ends: abs of a wrapped difference
        block(s, ["relative"], lengths=100)             # short overlaps: gaps are >= 20 % of the lengths
    # mixed strands on one read pair, and neighbours of different read pairs
    o.append(ov(90, 91, 100, 1100, 100, 1100, "+"))
    o.append(ov(90, 91, 1200, 2200, 1200, 2200, "-"))
    o.append(ov(90, 92, 2300, 3300, 2300, 3300, "-"))
    o.append(ov(91, 92, 3400, 4400, 3400, 4400, "-"))
    # huge coordinates: a difference whose int value is negative although the second lies behind the first
    o.append(ov(95, 96, 0, 10, 0, 10, "+"))
    o.append(ov(95, 96, 3000000000, 3000000010, 3000000000, 3000000010, "+"))
    # a strand byte that is neither: never fuses
    o.append(ov(97, 98, 100, 1100, 100, 1100, "*"))
    o.append(ov(97, 98, 1200, 2200, 1200, 2200, "*"))
    # the array ends inside a run of three
    o.append(ov(99, 100, 1000, 2000, 1000, 2000, "+", 7, 1))
    o.append(ov(99, 100, 2100, 3100, 2100, 3100, "+", 8, 0))
    o.append(ov(99, 100, 3200, 4200, 3200, 4200, "+", 9, 1))
    return np.array(o, O.OVERLAP)


def rescue_case(seed=7):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def rnd(n):
        return rng.choice(acgt, n).tobytes()

    def rc(s):
        return s.translate(_COMP)[::-1]

    queries, targets, o = [], [], []

    def add(core_len, qa, qb, ta, tb, reverse, with_n=False, odd=False):
        """query = junk(qa) + core + junk(qb); target = junk(ta) + core + junk(tb), reverse-complemented if asked.
        Returns (query id, target id, offset of the core in the query, in the forward target, core length)."""
        core = bytearray(rnd(core_len))
        if with_n:
            for p in rng.integers(0, core_len, 6):
                core[p] = ord("N")
        core = bytes(core)
        q = rnd(qa) + core + rnd(qb)
        t = rnd(ta) + core + rnd(tb)
        if odd and len(t) % 2 == 0:
            t += b"A"
        queries.append(q)
        targets.append(rc(t) if reverse else t)
        return len(queries) - 1, len(targets) - 1, qa, ta, core_len, len(t)

    def records(info, reverse, insets):
        qi, ti, qa, ta, n, tlen = info
        for x, y in insets:  # the overlap leaves x core bases before its start and y after its end
            qs, qe, ts, te = qa + x, qa + n - y, ta + x, ta + n - y
            if reverse:
                ts, te = tlen - te, tlen - ts
            o.append(ov(qi, ti, qs, qe, ts, te, "-" if reverse else "+"))

    insets = [(0, 0), (1, 14), (7, 3), (14, 1), (15, 49), (30, 20), (49, 15), (50, 50), (60, 75), (100, 100),
              (140, 130), (150, 150), (151, 160), (200, 10)]
    for reverse in (False, True):
        records(add(700, 120, 130, 200, 90, reverse), reverse, insets)
        records(add(700, 0, 0, 5, 9, reverse), reverse, insets)            # core at the very ends of the query
        records(add(600, 40, 10, 0, 0, reverse), reverse, insets)          # ... of the target
        records(add(650, 80, 80, 80, 80, reverse, with_n=True), reverse, insets)
        records(add(401, 60, 60, 60, 60, reverse, odd=True), reverse,
                [(a, b) for a in (0, 20, 60, 130, 215) for b in (0, 20, 60, 130)])  # a = 215: the head window holds the middle base
    # similarity exactly 0.5: one substitution at offset 38 of a 50-base window leaves 24 of 36 k-mers on each side
    base = rnd(600)
    for reverse in (False, True):
        t = bytearray(base)
        for p in (50 + 38, 500 + 38):  # head window [50, 100), tail window [500, 550): k-mers 24..35 hold offset 38
            t[p] = ord("A") if t[p] != ord("A") else ord("C")
        queries.append(base)
        targets.append(rc(bytes(t)) if reverse else bytes(t))
        qi = len(queries) - 1
        ts, te = (600 - 500, 600 - 100) if reverse else (100, 500)
        o.append(ov(qi, qi, 100, 500, ts, te, "-" if reverse else "+"))
    # a zero-length overlap, and one covering whole reads
    queries.append(rnd(300))
    targets.append(queries[-1])
    o.append(ov(len(queries) - 1, len(queries) - 1, 150, 150, 150, 150, "+"))
    o.append(ov(len(queries) - 1, len(queries) - 1, 0, 300, 0, 300, "+"))
    assert len(queries) == len(targets)
    return queries, targets, np.array(o, O.OVERLAP)


def mapped_case(seed=5):
    """Every third read loses 320..900 bases from its middle, so that its overlaps come in two pieces off one diagonal
    (the overlapper leaves those apart; post-processing fuses most of them)."""
    rng = np.random.default_rng(seed)
    reads = []
    for i, r in enumerate(MC.synthetic_reads(seed, 30000, 8, 2500, 0.04)):
        if i % 3 == 0 and len(r) > 2600:
            cut = int(rng.integers(320, 900))
            at = int(rng.integers(800, len(r) - cut - 800))
            r = r[:at] + r[at + cut:]
        reads.append(r.encode())
    return reads, reads, O.map_reads(reads, None, 15, 10, 1.0, **MC.OVERLAP_PARAMS)


def run_reference(exe, queries, targets, overlaps, with_rescue):
    lines = [str(len(queries))] + [q.decode() or "." for q in queries]
    lines += [str(len(targets))] + [t.decode() or "." for t in targets]
    lines.append("%d %d" % (len(overlaps), int(with_rescue)))
    for r in overlaps:
        lines.append(" ".join(str(int(r[f])) for f in FIELDS))
    text = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    out, it = {}, iter(text.splitlines())
    for head in it:
        tag, n = head.split()
        out[tag] = np.array([tuple(int(v) for v in next(it).split()) for _ in range(int(n))], O.OVERLAP)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GW_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "harness.cpp")
        with open(src, "w") as f:
            f.write(HARNESS)
        exe = os.path.join(tmp, "harness")
        inc = [os.path.join(ref, "cudamapper", "include"), os.path.join(ref, "common", "base", "include"),
               os.path.join(ref, "common", "io", "include"), os.path.join(ref, "cudamapper", "src"),
               os.path.join(ROOT, "oracle", "simt", "cuda_stubs"), os.path.join(ROOT, "oracle", "simt")]
        subprocess.run(["g++", "-std=c++17", "-O1", "-w"] + [a for i in inc for a in ("-I", i)] +
                       [src, os.path.join(ref, "cudamapper", "src", "overlapper.cpp"),
                        os.path.join(ref, "cudamapper", "src", "cudamapper_utils.cpp"), "-o", exe], check=True)
        data = {}
        q, t, o = rescue_case()
        cases = [("fuse", [], [], fuse_case(), False), ("rescue", q, t, o, True)]
        q, t, o = mapped_case()
        cases.append(("mapped", q, t, o, True))
        for name, q, t, o, with_rescue in cases:
            data[name + "_queries"] = np.array(b"\n".join(q))
            data[name + "_targets"] = np.array(b"\n".join(t))
            data[name + "_n_reads"] = np.array([len(q), len(t)])
            data[name + "_overlaps"] = o
            for tag, v in run_reference(exe, q, t, o, with_rescue).items():
                data[name + "_" + tag] = v
            print(name, len(o), "overlaps ->", {k: len(v) for k, v in data.items() if k.startswith(name + "_p")})
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
