"""The alignment stage of cudamapper as a consumer of cudaaligner: `align_overlaps` tool,
PAF in -> PAF with cg:Z: CIGARs out (reference: cudamapper/src/main.cu:54-187, utils.cpp:41-124). Every record the tool
writes is replayed over its reads (tests/cigar_replay.py) and held to the optimal edit distance of its slices."""
import os
import random
import re
import subprocess

import pytest

import cigar_replay as R
import mapper_cases as MC
import oracle_aligner as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "genomeworks_amd", "bin", "align_overlaps")
TOOL_TIMEOUT = 300  # seconds for one run of the tool
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def mutate(rng, s, rate):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue                                   # deletion
        if r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))             # substitution
            continue
        out.append(c)
        if r < rate:
            out.append(rng.choice("ACGT"))             # insertion
    return "".join(out)


def make_case(tmp_path, n_reads=14, seed=11):
    """Reads sampled from a random genome (some stored reverse-complemented) and every pairwise overlap of their
    genome intervals as PAF records with approximate read coordinates."""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(9000))
    reads = []
    for i in range(n_reads):
        a = rng.randrange(0, 7000)
        b = a + rng.randrange(900, 2000)
        seq = mutate(rng, genome[a:b], 0.06)
        rev = i % 3 == 2
        reads.append(dict(name="read_%d desc" % i, a=a, b=b, seq=revcomp(seq) if rev else seq, rev=rev))
    fasta = tmp_path / "reads.fasta"
    with open(fasta, "w") as f:
        for r in reads:
            f.write(">%s\n" % r["name"])
            for k in range(0, len(r["seq"]), 70):
                f.write(r["seq"][k:k + 70] + "\n")
    lines, expect = [], []
    for i, q in enumerate(reads):
        for j, t in enumerate(reads):
            if i >= j:
                continue
            lo, hi = max(q["a"], t["a"]), min(q["b"], t["b"])
            if hi - lo < 300:
                continue

            def span(r):  # read coordinates of genome interval [lo, hi), scaled, on the stored strand
                n, g = len(r["seq"]), r["b"] - r["a"]
                s, e = (lo - r["a"]) * n // g, (hi - r["a"]) * n // g
                return (n - e, n - s) if r["rev"] else (s, e)
            qs, qe = span(q)
            ts, te = span(t)
            strand = "-" if q["rev"] != t["rev"] else "+"
            lines.append("\t".join(map(str, ["read_%d" % i, len(q["seq"]), qs, qe, strand, "read_%d" % j, len(t["seq"]), ts, te,
                                             7, max(qe - qs, te - ts), 255])))
            tsub = t["seq"][ts:te]
            expect.append((q["seq"][qs:qe], revcomp(tsub) if strand == "-" else tsub))
    paf = tmp_path / "overlaps.paf"
    paf.write_text("\n".join(lines) + "\n")
    return str(fasta), str(paf), lines, expect


def run_tool(args):
    """One run of the tool in a child process of its own, under a time limit."""
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=TOOL_TIMEOUT)


def fasta_reads(path):
    return dict(zip(*MC.read_fasta(path)))


def test_tool_is_built_and_rejects_bad_input(tmp_path):
    assert os.access(TOOL, os.X_OK), "build it with __graft_entry__.build()"
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage: align_overlaps" in r.stderr
    fasta, paf, lines, _ = make_case(tmp_path, n_reads=4)
    bad = tmp_path / "bad.paf"
    bad.write_text(lines[0].replace("read_0", "nobody", 1) + "\n")
    r = subprocess.run([TOOL, fasta, fasta, str(bad)], capture_output=True, text=True)  # fails before any device call
    assert r.returncode == 1 and "unknown read name" in r.stderr
    bad.write_text("read_0\t10\tx\n")
    r = subprocess.run([TOOL, fasta, fasta, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "malformed PAF line 1" in r.stderr
    r = subprocess.run([TOOL, str(tmp_path / "missing.fasta"), fasta, paf], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open FASTA file" in r.stderr


def cigar_lengths(cigar):
    q = t = 0
    for n, op in re.findall(r"(\d+)([MIDX=])", cigar):
        n = int(n)
        if op in "M=X":
            q += n
            t += n
        elif op == "I":  # cudaaligner's convention (cudaaligner.hpp:47-53): insertion = absent in query, present in target
            t += n
        else:
            q += n
    return q, t


@pytest.mark.gpu
def test_paf_cigars_equal_direct_aligner_calls_for_any_engine_count(tmp_path):
    from genomeworks_amd import cudaaligner
    fasta, paf, lines, expect = make_case(tmp_path)
    assert len(lines) > 20 and any("\t-\t" in l for l in lines)
    outs = []
    for engines, batch in ((1, 0), (3, 4), (2, 1000)):
        r = run_tool(["-a", str(engines)] + (["-b", str(batch)] if batch else []) + [fasta, fasta, paf])
        assert r.returncode == 0, r.stderr
        assert "Aligning %d overlaps" % len(lines) in r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] == outs[2]          # record order and CIGARs do not depend on engines / batch size
    got = outs[0].strip().split("\n")
    assert len(got) == len(lines)
    # the same pairs straight through the Python mirror of the Aligner interface (default create_aligner)
    mq, mt = max(len(q) for q, _ in expect), max(len(t) for _, t in expect)
    batch = cudaaligner.CudaAlignerBatch(mq, mt, len(expect))
    for q, t in expect:
        assert batch.add_alignment(q, t) == 0
    batch.align_all()
    ref = batch.get_alignments()
    for line, src, (q, t), a in zip(got, lines, expect, ref):
        cols = line.split("\t")
        assert cols[:9] == src.split("\t")[:9] and cols[11] == "255"
        assert cols[12].startswith("cg:Z:")
        cigar = cols[12][5:]
        assert cigar == a.cigar
        assert cigar_lengths(cigar) == (len(q), len(t))
    # every record describes an optimal global alignment of its slices
    reads = fasta_reads(fasta)
    for line, (q, t) in zip(got, expect):
        assert R.replay_paf(line, reads, reads).edits == A.myers_full(q, t)["edit_distance"], line[:80]


@pytest.mark.gpu
def test_sam_records_carry_the_paf_cigars_in_strand_order(tmp_path):
    """`align_overlaps -S` (cudamapper's -S / print_sam, cudamapper/src/utils.cpp:190-318, without htslib): one @SQ line per
    distinct target read, the @PG line, and per overlap a record whose CIGAR is the `cg:Z:` tag of the PAF output (its runs
    reversed on the reverse strand), whose flag says the strand, whose RNAME / POS are the target read and the 1-based
    target start, with the whole query sequence, and which replays to the alignment of its PAF record."""
    fasta, paf, lines, _expect = make_case(tmp_path)
    p = run_tool(["-a", "2", fasta, fasta, paf])
    assert p.returncode == 0, p.stderr
    s = run_tool(["-a", "2", "-S", fasta, fasta, paf])
    assert s.returncode == 0, s.stderr
    paf_rows = [l.split("\t") for l in p.stdout.strip().split("\n")]
    sam = s.stdout.strip().split("\n")
    header = [l for l in sam if l.startswith("@")]
    records = [l.split("\t") for l in sam if not l.startswith("@")]
    targets_in_order = []
    for row in paf_rows:
        if row[5] not in targets_in_order:
            targets_in_order.append(row[5])
    assert [h.split("\t")[1][3:] for h in header if h.startswith("@SQ")] == targets_in_order
    assert sum(1 for h in header if h.startswith("@PG\tID:cudamapper")) == 1 and header[-1].startswith("@PG")
    assert len(records) == len(paf_rows)
    seqs = {}
    name = None
    for line in open(fasta):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = ""
        else:
            seqs[name] += line.strip()
    for rec, row in zip(records, paf_rows):
        assert len(rec) == 11
        assert rec[0] == row[0] and rec[2] == row[5]
        assert rec[1] == ("16" if row[4] == "-" else "0")
        assert int(rec[3]) == int(row[7]) + 1 and rec[4] == "255"
        # the PAF CIGAR between soft clips for the unaligned ends of the read, with I / D in SAM's sense (cudaaligner names them
        # from the other sequence's side); on the reverse strand SEQ is the reverse complement, the clips swap sides and the
        # runs come in reverse order (the PAF CIGAR walks the forward query against the reverse-complemented target)
        qlen, qs, qe = int(row[1]), int(row[2]), int(row[3])
        head, tail = (qs, qlen - qe) if row[4] == "+" else (qlen - qe, qs)
        runs = re.findall(r"[0-9]+[MID]", row[12][5:])
        assert "".join(runs) == row[12][5:]
        swapped = "".join(runs if row[4] == "+" else runs[::-1]).translate(str.maketrans("ID", "DI"))
        assert rec[5] == ("%dS" % head if head else "") + swapped + ("%dS" % tail if tail else "")
        seq = seqs[row[0]] if row[4] == "+" else seqs[row[0]][::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))
        assert rec[6:9] == ["*", "0", "0"] and rec[9] == seq and rec[10] == "*"
        # SAM validity: the operators that consume the query (M I S = X) add up to len(SEQ), those that consume the reference
        # (M D N = X) to the aligned target span
        ops = re.findall(r"(\d+)([MIDNSHP=X])", rec[5])
        assert "".join(n + o for n, o in ops) == rec[5]
        assert sum(int(n) for n, o in ops if o in "MIS=X") == len(rec[9])
        assert sum(int(n) for n, o in ops if o in "MDN=X") == int(row[8]) - int(row[7])
        # and the SAM record describes the alignment of its PAF record: the same columns, so the same mismatch count
        R.check_sam_against_paf(rec, row, seqs, seqs)


# ---- known answers, worked out by hand --------------------------------------------------------------------------------
# Each target read is a flank, a 120-base core and a flank. Each query read is a clip, the core with one 2-base edit, and
# a clip; the core is reverse-complemented on '-'. Call the query's aligned slice s, in the query's own orientation.
# "ins": two bases enter s after its 10th base, so the aligner's CIGAR is 10M2D110M (cudaaligner's D: query only).
# "del": s loses the two bases that follow its 108th, 10 bases before its end: 108M2I10M (cudaaligner's I: target only).
# The SAM CIGAR swaps I and D and opens with the clip of the read's left end; on '-' SEQ is the reverse complement, so it
# opens with the clip of the right end instead, and the runs come from last to first: 10M2D110M -> 110M2I10M and
# 108M2I10M -> 10M2D108M.
KNOWN_ANSWERS = [  # name, strand, edit, query clips (left, right), target flanks (left, right), PAF CIGAR, SAM CIGAR
    ("minus_ins", "-", "ins", (7, 23), (40, 5), "10M2D110M", "23S110M2I10M7S"),
    ("minus_del", "-", "del", (19, 0), (0, 30), "108M2I10M", "10M2D108M19S"),   # an N in the left clip; POS 1
    ("plus_ins", "+", "ins", (7, 23), (13, 25), "10M2D110M", "7S10M2I110M23S"),
    ("plus_del", "+", "del", (0, 12), (25, 9), "108M2I10M", "108M2D10M12S"),
]
KNOWN_CORE = 120


def _other(*bases):
    """The first of A, C, G, T that is none of `bases`."""
    return next(c for c in "ACGT" if c not in bases)


def known_answer_case(tmp_path):
    """Separate query and target FASTA files and the PAF of the KNOWN_ANSWERS overlaps. The target file starts with a
    decoy and lists the targets in the reverse order of the queries, so RNAME and POS must come from it. Each inserted or
    deleted base differs from the bases it could trade places with, which makes each best alignment unique."""
    rng = random.Random(2026)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    queries, targets, lines, slices = {}, [("decoy", rand(300))], [], []
    for name, strand, edit, (ql, qr), (tl, tr), _, _ in KNOWN_ANSWERS:
        s = rand(KNOWN_CORE)
        if edit == "ins":
            q_slice = s[:10] + _other(s[8], s[9], s[10]) + _other(s[9], s[10], s[11]) + s[10:]
        else:
            s = s[:108] + _other(s[106], s[107], s[110]) + _other(s[107], s[110], s[111]) + s[110:]
            q_slice = s[:108] + s[110:]
        left, right = rand(ql), rand(qr)
        if name == "minus_del":
            left = left[:5] + "N" + left[6:]  # an N inside a clipped end
        query = left + q_slice + right
        target = rand(tl) + (revcomp(s) if strand == "-" else s) + rand(tr)
        queries["q_" + name] = query
        targets.insert(1, ("t_" + name, target))
        lines.append("\t".join(map(str, ["q_" + name, len(query), ql, ql + len(q_slice), strand, "t_" + name, len(target),
                                         tl, tl + KNOWN_CORE, 1, max(len(q_slice), KNOWN_CORE), 255])))
        slices.append((q_slice, s))  # what the aligner sees: the query slice and the target slice on the query's strand
    qf, tf, paf = tmp_path / "ka_queries.fasta", tmp_path / "ka_targets.fasta", tmp_path / "ka.paf"
    qf.write_text("".join(">%s\n%s\n" % kv for kv in queries.items()))
    tf.write_text("".join(">%s\n%s\n" % kv for kv in targets))
    paf.write_text("\n".join(lines) + "\n")
    return str(qf), str(tf), str(paf), queries, dict(targets), lines, slices


def count_optimal_alignments(q, t):
    """(unit-cost edit distance, number of distinct alignments that reach it) by a counting Needleman-Wunsch."""
    m = len(t)
    prev_d, prev_n = list(range(m + 1)), [1] * (m + 1)
    for i in range(1, len(q) + 1):
        cur_d, cur_n = [i] + [0] * m, [1] + [0] * m
        for j in range(1, m + 1):
            moves = ((prev_d[j - 1] + (q[i - 1] != t[j - 1]), prev_n[j - 1]), (prev_d[j] + 1, prev_n[j]),
                     (cur_d[j - 1] + 1, cur_n[j - 1]))
            best = min(d for d, _ in moves)
            cur_d[j], cur_n[j] = best, sum(n for d, n in moves if d == best)
        prev_d, prev_n = cur_d, cur_n
    return prev_d[m], prev_n[m]


def known_sam_record(queries, paf_line, sam_cigar):
    """The SAM record of a PAF line, with the CIGAR worked out on paper."""
    f = paf_line.split("\t")
    seq = queries[f[0]] if f[4] == "+" else R.revcomp(queries[f[0]])
    return "\t".join([f[0], "16" if f[4] == "-" else "0", f[5], str(int(f[7]) + 1), "255", sam_cigar, "*", "0", "0", seq, "*"])


def test_known_answers_are_unique_and_the_oracles(tmp_path):
    """The CIGARs worked out on paper against the oracle, before any device runs: each best alignment is unique, the
    PAF CIGAR is the oracle's, and the SAM CIGAR replays to the same columns. The runs in forward order do not."""
    _, _, _, queries, targets, lines, slices = known_answer_case(tmp_path)
    assert "N" in queries["q_minus_del"][:19] and "N" not in "".join(q for q, _ in slices)
    for (name, strand, _, _, _, paf_cigar, sam_cigar), line, (q, t) in zip(KNOWN_ANSWERS, lines, slices):
        assert count_optimal_alignments(q, t) == (2, 1), name
        assert A.myers_full(q, t)["cigar"] == paf_cigar, name
        p, _ = R.check_sam_against_paf(known_sam_record(queries, line, sam_cigar), line + "\tcg:Z:" + paf_cigar,
                                       queries, targets)
        assert (p.mismatches, p.edits, p.matches) == (0, 2, min(len(q), len(t))), name
        if strand == "-":  # the same clips around the runs in forward order: what align_overlaps -S used to write
            lead, _, trail = re.fullmatch(r"([0-9]+S)?(.*?)([0-9]+S)?", sam_cigar).groups()
            forward = (lead or "") + paf_cigar.translate(str.maketrans("ID", "DI")) + (trail or "")
            assert forward != sam_cigar
            with pytest.raises(R.ReplayError):
                R.check_sam_against_paf(known_sam_record(queries, line, forward), line + "\tcg:Z:" + paf_cigar,
                                        queries, targets)


@pytest.mark.gpu
def test_known_answer_records(tmp_path):
    """align_overlaps on the hand-built overlaps, from separate query and target files: the exact PAF and SAM CIGARs worked
    out on paper, RNAME / POS / SEQ from the right file and strand, and every record replayed."""
    qf, tf, paf, queries, targets, lines, _ = known_answer_case(tmp_path)
    p = run_tool([qf, tf, paf])
    assert p.returncode == 0, p.stderr
    s = run_tool(["-S", qf, tf, paf])
    assert s.returncode == 0, s.stderr
    paf_rows = p.stdout.strip().split("\n")
    sam = s.stdout.strip().split("\n")
    header = [l for l in sam if l.startswith("@")]
    records = [l for l in sam if not l.startswith("@")]
    assert [h for h in header if h.startswith("@SQ")] == \
        ["@SQ\tSN:t_%s\tLN:%d" % (c[0], len(targets["t_" + c[0]])) for c in KNOWN_ANSWERS]
    assert len(paf_rows) == len(records) == len(KNOWN_ANSWERS)
    for (name, strand, _, _, (tl, _), paf_cigar, sam_cigar), line, row, rec in zip(KNOWN_ANSWERS, lines, paf_rows, records):
        assert row == line + "\tcg:Z:" + paf_cigar, name
        f = rec.split("\t")
        assert f[:6] == ["q_" + name, "16" if strand == "-" else "0", "t_" + name, str(tl + 1), "255", sam_cigar], name
        assert f[9] == (R.revcomp(queries["q_" + name]) if strand == "-" else queries["q_" + name]), name
        p_replay, _ = R.check_sam_against_paf(rec, row, queries, targets)
        assert p_replay.edits == 2, name


# ---- mapper -> aligner ------------------------------------------------------------------------------------------------
# Raw '-' overlaps of the mapper end at the last anchor's k-mer start on both reads, which puts their slices up to k
# bases out of step (about 2k extra edits); reads with 3 % errors differ by about 6 %. A strand or coordinate mistake
# aligns unrelated sequence, at about 0.5 edits per base.
MAX_EDIT_RATIO = 0.30


@pytest.mark.gpu
def test_mapper_overlaps_align_end_to_end(tmp_path):
    """cudamapper's overlaps of seeded synthetic reads through align_overlaps: every PAF record replays to an optimal
    alignment of its slices, every SAM record to the same columns, at a bounded edit rate, whatever the engine layout."""
    from genomeworks_amd import cudamapper
    k, w = 15, 10
    worst, n_total, strands = 0.0, 0, set()
    for seed in (51, 52):
        reads = MC.synthetic_reads(seed, 20000, 4, 2000, 0.03)
        assert min(len(r) for r in reads) >= k + w - 1     # every read is indexed, so read ids are list positions
        overlaps = cudamapper.map_reads(reads, k=k, w=w, filtering_parameter=1.0)
        names = ["s%d_read_%d" % (seed, i) for i in range(len(reads))]
        by_name = dict(zip(names, reads))
        fasta, paf = tmp_path / ("reads_%d.fasta" % seed), tmp_path / ("overlaps_%d.paf" % seed)
        fasta.write_text("".join(">%s\n%s\n" % nr for nr in zip(names, reads)))
        lines = []
        for o in overlaps:
            qi, ti = int(o["query_read_id"]), int(o["target_read_id"])
            qs, qe = int(o["query_start_position_in_read"]), int(o["query_end_position_in_read"])
            ts, te = int(o["target_start_position_in_read"]), int(o["target_end_position_in_read"])
            lines.append("\t".join(map(str, [names[qi], len(reads[qi]), qs, qe, chr(o["relative_strand"]), names[ti],
                                             len(reads[ti]), ts, te, int(o["num_residues"]), max(qe - qs, te - ts), 255])))
        paf.write_text("\n".join(lines) + "\n")
        outs = {}
        for mode in ([], ["-S"]):
            for layout in (["-a", "1"], ["-a", "3", "-b", "4"]):
                r = run_tool(layout + mode + [str(fasta), str(fasta), str(paf)])
                assert r.returncode == 0, r.stderr
                # the @PG line carries the command line; everything else must not depend on the engine layout
                outs[tuple(mode + layout)] = [l for l in r.stdout.split("\n") if not l.startswith("@PG")]
        paf_out, sam_out = outs[("-a", "1")], outs[("-S", "-a", "1")]
        assert paf_out == outs[("-a", "3", "-b", "4")] and sam_out == outs[("-S", "-a", "3", "-b", "4")]
        paf_rows = [l for l in paf_out if l]
        records = [l for l in sam_out if l and not l.startswith("@")]
        assert len(paf_rows) == len(records) == len(lines)
        wrong_strand = []
        for line, row, rec in zip(lines, paf_rows, records):
            f = row.split("\t")
            assert f[:9] == line.split("\t")[:9]
            p_replay, _ = R.check_sam_against_paf(rec, row, by_name, by_name)
            q, t = by_name[f[0]], by_name[f[5]]
            (qs, qe), (ts, te) = p_replay.query_span, p_replay.target_span
            t_slice = t[ts:te] if f[4] == "+" else R.revcomp(t[ts:te])
            assert p_replay.edits == A.myers_full(q[qs:qe], t_slice)["edit_distance"], row[:120]
            ratio = p_replay.edits / max(qe - qs, te - ts)
            assert ratio <= MAX_EDIT_RATIO, (ratio, row[:120])
            worst = max(worst, ratio)
            strands.add(f[4])
            if f[4] == "-" and len(wrong_strand) < 5:  # the bound has teeth: the same slices on the wrong strand
                wrong_strand.append(A.myers_full(q[qs:qe], t[ts:te])["edit_distance"] / max(qe - qs, te - ts))
        assert wrong_strand and min(wrong_strand) > MAX_EDIT_RATIO, wrong_strand
        n_total += len(lines)
    assert n_total >= 20 and strands == {"+", "-"}
    print("mapper -> aligner: %d overlaps, largest edit ratio %.4f (bound %.2f)" % (n_total, worst, MAX_EDIT_RATIO))
