"""An independent replay of the CIGARs that `align_overlaps` writes: a PAF record's `cg:Z:` tag or a SAM record, walked
over the two reads it names. It knows nothing about how the records were made. It returns the alignment's columns in
forward read coordinates, so that two records of one overlap can be compared column for column, and counts matches,
mismatches and gaps, so that a record can be held to the optimal edit distance of its slices. A record that does not
describe an alignment of its reads raises ReplayError. TEST INFRASTRUCTURE ONLY.

Columns are `(query index, target index, op)`. Both indices are forward read coordinates, and a gap side is None. The op
uses cudaaligner's names (cudaaligner.hpp:47-53) for both record kinds: '=' match, 'X' mismatch, 'I' a base in the
target only, 'D' a base in the query only. A SAM record's own 'I' (query only) and 'D' (reference only) are renamed."""
import re
from typing import NamedTuple, Optional, Tuple

_COMP = str.maketrans("ACGTacgt", "TGCAtgca")  # N and the other IUPAC codes stay as they are


class ReplayError(ValueError):
    pass


def revcomp(s):
    return s.translate(_COMP)[::-1]


def same_base(a, b):
    """A match: equal bases of A, C, G, T in any letter case. N matches nothing."""
    a, b = a.upper(), b.upper()
    return a == b and a in "ACGT"


def parse_cigar(cigar, ops):
    """[(n, op), ...] of a CIGAR made only of <n><op> runs with n >= 1 (no leading zeros) and op in `ops`."""
    if not isinstance(cigar, str) or not re.fullmatch(r"(?:[1-9][0-9]*[%s])+" % re.escape(ops), cigar):
        raise ReplayError("malformed CIGAR %r: expected <n><op> runs with n >= 1 and op in %s" % (cigar, ops))
    return [(int(n), op) for n, op in re.findall(r"([0-9]+)([^0-9])", cigar)]


class Replay(NamedTuple):
    columns: list                         # (query index, target index, op) in the order the record walks them
    matches: int
    mismatches: int
    ins: int                              # cudaaligner 'I': bases in the target only
    dels: int                             # cudaaligner 'D': bases in the query only
    query_span: Tuple[int, int]           # [start, end) of the aligned query bases, forward coordinates
    target_span: Tuple[int, int]          # [start, end) of the aligned target bases, forward coordinates

    @property
    def edits(self):
        return self.mismatches + self.ins + self.dels

    def column_set(self):
        return frozenset(self.columns)


def _fields(record):
    return record.rstrip("\n").split("\t") if isinstance(record, str) else list(record)


def _read(reads, name, what):
    if name not in reads:
        raise ReplayError("%s %r is not among the reads" % (what, name))
    return reads[name]


def _int(field, what):
    if not re.fullmatch(r"-?[0-9]+", field):
        raise ReplayError("%s %r is not an integer" % (what, field))
    return int(field)


class _Walk:
    """Accumulates the columns of one record and checks the operators that name the bases' equality."""

    def __init__(self):
        self.columns, self.counts = [], {"=": 0, "X": 0, "I": 0, "D": 0}

    def pair(self, qi, ti, qbase, tbase, op):
        eq = same_base(qbase, tbase)
        if (op == "=" and not eq) or (op == "X" and eq):
            raise ReplayError("'%s' column on %s / %s (query %d, target %d)" % (op, qbase, tbase, qi, ti))
        col = "=" if eq else "X"
        self.columns.append((qi, ti, col))
        self.counts[col] += 1

    def gap(self, qi, ti):
        op = "D" if ti is None else "I"
        self.columns.append((qi, ti, op))
        self.counts[op] += 1

    def result(self, query_span, target_span):
        c = self.counts
        return Replay(self.columns, c["="], c["X"], c["I"], c["D"], query_span, target_span)


def replay_paf(record, queries, targets):
    """Replay the `cg:Z:` CIGAR of a PAF record. `queries` and `targets` map read names to sequences.

    The CIGAR (cudaaligner's M / = / X / I / D) walks query[qs:qe] against target[ts:te], or on strand '-' against
    the reverse complement of target[ts:te]; it must use up both slices exactly."""
    f = _fields(record)
    if len(f) < 12:
        raise ReplayError("a PAF record has at least 12 fields, this one %d" % len(f))
    qname, strand, tname = f[0], f[4], f[5]
    qlen, qs, qe = (_int(x, "PAF field") for x in f[1:4])
    tlen, ts, te = (_int(x, "PAF field") for x in f[6:9])
    q, t = _read(queries, qname, "query"), _read(targets, tname, "target")
    if strand not in ("+", "-"):
        raise ReplayError("strand %r" % strand)
    if qlen != len(q) or tlen != len(t):
        raise ReplayError("read lengths %d / %d, the reads have %d / %d" % (qlen, tlen, len(q), len(t)))
    if not (0 <= qs <= qe <= qlen and 0 <= ts <= te <= tlen):
        raise ReplayError("coordinates outside the reads")
    tags = [x[5:] for x in f[12:] if x.startswith("cg:Z:")]
    if len(tags) != 1:
        raise ReplayError("%d cg:Z: tags" % len(tags))
    runs = parse_cigar(tags[0], "MID=X")
    reverse = strand == "-"
    walk = _Walk()
    i = j = 0  # offsets into the query slice and into the (possibly reverse-complemented) target slice
    for n, op in runs:
        for _ in range(n):
            if op in "M=X" and (i >= qe - qs or j >= te - ts) or op == "D" and i >= qe - qs or op == "I" and j >= te - ts:
                raise ReplayError("CIGAR %s runs past the end of a slice" % tags[0])
            ti = te - 1 - j if reverse else ts + j
            if op in "M=X":
                tb = t[ti].translate(_COMP) if reverse else t[ti]
                walk.pair(qs + i, ti, q[qs + i], tb, op)
                i, j = i + 1, j + 1
            elif op == "D":
                walk.gap(qs + i, None)
                i += 1
            else:
                walk.gap(None, ti)
                j += 1
    if (i, j) != (qe - qs, te - ts):
        raise ReplayError("CIGAR %s uses %d of %d query and %d of %d target bases" % (tags[0], i, qe - qs, j, te - ts))
    return walk.result((qs, qe), (ts, te))


def replay_sam(record, queries, targets, query_span: Optional[Tuple[int, int]] = None):
    """Replay a SAM record (FLAG 0 or 16). `queries` and `targets` map read names to sequences.

    SEQ must be the read, or on FLAG 16 its reverse complement with N as it is. Soft clips may only open and close the
    CIGAR; the operators that consume the query must add up to len(SEQ). The rest of the CIGAR (SAM's M / = / X / I / D)
    walks SEQ against target[POS-1:], and SEQ indices map back to forward query indices (on FLAG 16, i -> len - 1 - i).
    `query_span`, the [start, end) that another record aligns, makes the clips the read's unaligned ends."""
    f = _fields(record)
    if len(f) < 11:
        raise ReplayError("a SAM record has at least 11 fields, this one %d" % len(f))
    qname, rname, cigar, seq = f[0], f[2], f[5], f[9]
    flag, pos = _int(f[1], "FLAG"), _int(f[3], "POS")
    if flag not in (0, 16):
        raise ReplayError("FLAG %d (only 0 and 16 are written)" % flag)
    read, t = _read(queries, qname, "QNAME"), _read(targets, rname, "RNAME")
    reverse = flag == 16
    if seq != (revcomp(read) if reverse else read):
        raise ReplayError("SEQ is not the read%s" % (" reverse-complemented" if reverse else ""))
    runs = parse_cigar(cigar, "MIDS=X")
    lead = runs.pop(0)[0] if runs and runs[0][1] == "S" else 0
    trail = runs.pop()[0] if runs and runs[-1][1] == "S" else 0
    if not runs or any(op == "S" for _, op in runs):
        raise ReplayError("CIGAR %s: soft clips may only open and close it, around an alignment" % cigar)
    if not 1 <= pos <= len(t):
        raise ReplayError("POS %d outside the target of %d bases" % (pos, len(t)))
    n = len(seq)
    qidx = (lambda k: n - 1 - k) if reverse else (lambda k: k)
    walk = _Walk()
    i, tp = lead, pos - 1
    for run, op in runs:
        for _ in range(run):
            if op in "M=XI" and i >= n - trail or op in "M=XD" and tp >= len(t):
                raise ReplayError("CIGAR %s runs past the end of SEQ or of the target" % cigar)
            if op in "M=X":
                walk.pair(qidx(i), tp, seq[i], t[tp], op)
                i, tp = i + 1, tp + 1
            elif op == "I":  # SAM: a base of the query only
                walk.gap(qidx(i), None)
                i += 1
            else:            # SAM: a base of the reference only
                walk.gap(None, tp)
                tp += 1
    if i != n - trail:
        raise ReplayError("CIGAR %s uses %d of the %d bases of SEQ" % (cigar, i + trail, n))
    aligned = (trail, n - lead) if reverse else (lead, n - trail)
    if query_span is not None and tuple(query_span) != aligned:
        raise ReplayError("CIGAR %s clips the read to [%d, %d), the overlap aligns [%d, %d)"
                          % ((cigar,) + aligned + tuple(query_span)))
    return walk.result(aligned, (pos - 1, tp))


def check_sam_against_paf(sam, paf, queries, targets):
    """Both records of one overlap describe the same alignment: names, strand and spans agree, and both replay to the
    same columns. Returns the two replays (PAF, SAM)."""
    s, p = _fields(sam), _fields(paf)
    p_replay = replay_paf(p, queries, targets)
    if s[:3] != [p[0], "16" if p[4] == "-" else "0", p[5]]:
        raise ReplayError("QNAME / FLAG / RNAME %s do not belong to the PAF record %s" % (s[:3], p[:9]))
    s_replay = replay_sam(s, queries, targets, query_span=p_replay.query_span)
    if s_replay.target_span != p_replay.target_span:
        raise ReplayError("SAM aligns target %s, PAF %s" % (s_replay.target_span, p_replay.target_span))
    if s_replay.column_set() != p_replay.column_set():
        only_sam = sorted(s_replay.column_set() - p_replay.column_set(), key=str)
        raise ReplayError("%d columns differ, e.g. %s only in SAM" % (len(only_sam), only_sam[:3]))
    counts = lambda r: (r.matches, r.mismatches, r.ins, r.dels)
    if counts(s_replay) != counts(p_replay):
        raise ReplayError("counts differ: SAM %s, PAF %s" % (counts(s_replay), counts(p_replay)))
    return p_replay, s_replay
