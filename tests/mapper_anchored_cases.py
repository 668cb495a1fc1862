"""Inputs of the anchored-alignment tests (tests/test_mapper_anchored_oracle.py, tests/test_gpu_mapper_anchored.py):
hand-made anchor lists at every edge of rules G1-G6, the 16 chained records of the synthetic reads, and the capacity
case. Anchors are (query_position_in_read, target_position_in_read) rows in forward read coordinates."""
import functools

import numpy as np

import mapper_chain_cases as CC
import oracle_mapper as O
import oracle_mapper_anchored as OG
import oracle_mapper_chain as OC
from oracle_mapper import OVERLAP

K = 15
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
SCORINGS = (None, (4, 6, 2, 16), (6, 4, 3, 24, 2, 16))  # no scoring, one piece, the two-piece default at band 16


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist()).decode()


def mutated(rng, s, rate):
    """s with every base substituted, followed by an inserted base or deleted with probability rate / 3 each"""
    out = []
    for c in s:
        u = rng.random()
        if u < rate / 3:
            out.append("ACGT"[int(rng.integers(0, 4))])
        elif u < 2 * rate / 3:
            out += [c, "ACGT"[int(rng.integers(0, 4))]]
        elif u >= rate:
            out.append(c)
    return "".join(out)


def revcomp(s):
    return s.encode().translate(_COMP)[::-1].decode()


def record(qid, tid, qs, qe, ts, te, strand, residues=0):
    o = np.zeros((), OVERLAP)
    o["query_read_id"], o["target_read_id"] = qid, tid
    o["query_start_position_in_read"], o["query_end_position_in_read"] = qs, qe
    o["target_start_position_in_read"], o["target_end_position_in_read"] = ts, te
    o["relative_strand"], o["num_residues"], o["overlap_complete"] = ord(strand), residues, 1
    return o


def lists(per_record):
    """(anchor_offsets, anchor_positions) of [[(q, t), ...], ...]"""
    offsets = np.cumsum([0] + [len(a) for a in per_record]).astype(np.int64)
    rows = [r for a in per_record for r in a]
    return offsets, np.array(rows, np.uint32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def hand_made():
    """(queries, targets, overlaps, per-record anchor lists, what each record is there for). Query 0 is a 6 % copy of
    target 0, query 1 one of the reverse complement of target 1; the anchors are diagonal points of the slices, not
    k-mer matches -- the rules read positions only. Slices: n = 400, m = 410 on '+', n = 380, m = 372 on '-'."""
    rng = np.random.default_rng(41)
    targets = [random_bases(rng, 700), random_bases(rng, 650)]
    queries = [mutated(rng, targets[0], 0.06), mutated(rng, revcomp(targets[1]), 0.06), random_bases(rng, 2100)]
    targets.append(mutated(rng, queries[2], 0.04))
    qs, qe, ts, te = 100, 500, 120, 530
    plus = lambda: record(0, 0, qs, qe, ts, te, "+")
    n, m = qe - qs, te - ts
    mqs, mqe, mts, mte = 90, 470, 184, 556  # the slices that correspond: revcomp(T)[94:466] is T[184:556] back to front
    minus = lambda: record(1, 1, mqs, mqe, mts, mte, "-")
    mv = lambda v: mte - v - K  # the target position whose k-mer starts at v of the reverse-complemented slice
    out = []
    # on and next to u = 0, u = n, v = 0, v = m: only the anchors strictly inside count
    out.append((plus(), [(qs, ts + 5), (qs + 1, ts), (qs + 1, ts + 1), (qs + 200, ts + 204), (qs + n - 1, ts + m - 1),
                         (qs + n, ts + m - 1), (qs + n - 1, ts + m), (qs + n, ts + m)], "corners"))
    # '-': v = -k, 0 and 1, then the far end v = m - 1, m
    out.append((minus(), [(mqs + 1, mte), (mqs + 2, mv(0)), (mqs + 3, mv(1)), (mqs + 150, mv(146)), (mqe - 2, mv(372 - 1)),
                          (mqe - 1, mv(372))], "minus corners"))
    # two anchors in one cell and in neighbouring cells of 64: u = 63, 64, 65, then 127 and 128
    out.append((plus(), [(qs + 63, ts + 60), (qs + 64, ts + 66), (qs + 65, ts + 67), (qs + 127, ts + 130),
                         (qs + 128, ts + 131)], "cells"))
    out.append((plus(), [], "no anchors"))
    out.append((minus(), [(mqs + 40 * i, mv(39 * i)) for i in range(1, 9)], "minus diagonal"))
    # an invalid anchor in the middle of a list breaks neither order nor cells
    out.append((plus(), [(qs + 10, ts + 10), (qs + 5, ts + 900), (qs + 20, ts + 21), (qs + 300, ts + 310)], "stray"))
    # n or m of 0: no anchor can be valid
    out.append((record(0, 0, 200, 200, 120, 140, "+"), [(200, 125), (201, 126)], "n = 0"))
    out.append((record(0, 0, 200, 230, 300, 300, "+"), [(210, 300)], "m = 0"))
    out.append((record(0, 0, 50, 50, 60, 60, "+"), [], "both empty"))
    # a long record: spacing 1 gives far more than 128 pieces
    out.append((record(2, 2, 0, len(queries[2]), 0, len(targets[2]), "+"),
                _diagonal_anchors(queries[2], targets[2], 7), "long"))
    assert len(out[-1][1]) > 140
    overlaps = np.array([o for o, _, _ in out], OVERLAP)
    return queries, targets, overlaps, [a for _, a, _ in out], [w for _, _, w in out]


def _diagonal_anchors(q, t, step):
    """exact k-mer matches of q in t near the diagonal, one per `step` query bases at the most, strictly increasing"""
    out, last_t = [], -1
    for u in range(1, len(q) - K, step):
        for shift in range(0, 60):
            for v in (u + shift, u - shift):
                if v > last_t and 0 < v < len(t) - K and q[u:u + K] == t[v:v + K]:
                    out.append((u, v))
                    last_t = v
                    break
            else:
                continue
            break
    return out


def not_monotone():
    """the hand-made call with records 2 and 5 broken: 2 repeats a query position, 5 steps back in the target"""
    queries, targets, overlaps, anchors, _ = hand_made()
    anchors = [list(a) for a in anchors]
    anchors[2] = anchors[2][:2] + [(anchors[2][1][0], anchors[2][1][1] + 1)] + anchors[2][2:]
    anchors[5] = [(110, 130), (120, 129), (400, 430)]
    return queries, targets, overlaps, anchors


def piece_count_records(counts=(1, 63, 64, 65)):
    """records over read pair 2 of the hand-made set with exactly these numbers of pieces at spacing 1: c - 1 anchors
    on consecutive exact matches"""
    queries, targets, _, anchors, _ = hand_made()
    long_anchors = anchors[-1]
    records, per_record = [], []
    for c in counts:
        records.append(record(2, 2, 0, len(queries[2]), 0, len(targets[2]), "+"))
        per_record.append(long_anchors[5:5 + c - 1])
    return queries, targets, np.array(records, OVERLAP), per_record


def small_slot_records():
    """records whose first pieces have slots of 1 .. 5 bytes and more: anchors one or two bases apart in query and
    target right behind the slices' starts"""
    queries, targets, _, _, _ = hand_made()
    records, per_record = [], []
    for shift in range(4):  # every alignment of the record's slot within a dword
        qs, ts = 100 + shift, 120
        records.append(record(0, 0, qs, qs + 300, ts, ts + 305, "+"))
        steps = [(1, 1), (1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3), (3, 3), (4, 3), (5, 5), (7, 6)]
        u = v = 0
        rows = []
        for du, dv in steps:
            u, v = u + du, v + dv
            rows.append((qs + u, ts + v))
        per_record.append(rows)
        # a slot of one byte: a piece needs a base of both sides, so only a record of one base has it
        records.append(record(0, 0, 200, 200 + (shift & 1), 120, 120 + 1 - (shift & 1), "+"))
        per_record.append([])
    return queries, targets, np.array(records, OVERLAP), per_record


SIXTEEN = tuple(range(0, 336, 21))


@functools.lru_cache(maxsize=None)
def synthetic():
    """the 40 synthetic reads, their anchors and the chaining oracle's records with their chains"""
    reads, _ = CC.reads_with_origin(CC.SYNTHETIC_SEED)
    index = O.index(reads, K, 10, True, 1.0)
    anchors = O.anchors(index, index)
    overlaps, scores, chains = OC.chain_overlaps(anchors, with_chains=True)
    return reads, anchors, overlaps, chains


@functools.lru_cache(maxsize=None)
def sixteen_records():
    """(reads, the 16 records with indices 0, 21, ..., 315, their anchor lists)"""
    reads, anchors, overlaps, chains = synthetic()
    picked = list(SIXTEEN)
    offsets, positions = OG.lists_of([chains[i] for i in picked], anchors)
    return reads, overlaps[picked], offsets, positions


DELETION = 450


@functools.lru_cache(maxsize=None)
def capacity_case(deletions=5, length=DELETION, seed=23, target_length=5000):
    """(query, target, overlap record, anchors): the query is the random target with `deletions` deletions of `length`
    bases, evenly placed; exact anchors every 100 target bases whose k-mer lies outside the deletions"""
    rng = np.random.default_rng(seed)
    target = random_bases(rng, target_length)
    room = target_length // deletions
    holes = [(room * i + (room - length) // 2, room * i + (room - length) // 2 + length) for i in range(deletions)]
    query = "".join(target[a:b] for a, b in zip([0] + [e for _, e in holes], [s for s, _ in holes] + [target_length]))
    rows = []
    for t in range(100, target_length - K, 100):
        if any(t + K > s and t < e for s, e in holes):
            continue
        q = t - sum(e - s for s, e in holes if e <= t)
        assert query[q:q + K] == target[t:t + K]
        rows.append((q, t))
    return query, target, record(0, 0, 0, len(query), 0, target_length, "+", len(rows)), rows
