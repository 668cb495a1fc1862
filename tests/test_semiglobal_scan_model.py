"""A word-level model of the ends scan of the infix / prefix alignment types (genomeworks_amd/semiglobal/gws_ends.hip),
held to the DP oracle (tests/oracle_semiglobal.py). It restates what the kernel does with the same quantities:

  * the column as 32-bit words, lane l of round r owning word 64 r + l, its four pattern words built base by base;
  * the addition of Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq word by word: every lane's own sum, the two ballots "generates a
    carry" / "would pass one on", one 64-bit addition with bit 63 kept out, the carry out of lane 63 taken separately and
    handed to the next round together with the top bits of ph / mh;
  * the bit shifted into word 0: +1 for prefix and for the anchored pass, 0 for infix;
  * the bookkeeping of the word that holds query bit n - 1: the running bottom score, its minimum, the first column
    that reached it (column 0 counts);
  * the second pass over the reversed query and the reversed T[0:te], stopped at the first column whose bottom score is
    d, and bounded by n + d columns.

The lanes of a round are a numpy vector; ballots are Python integers."""
import random

import numpy as np
import pytest

import oracle_semiglobal as S
import semiglobal_cases as K

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
TOP = 1 << 63
LANES = np.arange(64, dtype=np.uint64)


def ballot(flags):
    return int.from_bytes(np.packbits(flags, bitorder="little").tobytes(), "little")


def patterns(query, reverse):
    """eq[c][round] = uint32[64]: bit b of word w = (base 32 w + b of the (reversed) query == "ACTG"[c])."""
    n = len(query)
    rounds = ((n + 31) // 32 + 63) // 64
    eq = np.zeros((4, rounds * 64), np.uint32)
    for i in range(n):
        c = query[n - 1 - i] if reverse else query[i]
        if c in "ACTG":
            eq["ACTG".index(c), i // 32] |= np.uint32(1 << (i % 32))
    return eq.reshape(4, rounds, 64), rounds


def round_advance(eq, pv, mv, carry, ph_top, mh_top):
    xv = eq | mv
    a = eq & pv
    s0 = a + pv                                              # uint32: wraps
    gen, prp = ballot(s0 < a), ballot(s0 == M32)
    A, B = (gen | prp) & ~TOP & M64, gen & ~TOP & M64
    cin = ((A + B + carry) & M64) ^ (prp & ~TOP & M64)
    total = s0 + ((np.uint64(cin) >> LANES) & np.uint64(1)).astype(np.uint32)
    carry = ((gen >> 63) | ((prp >> 63) & (cin >> 63))) & 1
    xh = (total ^ pv) | eq
    ph = mv | ~(xh | pv)
    mh = pv & xh
    ph_lo = np.concatenate(([np.uint32(ph_top)], ph[:-1] >> np.uint32(31)))    # wave_shr:1, lane 0 from the round below
    mh_lo = np.concatenate(([np.uint32(mh_top)], mh[:-1] >> np.uint32(31)))
    phs, mhs = (ph << np.uint32(1)) | ph_lo, (mh << np.uint32(1)) | mh_lo
    return mhs | ~(xv | phs), phs & xv, ph, mh, carry, int(ph[63] >> np.uint32(31)), int(mh[63] >> np.uint32(31))


def scan(query, target, top, reverse=False, stop_at=None, limit=None):
    """Forward (stop_at None): (min_j D[n][j], first column at the minimum). Anchored: the first column whose bottom score
    is stop_at within `limit` columns, or -1. `reverse` reads both sequences back to front."""
    n = len(query)
    cols = len(target) if limit is None else min(len(target), limit)
    eq, rounds = patterns(query, reverse)
    pv = np.full((rounds, 64), M32, np.uint32)
    mv = np.zeros((rounds, 64), np.uint32)
    owner_word, owner_bit = (n - 1) // 32, (n - 1) % 32
    owner_round, owner_lane = owner_word >> 6, owner_word & 63
    score = best = n
    best_col = 0
    for j in range(cols):
        ci = (ord(target[len(target) - 1 - j] if reverse else target[j]) >> 1) & 3
        carry, ph_top, mh_top = 0, top, 0
        for r in range(rounds):
            pv[r], mv[r], ph, mh, carry, ph_top, mh_top = round_advance(eq[ci, r], pv[r], mv[r], carry, ph_top, mh_top)
            if r == owner_round:
                score += int((ph[owner_lane] >> np.uint32(owner_bit)) & 1) - int((mh[owner_lane] >> np.uint32(owner_bit)) & 1)
        if stop_at is None:
            if score < best:
                best, best_col = score, j + 1
        elif score == stop_at:
            return j + 1
    return (best, best_col) if stop_at is None else -1


def ends(query, target, mode):
    """(d, te, tb) the way gwhip_semiglobal_ends() computes them."""
    n, m = len(query), len(target)
    if n == 0 or m == 0:
        return n, 0, 0
    d, te = scan(query, target, 1 if mode == "prefix" else 0)
    if mode == "prefix":
        return d, te, 0
    if d == n:                      # column 0 of the anchored pass
        return d, te, te
    found = scan(query, target[:te], 1, reverse=True, stop_at=d, limit=n + d)
    assert found > 0, "the anchored pass must find its column within n + d"
    return d, te, te - found


def test_carry_out_of_the_last_lane_reaches_the_next_round():
    # 2 049 bases: word 64 is round 1, lane 0. A query of one base repeated against itself: every column carries through all words
    q = "A" * 2049
    assert ends(q, "C" + q, "infix") == S.semiglobal(q, "C" + q, "infix") == (0, 2050, 1)
    assert ends(q, q[:-1] + "C", "prefix") == S.semiglobal(q, q[:-1] + "C", "prefix")


@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_small_lengths_every_target_length(mode):
    rng = random.Random(17)
    for n in K.SMALL_LENGTHS:
        for m in K.target_lengths(n):
            q, t = K.sized_pair(rng, n, m)
            assert ends(q, t, mode) == S.semiglobal(q, t, mode), (n, m)
        for where in ("start", "middle", "end"):
            q, t, begin = K.planted(rng, n, where, edits=False)
            if mode == "infix":
                d, te, tb = ends(q, t, mode)
                assert d == 0 and te - tb == n and (n < 8 or (tb, te) == (begin, begin + n))
            assert ends(q, t, mode) == S.semiglobal(q, t, mode), (n, where)
            q, t, _ = K.planted(rng, n, where, edits=True)
            assert ends(q, t, mode) == S.semiglobal(q, t, mode), (n, where)


@pytest.mark.parametrize("n", K.LARGE_LENGTHS)
def test_large_lengths(n):
    rng = random.Random(n)
    for m in K.target_lengths(n):
        q, t = K.sized_pair(rng, n, m)
        assert ends(q, t, "infix") == S.semiglobal(q, t, "infix"), (n, m)
    q, t = K.sized_pair(rng, n, n)
    assert ends(q, t, "prefix") == S.semiglobal(q, t, "prefix"), n


def test_known_cases_and_empty_sequences():
    assert ends("AAAA", "CCCC", "infix") == (4, 0, 0)
    assert ends("ACG", "ACGACG", "infix") == (0, 3, 0)
    assert ends("GAC", "TTAC", "infix") == (1, 4, 2)
    assert ends("", "ACGT", "infix") == (0, 0, 0) and ends("ACGT", "", "prefix") == (4, 0, 0)
    rng = random.Random(5)
    for _ in range(300):
        q, t = K.bases(rng, rng.randrange(1, 70)), K.bases(rng, rng.randrange(1, 90))
        for mode in ("infix", "prefix"):
            assert ends(q, t, mode) == S.semiglobal(q, t, mode), (q, t, mode)


def test_early_stop_is_within_n_plus_d():
    rng = random.Random(23)
    for _ in range(40):
        n = rng.choice([5, 33, 64, 100])
        q, t, _ = K.planted(rng, n, "end", edits=True)
        d, te = scan(q, t, 0)
        if d < n:                   # (d == n is column 0 of the anchored pass: nothing is scanned)
            assert 0 < scan(q, t[:te], 1, reverse=True, stop_at=d, limit=n + d) <= n + d
