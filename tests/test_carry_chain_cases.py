"""The witness that the low-complexity cases (tests/low_complexity_cases.py) are worth running on the GPU: on the CPU, with
the word-level column model of that file.

For every pair that tests/test_gpu_carry_chains.py gives to a kernel that works on the whole query column -- the bands of
more than 64 words of algorithm="myers", the halves of Hirschberg's parts, the ends scan of infix / prefix:

  * the intact model equals the DP oracle (oracle_aligner.myers_full, oracle_semiglobal.last_row / semiglobal);
  * the model in which no propagating word passes its carry-in on (drop = "all") does not;
  * for each hand-over the pair is meant to reach -- word 63 -> 64 (the carry out of lane 63 into the next round or
    chunk), word 127 -> 128 -- dropping the propagated carry at that word alone changes the answer, and the count shows
    propagated carries crossing it; for the level-by-level kernel and the group kernels, whose chains are cut at a
    segment's or group's last word, the count shows that this word does produce a carry which has to go nowhere.

For Hirschberg "the answer" is first the bottom row of a half, and for the pairs aimed at a chunk hand-over also the
split column taken from the two rows: a dropped carry raises a half's whole row by about one per column, which the split
shrugs off unless the sums are flat around it -- the pairs in question are built so that it moves.

Who is held to "drop changes the answer" follows from what a propagating word is (low_complexity_cases.propagating_words):
a whole query word of bases absent from the target, a word below it that holds a target base, a word above it to receive
the carry. Not held to it are therefore
  * the pairs around the leaf threshold (hirschberg_threshold_pairs, queries of 40 .. 100 bases): a column of fewer than
    three words has no word for a carry to pass through;
  * the edges of the absent-run family: runs of 31, 32 and 33 bases (too short to fill a word at most offsets), runs at
    the query's first or last base (no word below them in one of the two directions), runs that the query's midpoint cuts;
  * unequal homopolymers and tandem repeats: their words generate carries and do not propagate them. They are held to the
    generated carry instead -- cutting the hand-over into the middle word (cut = w) changes the row -- and carry random
    flanks, because inside a run of the target's own base Eq is all ones and Xh with it, whatever the carry. That is
    also why "A" * 2049 against "C" + "A" * 2049 witnesses nothing; it runs on the GPU all the same.

The sliding bands of the banded kernels (one lane, groups of 6 .. 64 lanes, and the sliding stripe of the wide bands) lay
their 32-bit windows over the query at an offset that moves one bit per column, so the model's word layout is not theirs.
For them the cover rule stands in: a run of L bases covers floor((L - 31) / 32) whole words of any window, whatever its
offset, and the query word below the run generates the carry -- checked here on the windows of every offset.

Measured with the seeds below (test_suite_style_pairs_hardly_notice_a_dropped_carry): of 150 pairs of the kind the other
GPU aligner tests draw (uniformly random queries of 33 .. 1 500 bases, targets by random edits), the drop = "all" model
still returns the right edit distance on 148, and no chain of propagating words is longer than one."""
import functools
import random

import pytest

import low_complexity_cases as L
import oracle_aligner as A
import oracle_semiglobal as S


@functools.lru_cache(maxsize=None)
def _row(query, target, top=1, drop=None, cut=None):
    return tuple(L.column_model(query, target, top, drop=drop, cut=cut))


def _dp_row(query, target, free_top_row=False):
    return tuple(int(x) for x in S.last_row(query, target, free_top_row))


def _counted(query, target, top=1):
    c = L.Count()
    L.column_model(query, target, top, count=c)
    return c


# ---- the model itself ------------------------------------------------------------------------------------------------
def test_model_equals_the_oracles_on_random_and_low_complexity_pairs():
    rng = random.Random(1)
    pairs = [L.suite_style_pair(rng) for _ in range(25)] + [L.fuzz_pair(rng) for _ in range(25)]
    pairs += [("A" * 300, "C" * 300), ("A", "A"), ("ACGT" * 20, "ACG")]
    for q, t in pairs:
        assert L.global_distance(q, t) == A.myers_full(q, t)["edit_distance"], (q, t)
        assert _row(q, t) == _dp_row(q, t)
        assert _row(q, t, 0) == _dp_row(q, t, True)
        for mode in ("infix", "prefix"):
            assert L.ends(q, t, mode) == S.semiglobal(q, t, mode), (q, t, mode)


def test_count_and_drop_switches_on_a_case_worked_out_by_hand():
    """96 'A' against one 'C' after a 'C': word 0 generates (its Eq has bit 0, its Pv is all ones), words 1 and 2 hold Eq = 0 and
    Pv all ones. The carry passes through both: two events, a chain of two, one crossing of each boundary."""
    q, t = "C" + "A" * 95, "C"
    c = _counted(q, t)
    assert (c.events, c.longest, c.crossed, c.top_out) == (2, 2, {1: 1}, 1)
    assert L.global_distance(q, t) == 95
    assert L.global_distance(q, t, drop="all") != 95 and L.global_distance(q, t, drop=1) != 95
    assert L.global_distance(q, t, drop=2) == 95      # the last word has nobody to hand it to


def test_cover_rule_on_windows_of_every_offset():
    """A run of L bases covers floor((L - 31) / 32) whole 32-bit words of a window at any offset, and the word below them holds a
    base of the target's alphabet (so that it generates while its Pv is all ones)."""
    rng = random.Random(2)
    for length in L.RUN_LENGTHS + sorted(L.GROUP_RUN_LENGTHS.values()) + [1000, 2010, 2100]:
        q, _ = L.absent_runs(rng, 200, [(70, length)])
        for offset in range(32):
            words = [q[i:i + 32] for i in range(offset, len(q) - 31, 32)]
            whole = [k for k, w in enumerate(words) if w == "A" * 32]
            assert len(whole) >= (length - 31) // 32, (length, offset)
            if whole:
                assert whole == list(range(whole[0], whole[-1] + 1)) and whole[0] > 0
                assert set(words[whole[0] - 1]) & set("CGT")
    for g, length in L.GROUP_RUN_LENGTHS.items():
        assert (length - 31) // 32 == g


def test_suite_style_pairs_hardly_notice_a_dropped_carry():
    rng = random.Random(150)
    survived, longest = 0, 0
    for _ in range(150):
        q, t = L.suite_style_pair(rng)
        want = A.myers_full(q, t)["edit_distance"]
        c = L.Count()
        assert L.column_model(q, t, 1, count=c)[-1] == want
        longest = max(longest, c.longest)
        survived += L.global_distance(q, t, drop="all") == want
    print("drop-everywhere model right on %d of 150 suite-style pairs; longest chain %d" % (survived, longest))
    assert survived >= 140 and longest <= 1     # (the figures of the module docstring: 148, 1)


# ---- bands of more than 64 words -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.wide_band_pairs(), ids=lambda c: c[0])
def test_wide_band_pairs_carry_across_word_63(case):
    name, q, t = case
    want = A.myers_full(q, t)["edit_distance"]
    # the first attempt's band: the length difference + 5 % of the shorter sequence, more than 64 words and less than the query
    dlen = abs(len(q) - len(t))
    estimate = dlen + min(len(q), len(t)) // 20
    assert want <= estimate and 64 * 32 < estimate < len(q)
    c = _counted(q, t)
    assert _row(q, t)[-1] == want
    assert _row(q, t, 1, "all")[-1] != want
    assert _row(q, t, 1, 63)[-1] != want
    assert c.longest >= 64 and c.crossed.get(63, 0) > 0 and c.crossed.get(64, 0) > 0


# ---- Hirschberg's halves ---------------------------------------------------------------------------------------------
_HB = L.hirschberg_short_pairs() + L.hirschberg_long_pairs() + \
    [("neighbour probe " + name, ) + L.neighbour_batch()[0][slots[0]] for name, slots in L.neighbour_batch()[1].items()]


@pytest.mark.parametrize("case", _HB, ids=lambda c: c[0])
def test_hirschberg_pairs_need_their_propagated_carries(case):
    name, q, t = case
    halves = L.hirschberg_halves(q, t)
    for hq, ht in halves:
        assert _row(hq, ht) == _dp_row(hq, ht)
    assert A.hirschberg(q, t)["edit_distance"] == A.myers_full(q, t)["edit_distance"]
    if any(L.propagating_words(hq, ht) for hq, ht in halves):
        assert any(_row(hq, ht, 1, "all") != _row(hq, ht) for hq, ht in halves)
    elif name.split()[-1].startswith(("homopolymer", "tandem")):
        # the generating families: the halves need the carries that their words generate, here the one into the middle word
        assert any(_row(hq, ht, 1, None, len(hq) // 64) != _row(hq, ht) for hq, ht in halves)
    if name in L.HIRSCHBERG_BOUNDARY:
        half, boundary = L.HIRSCHBERG_BOUNDARY[name]
        hq, ht = halves[half]
        assert len(hq) > 65 * 32
        assert _row(hq, ht, 1, boundary) != _row(hq, ht)
        assert _counted(hq, ht).crossed.get(boundary, 0) > 0
        # ... and moves the split, so that the alignment shows it
        rows = [_row(*h) for h in halves]
        broken = list(rows)
        broken[half] = _row(hq, ht, 1, boundary)
        assert L.hirschberg_split(*broken) != L.hirschberg_split(*rows)


def test_most_absent_run_pairs_hold_a_word_that_propagates():
    """The rest are the family's edges: a run too short to fill a word at its offset (31, 32, 33 bases), a run with no word below
    it (at the query's first base; at its last base, which is the first of the reversed half), or one that the split of the
    query cuts in two."""
    runs = [c for c in _HB if c[0].startswith("run") or "half" in c[0] or "absent" in c[0]]
    held = [c[0] for c in runs if any(L.propagating_words(hq, ht) for hq, ht in L.hirschberg_halves(c[1], c[2]))]
    print("%d of %d absent-run pairs hold a propagating word in a half" % (len(held), len(runs)))
    assert len(held) >= 50
    for name in ("run543@", "run287@", "run223@", "run127@", "run96@", "run95@"):
        assert sum(h.startswith(name) for h in held) >= 3, name


def test_segments_and_groups_end_in_words_that_produce_a_carry():
    """The level-by-level kernel stands the two halves of a part side by side and cuts the chain at each half's last word; the
    group kernels cut it at each group's last lane. The neighbour batch's probes make that word produce a carry in many
    columns -- which must not reach the neighbour."""
    pairs, probes = L.neighbour_batch()
    for name, slots in probes.items():
        q, t = pairs[slots[0]]
        for hq, ht in L.hirschberg_halves(q, t):
            assert _counted(hq, ht).top_out > 10, name
    for name, q, t in L.hirschberg_short_pairs():
        if name.startswith("homopolymer"):
            hq, ht = L.hirschberg_halves(q, t)[0]
            assert _counted(hq, ht).top_out > 10, name


def test_neighbour_batch_puts_every_probe_at_every_residue():
    pairs, probes = L.neighbour_batch()
    assert len(pairs) == 126 and all(len(q) + len(t) == L.NEIGHBOUR_TOTAL for q, t in pairs)
    for name, slots in probes.items():
        assert len({pairs[s] for s in slots}) == 1
        for per_wave in (10, 8, 4, 2):          # pairs per wavefront of G = 6, 8, 16, 32
            assert {s % per_wave for s in slots} == set(range(per_wave)), (name, per_wave)
        assert len({(pairs[s - 1], pairs[(s + 1) % len(pairs)]) for s in slots}) > len(slots) // 2   # different neighbours


# ---- the ends scan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.semiglobal_pairs(), ids=lambda c: c[0])
def test_semiglobal_pairs_need_their_propagated_carries(case):
    name, q, t, boundaries, generated = case
    for mode in ("infix", "prefix"):
        top = 1 if mode == "prefix" else 0
        want = S.semiglobal(q, t, mode)
        assert L.ends(q, t, mode) == want, mode
        assert _row(q, t, top) == _dp_row(q, t, mode == "infix")
        c = _counted(q, t, top)
        if generated is None:
            continue
        if not generated:
            assert L.propagating_words(q, t)
            assert _row(q, t, top, "all") != _row(q, t, top), mode
        for b in boundaries:
            assert _row(q, t, top, b) != _row(q, t, top), (mode, b)
            assert c.crossed.get(b, 0) > 0, (mode, b)
            assert L.ends(q, t, mode, drop=b) != want, (mode, b)
        for b in generated:
            assert _row(q, t, top, None, b) != _row(q, t, top), (mode, b)
            assert c.generated[b] > 0, (mode, b)


# ---- the mapper's slices ---------------------------------------------------------------------------------------------
def test_mapper_slices_need_their_propagated_carries():
    queries, targets, rows = L.mapper_reads()
    assert {r[6] for r in rows} == {"+", "-"}
    for qi, ti, qs, qe, ts, te, strand in rows:
        q, t = queries[qi][qs:qe], targets[ti][ts:te]
        t = L.revcomp(t) if strand == "-" else t
        assert "A" * 300 in q and "A" not in t
        halves = L.hirschberg_halves(q, t)
        assert any(L.propagating_words(hq, ht) for hq, ht in halves)
        assert any(_row(hq, ht, 1, "all") != _row(hq, ht) for hq, ht in halves)


# ---- what the GPU tests take for granted -----------------------------------------------------------------------------
def test_banded_oracle_accepts_every_pair_at_both_band_widths():
    BANDED_LONG_WIDTHS = L.BANDED_LONG_WIDTHS
    for pairs, widths in ((L.banded_pairs(), L.BANDED_WIDTHS), (L.banded_long_pairs(), BANDED_LONG_WIDTHS),
                          ([("n",) + p for p in L.neighbour_batch()[0]], (L.NEIGHBOUR_WIDTH,))):
        assert all(300 <= len(q) <= 2400 for _, q, _ in pairs)
        for max_bw in widths:
            for name, q, t in pairs:
                assert A.align(q, t, max_bw)["status"] == 0, (name, max_bw)
    # the long pairs' first band attempt is the 32 / 64 words that the groups of 32 / 64 lanes keep
    for name, q, t in L.banded_long_pairs():
        dlen = len(q) - len(t)
        estimate = dlen + len(t) // 20
        band = 1 + 2 * ((estimate - dlen) // 2) + dlen
        assert A.align(q, t, BANDED_LONG_WIDTHS[0])["edit_distance"] <= estimate, name
        assert (band + 31) // 32 in (32, 64), (name, band)
