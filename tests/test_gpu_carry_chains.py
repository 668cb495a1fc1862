"""The Myers kernels' carry chains on low-complexity sequences (tests/low_complexity_cases.py): absent-base runs, unequal
homopolymers and tandem repeats through every kernel that writes out the two-ballot carry look-ahead, bit for bit against
the oracle of its class. tests/test_carry_chain_cases.py shows on the CPU that these pairs need their propagated carries,
and which hand-over each one reaches.

  group_advance<G>           test_banded_variants_equal_the_oracle, test_banded_long_runs_reach_the_last_lanes_of_wide_groups,
                             test_banded_result_does_not_depend_on_slot_or_neighbours  (G = 6, 8, 16, 32, 64)
  one lane per pair          the same tests with GWHIP_MYERS_GROUP=0
  multi_advance              test_wide_bands_hand_the_carry_from_round_to_round
  hirschberg_wave_kernel     test_default_aligner_*  (default above 2 048 bases; GWHIP_HIRSCHBERG_LEVELS=0, GWHIP_HIRSCHBERG_SPAN=0)
  hirschberg_myers_kernel    test_default_aligner_*  (GWHIP_HIRSCHBERG_WAVE=0: one lane per pair)
  hirschberg_levels_kernel   test_default_aligner_short_pairs, test_default_aligner_result_does_not_depend_on_neighbours
  hb_span_rows_mw_kernel     test_default_aligner_long_pairs[span]      (GWHIP_HIRSCHBERG_SPAN unset)
  hb_span_rows_kernel        test_default_aligner_long_pairs[span_one_wavefront]  (GWHIP_HIRSCHBERG_SPAN=1)
  round_advance (gws_ends)   test_infix_and_prefix_ends
  the mapper's aligner       test_mapper_aligns_slices_with_absent_runs"""
import functools

import numpy as np
import pytest

import cigar_replay
import low_complexity_cases as L
import oracle_aligner as A

pytestmark = pytest.mark.gpu

CACHE = 4 << 30


def _set(monkeypatch, **env):
    for name in ("GWHIP_MYERS_GROUP", "GWHIP_MYERS_GROUP_LANES", "GWHIP_MYERS_SKIP", "GWHIP_HIRSCHBERG_WAVE",
                 "GWHIP_HIRSCHBERG_LEVELS", "GWHIP_HIRSCHBERG_SPAN"):
        if name in env and env[name] is not None:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)


# ---- banded Myers ----------------------------------------------------------------------------------------------------
BANDED_VARIANTS = [("one_lane", dict(GWHIP_MYERS_GROUP="0")), ("default_choice", dict())] + \
    [("group%d" % g, dict(GWHIP_MYERS_GROUP="1", GWHIP_MYERS_GROUP_LANES=str(g))) for g in (6, 8, 16, 32, 64)]


def _banded(pairs, max_bw):
    from genomeworks_amd import cudaaligner
    al = cudaaligner.CudaAlignerBatch(max_bandwidth=max_bw, max_device_memory_allocator_caching_size=CACHE)
    for q, t in pairs:
        assert al.add_alignment(q, t) == 0
    al.align_all()
    return [(r.status, r.cigar_extended, list(r.alignment), bool(r.is_optimal), r.edit_distance) for r in al.get_alignments()]


@functools.lru_cache(maxsize=None)
def _banded_oracle(which, max_bw):
    cases = {"short": L.banded_pairs, "long": L.banded_long_pairs}[which]()
    out = []
    for name, q, t in cases:
        e = A.align(q, t, max_bw)
        assert e["status"] == 0, (name, max_bw)      # no pair rejected
        states = [op for op, n in e["runs"] for _ in range(n)]
        out.append((0, e["cigar_extended"], states, e["optimal"], e["edit_distance"]))
    return [(q, t) for _, q, t in cases], [c[0] for c in cases], out


def _compare(got, want, names, what):
    assert len(got) == len(want)
    bad = [names[i] for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (what, bad[:10])


@pytest.mark.parametrize("variant", BANDED_VARIANTS, ids=lambda v: v[0])
def test_banded_variants_equal_the_oracle(monkeypatch, variant):
    """Queries of 300 .. 1 200 bases with every run length at every start offset, at two band widths: one lane per pair, the
    default choice and the group kernel forced with 6, 8, 16, 32 and 64 lanes per pair all equal oracle_aligner.align -- and
    with that each other."""
    _set(monkeypatch, **variant[1])
    for max_bw in L.BANDED_WIDTHS:
        pairs, names, want = _banded_oracle("short", max_bw)
        _compare(_banded(pairs, max_bw), want, names, (variant[0], max_bw))


@pytest.mark.parametrize("variant", BANDED_VARIANTS, ids=lambda v: v[0])
def test_banded_long_runs_reach_the_last_lanes_of_wide_groups(monkeypatch, variant):
    """Queries of about 1 300 and 2 300 bases whose first band attempt is 32 resp. 64 words: with 32 / 64 lanes per pair the
    run's chain reaches the group's last lanes; narrower groups hand these bands to their first lane."""
    _set(monkeypatch, **variant[1])
    for max_bw in L.BANDED_LONG_WIDTHS:
        pairs, names, want = _banded_oracle("long", max_bw)
        _compare(_banded(pairs, max_bw), want, names, (variant[0], max_bw))


@functools.lru_cache(maxsize=None)
def _neighbour_oracle():
    pairs, probes = L.neighbour_batch()
    memo = {}
    want = []
    for q, t in pairs:
        if (q, t) not in memo:
            e = A.align(q, t, L.NEIGHBOUR_WIDTH)
            assert e["status"] == 0
            memo[(q, t)] = (0, e["cigar_extended"], [op for op, n in e["runs"] for _ in range(n)], e["optimal"], e["edit_distance"])
        want.append(memo[(q, t)])
    return pairs, probes, want


@pytest.mark.parametrize("variant", BANDED_VARIANTS, ids=lambda v: v[0])
def test_banded_result_does_not_depend_on_slot_or_neighbours(monkeypatch, variant):
    """One batch of pairs of equal total length (so the batch runs in input order): three run-heavy probes -- a band whose top
    word propagates, one whose words all generate, a tandem repeat -- 18 times each, at every residue modulo the 10, 8, 4 and 2
    pairs that a wavefront holds, between random pairs and other run-heavy ones. What protects them is the ~top_mask cut of
    group_advance: a carry out of a group's last lane must not enter the neighbour's first."""
    _set(monkeypatch, **variant[1])
    pairs, probes, want = _neighbour_oracle()
    got = _banded(pairs, L.NEIGHBOUR_WIDTH)
    for name, slots in probes.items():
        assert all(got[s] == got[slots[0]] for s in slots), (variant[0], name)
    _compare(got, want, ["slot %d" % i for i in range(len(pairs))], variant[0])


# ---- bands of more than 64 words -------------------------------------------------------------------------------------
def test_wide_bands_hand_the_carry_from_round_to_round(monkeypatch):
    """algorithm="myers", 4 400 against 2 300 bases with a run of 2 100: the band of the first attempt is 70 words, two rounds of
    multi_advance, and the run's chain spans words 63 and 64 -- the carry out of lane 63 and the top bits of ph / mh go from
    round to round. Against the full-matrix oracle, and against the one-lane stripes (GWHIP_MYERS_SKIP=8)."""
    from genomeworks_amd import cudaaligner
    cases = L.wide_band_pairs()
    max_len = 4608

    def run():
        al = cudaaligner.CudaAlignerBatch(max_len, max_len, len(cases), algorithm="myers", max_device_memory_allocator_caching_size=16 << 30)
        for _, q, t in cases:
            assert al.add_alignment(q, t) == 0
        al.align_all()
        return [(r.status, bool(r.is_optimal), list(r.alignment), r.cigar_extended, r.edit_distance) for r in al.get_alignments()]

    _set(monkeypatch)
    got = run()
    for (name, q, t), (st, opt, states, cigar, dist) in zip(cases, got):
        ref = A.myers_full(q, t)
        assert (st, opt) == (0, True), name
        assert states == ref["states"], name
        assert (cigar, dist) == (ref["cigar_extended"], ref["edit_distance"]), name
    _set(monkeypatch, GWHIP_MYERS_SKIP="8")
    assert run() == got


# ---- the default aligner (Hirschberg + Myers) ------------------------------------------------------------------------
def _default(pairs, max_len):
    from genomeworks_amd import cudaaligner
    al = cudaaligner.CudaAlignerBatch(max_len, max_len, len(pairs), max_device_memory_allocator_caching_size=8 << 30)
    for q, t in pairs:
        assert al.add_alignment(q, t) == 0, (len(q), len(t))
    al.align_all()
    return [(r.status, list(r.alignment), r.cigar_extended, bool(r.is_optimal), r.edit_distance) for r in al.get_alignments()]


@functools.lru_cache(maxsize=None)
def _default_oracle(which, max_len):
    cases = {"threshold": L.hirschberg_threshold_pairs, "short": L.hirschberg_short_pairs, "long": L.hirschberg_long_pairs}[which]()
    want = []
    for name, q, t in cases:
        e = A.hirschberg(q, t, max_len)
        assert e["status"] == 0
        assert e["edit_distance"] == A.myers_full(q, t)["edit_distance"], name   # the oracle's own path is optimal
        want.append((0, e["states"], e["cigar_extended"], True, e["edit_distance"]))
    return [(q, t) for _, q, t in cases], [c[0] for c in cases], want


SHORT_VARIANTS = [("levels", dict()), ("depth_first_wave", dict(GWHIP_HIRSCHBERG_LEVELS="0")), ("one_lane", dict(GWHIP_HIRSCHBERG_WAVE="0"))]
LONG_VARIANTS = [("span", dict()), ("span_off", dict(GWHIP_HIRSCHBERG_SPAN="0")), ("span_one_wavefront", dict(GWHIP_HIRSCHBERG_SPAN="1")),
                 ("one_lane", dict(GWHIP_HIRSCHBERG_WAVE="0"))]


@pytest.mark.parametrize("variant", SHORT_VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("which,max_len", [("threshold", 128), ("short", 2048)])
def test_default_aligner_short_pairs(monkeypatch, variant, which, max_len):
    """Queries of up to 2 048 bases -- around the leaf threshold (63), and the three families at 300 .. 2 048 bases -- through the
    level-by-level kernel, the depth-first wavefront kernel alone (GWHIP_HIRSCHBERG_LEVELS=0) and the one-lane kernel
    (GWHIP_HIRSCHBERG_WAVE=0): the states, CIGAR and distance of the Hirschberg oracle, whose distance is myers_full's."""
    _set(monkeypatch, **variant[1])
    pairs, names, want = _default_oracle(which, max_len)
    _compare(_default(pairs, max_len), want, names, variant[0])


@pytest.mark.parametrize("variant", LONG_VARIANTS, ids=lambda v: v[0])
def test_default_aligner_long_pairs(monkeypatch, variant):
    """Queries of 2 049 .. 4 400 bases in a batch small enough for the span path: the span path (its rows by one wavefront per
    64-word chunk, hb_span_rows_mw_kernel, the chunk carries travelling between wavefronts), off (the depth-first
    hirschberg_wave_kernel alone, parts in 64-word chunks) and in its one-wavefront form (hb_span_rows_kernel), and the
    one-lane kernel. Two queries put a run across word 64 of the forward half resp. of the reversed second half."""
    _set(monkeypatch, **variant[1])
    pairs, names, want = _default_oracle("long", 4608)
    _compare(_default(pairs, 4608), want, names, variant[0])


@pytest.mark.parametrize("variant", SHORT_VARIANTS[:2], ids=lambda v: v[0])
def test_default_aligner_result_does_not_depend_on_neighbours(monkeypatch, variant):
    """The neighbour batch through the default aligner: hirschberg_levels_kernel stands the segments of a level side by side in
    one wavefront and cuts the chain at every segment's last lane; the probes' segments end in words that produce a carry."""
    _set(monkeypatch, **variant[1])
    pairs, probes = L.neighbour_batch()
    got = _default(pairs, 2048)
    for name, slots in probes.items():
        q, t = pairs[slots[0]]
        e = A.hirschberg(q, t, 2048)
        want = (0, e["states"], e["cigar_extended"], True, e["edit_distance"])
        assert e["edit_distance"] == A.myers_full(q, t)["edit_distance"]
        assert all(got[s] == want for s in slots), (variant[0], name)
    for k in (1, 3, 8, 15):      # and a few of the pairs between them
        e = A.hirschberg(*pairs[k], 2048)
        assert got[k][:2] == (0, e["states"])


# ---- infix / prefix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["infix", "prefix"])
def test_infix_and_prefix_ends(mode):
    """The ends scan (round_advance, gws_ends.hip): queries of 2 047, 2 048, 2 049 and 4 100 bases with runs across word 64 and
    word 128, "A" * 2049 against "C" + "A" * 2049 and its prefix twin, and one query of 16 400 bases (the workspace variant)
    -- each held to the three conditions of test_gpu_semiglobal._check: the DP oracle's (d, begin, end), the states of a
    global batch on the slice, and the CIGAR's replay."""
    from test_gpu_semiglobal import _check
    cases = L.semiglobal_pairs()
    small = [(q, t) for _, q, t, _, _ in cases if len(q) <= 16384]
    large = [(q, t) for _, q, t, _, _ in cases if len(q) > 16384]
    assert len(large) == 1
    _check(small, mode)
    _check(large, mode)


# ---- the mapper ------------------------------------------------------------------------------------------------------
def test_mapper_aligns_slices_with_absent_runs():
    """One call of cudamapper.align_overlaps over two hand-built overlaps, one per strand, whose query slices carry a 300-base
    absent run: the CIGARs and distances of oracle_mapper_align.alignments, which replay on the reads at the optimal cost."""
    import oracle_mapper as O
    import oracle_mapper_align as OA
    from genomeworks_amd import cudamapper as cm
    queries, targets, rows = L.mapper_reads()
    o = np.zeros(len(rows), O.OVERLAP)
    for r, (qi, ti, qs, qe, ts, te, strand) in zip(o, rows):
        r["query_read_id"], r["target_read_id"] = qi, ti
        r["query_start_position_in_read"], r["query_end_position_in_read"] = qs, qe
        r["target_start_position_in_read"], r["target_end_position_in_read"] = ts, te
        r["relative_strand"], r["num_residues"] = ord(strand), 10
    ref = OA.alignments(o, queries, targets)
    cigars, edits = cm.align_overlaps(o, queries, targets)
    assert all(a["status"] == 0 for a in ref)
    assert cigars == [a["cigar"] for a in ref]
    assert edits.tolist() == [a["edit_distance"] for a in ref]
    for k, ((qi, ti, qs, qe, ts, te, strand), cigar, a) in enumerate(zip(rows, cigars, ref)):
        record = ["q", str(len(queries[qi])), str(qs), str(qe), strand, "t", str(len(targets[ti])), str(ts), str(te), "0", "0", "0",
                  "cg:Z:" + cigar]
        replay = cigar_replay.replay_paf(record, {"q": queries[qi]}, {"t": targets[ti]})
        q, t = OA.slices(o[k], queries, targets)
        assert replay.edits == a["edit_distance"] == A.myers_full(q, t)["edit_distance"]
