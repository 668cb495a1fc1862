"""The window set of tests/test_gpu_pred_rows.py holds the rows it was built for (CPU, the oracle's row hook): the counts its
docstring states, in both phases of the packed forward pass."""
import pred_rows_windows as P

# band 256, over the 24 windows, per phase (band start 0, moved band): rows with 4 / 5 / 6 predecessors all within 7 rows, rows
# with more than six predecessors, rows with a predecessor more than 7 rows up, rows with 4..6 predecessors that lose their
# side-table slot to a later row of the same pass
EXPECTED = {0: {"4": 185, "5": 48, "6": 26, "more_than_6": 39, "far": 156, "lost_slot": 90},
            1: {"4": 340, "5": 167, "6": 59, "more_than_6": 17, "far": 726, "lost_slot": 76}}


FOUR_INSIDE = 15  # windows whose MSA holds all four bases in one column before the last


def test_the_set_holds_the_rows_it_was_built_for():
    windows = P.build_windows()
    assert len(windows) == 24
    for w in windows:
        assert 8 <= len(w) <= 16 and 300 <= len(w[0]) <= 700 and all(0 < len(r) < 1024 for r in w)
    counts, max_row, refs = P.observe_rows(windows)
    print(counts, max_row)
    assert all(r["status"] == 0 for r in refs)
    assert counts == EXPECTED
    for phase in (0, 1):
        assert all(counts[phase][k] >= 10 for k in ("4", "5", "6", "more_than_6", "far", "lost_slot")), counts
    assert max_row > 2 * 256 + 64  # graphs well beyond one turn of the side table
    # a novel stretch of 70-90 bases in one read: more than 64 new nodes at once (the graph outgrows the backbone by more)
    assert all(r["node_count"] >= len(w[0]) + 70 for r, w in zip(refs, windows))


def test_the_set_holds_the_merges_and_sinks_it_was_built_for():
    """From the oracle's MSA: in 15 of the 24 windows a column before the last holds all four bases (reads 3, 4 and 5 each brought
    a new node aligned to a node that had none, one, two aligned nodes before; in the other windows the aligner placed one of the
    three elsewhere), and in every window the backbone and reads 6, 7 and 8 end in one column with four different bases: four
    sinks aligned to each other. Read 8 met three of them, which differ from its last base alike."""
    import oracle_poa as O
    windows = P.build_windows()
    four_inside = 0
    with O.Workspace(P.oracle_config(output_mask=2)) as ws:
        for i, w in enumerate(windows):
            ref = ws.process(w)
            assert ref["status"] == 0
            msa = ref["msa"]
            cols = list(zip(*msa))
            enders = [m.rstrip("-") for m in (msa[0], msa[6], msa[7], msa[8])]
            assert len({len(m) for m in enders}) == 1 and {m[-1] for m in enders} == set("ACGT"), i
            four_inside += any(set(c) >= set("ACGT") for c in cols[:len(enders[0]) - 1])
    print(four_inside)
    assert four_inside == FOUR_INSIDE
