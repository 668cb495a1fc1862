"""The window set of tests/test_gpu_pred_rows.py and what the oracle's rows hold on it (no GPU needed; not a test module).

Every window is a random backbone and reads that differ from it by DELETIONS ONLY in its first part, so that the graph stays a
line there and a backbone position is a DP row: a hub is a position that several reads reach by deletions of different lengths
ending right before it -- its node collects one in-edge per length, from 2 .. length + 1 rows up. Hubs come in pairs 256 rows
apart (two rows of one read's pass that want the same slot of the side table of predecessors 3..5: the lower one loses it), early
in the window (band start 0) and late (moved band), with 3..5 lengths (4..6 predecessors within 7 rows), 7..9 lengths (more than
six predecessors) and one long deletion (a predecessor more than 7 rows up). Behind the last hub the reads carry what the merge
and the sink selection are to see: a novel stretch of 70-90 bases in one read (more than 64 new nodes at once), one position
where three reads in turn bring a third, a fourth base (a new node aligned to a node that already has one, two aligned nodes),
and ragged ends -- reads cut short, and two reads that end in different bases the next reads mismatch alike (several sinks, and
two of them tie)."""
import ctypes as C
import random

import oracle_poa as O

WINDOWS = 24
SEED = 4711


def build_windows():
    rng = random.Random(SEED)
    out = []
    for k in range(WINDOWS):
        length = rng.randrange(560, 700) if k % 3 else rng.randrange(300, 420)
        reads_n = rng.randrange(10, 17)
        backbone = "".join(rng.choice("ACGT") for _ in range(length))
        # hubs: (position, deletion lengths that end right before it)
        hubs = []
        firsts = [rng.randrange(30, 50), rng.randrange(70, 90), rng.randrange(180, 200), rng.randrange(215, 235)] if length >= 560 else \
                 [rng.randrange(30, 50), rng.randrange(70, 90)]
        for n, h in enumerate(firsts):
            many = (n + k) % 4 == 3
            lens = list(range(1, rng.randrange(8, 11))) if many else list(range(1, rng.randrange(4, 7)))
            if (n + k) % 4 == 1:
                lens[-1] = rng.randrange(9, 14)  # one predecessor more than 7 rows up
            hubs.append((h, lens))
            if h + 256 < length - 110:
                hubs.append((h + 256, list(range(1, rng.randrange(4, 7)))))
        tail = max(h for h, _ in hubs) + 12  # free play behind the last hub
        sub_at = rng.randrange(tail, tail + 20)
        reads = [backbone]
        for r in range(1, reads_n):
            s = list(backbone)
            for h, lens in hubs:
                d = lens[(r - 1) % (len(lens) + 1)] if (r - 1) % (len(lens) + 1) < len(lens) else 0
                for x in range(h - d, h):
                    s[x] = ""
            if r == 2:  # a novel stretch: more than 64 new nodes in one read
                at = rng.randrange(tail + 25, tail + 40)
                s[at] = s[at] + "".join(rng.choice("ACGT") for _ in range(rng.randrange(70, 91)))
            if r in (3, 4, 5):  # a second, third, fourth base at one position
                s[sub_at] = [b for b in "ACGT" if b != backbone[sub_at]][r - 3]
            t = "".join(s)
            if r in (6, 7):  # two ends in different bases ...
                t = t[:-1] + [b for b in "ACGT" if b != backbone[-1]][r - 6]
            elif r == 8:     # ... that the next read mismatches alike
                t = t[:-1] + [b for b in "ACGT" if b != backbone[-1]][2]
            elif r % 4 == 1:
                t = t[:len(t) - rng.randrange(1, 9)]
            reads.append(t)
        out.append(reads)
    return out


def oracle_config(band_mode="static_band", band_width=256, output_mask=1):
    from test_gpu_poa import oracle_cfg
    return oracle_cfg(band_mode, band_width=band_width, output_mask=output_mask)


_HOOK_T = C.CFUNCTYPE(None, C.c_int32, C.c_int32, C.c_int32, C.c_int32)


def observe_rows(windows):
    """The oracle's banded forward passes at band 256 over the set, through its row hook: per phase (band start 0, moved band) the
    number of rows with 4, 5, 6 predecessors all within 7 rows, with more than six predecessors, with a predecessor more than 7
    rows up, and with 4..6 predecessors whose side-table slot (row & 255) a later row of the same pass with more than three
    predecessors takes; and the largest row seen."""
    counts = {ph: {"4": 0, "5": 0, "6": 0, "more_than_6": 0, "far": 0, "lost_slot": 0} for ph in (0, 1)}
    state = {"pass": [], "max_row": 0}

    def close_pass():
        rows = state["pass"]
        last_writer = {}
        for row, cnt, _, _ in rows:
            if cnt > 3:
                last_writer[row & 255] = row
        for row, cnt, far, bs in rows:
            if 4 <= cnt <= 6 and last_writer[row & 255] != row:
                counts[1 if bs > 0 else 0]["lost_slot"] += 1
        state["pass"] = []

    def hook(row, cnt, far, bs):
        if row == 1 and state["pass"]:
            close_pass()
        state["pass"].append((row, cnt, far, bs))
        state["max_row"] = max(state["max_row"], row)
        c = counts[1 if bs > 0 else 0]
        if 4 <= cnt <= 6 and far <= 7:
            c[str(cnt)] += 1
        if cnt > 6:
            c["more_than_6"] += 1
        if cnt >= 1 and far > 7:
            c["far"] += 1

    cb = _HOOK_T(hook)
    slot = C.c_void_p.in_dll(O.lib(), "poa_oracle_row_hook")
    slot.value = C.cast(cb, C.c_void_p).value
    try:
        refs = []
        with O.Workspace(oracle_config()) as ws:
            for w in windows:
                refs.append(ws.process(w))
        if state["pass"]:
            close_pass()
    finally:
        slot.value = None
    return counts, state["max_row"], refs
