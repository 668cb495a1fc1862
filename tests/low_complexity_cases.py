"""Seeded low-complexity inputs for the Myers kernels' carry chains, and a word-level model of one column step that can
count and drop propagated carries. TEST INFRASTRUCTURE ONLY (no GPU).

Every bit-vector aligner of the project computes Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq as one multi-word addition. A word
passes a carry on only when its Pv is all ones and its Eq is zero: 32 consecutive query bases that all differ from the
current target base and all lie below the alignment's diagonal. Uniformly random queries never give two such words in
a row; the three families below do.

  * Absent-base runs: a target over {C, G, T}; the query is that target (optionally with about 2 % edits drawn from
    C, G, T) with runs of 'A' inserted. A run of L bases covers floor((L - 31) / 32) whole words of ANY 32-bit window
    laid over the query, whatever the window's offset (the cover rule) -- which is what makes the family work for the
    sliding bands too, whose windows move one bit per column. The query word just below the run has Eq != 0 while its
    Pv is still all ones, so it generates the carry that the run's words pass on.
  * Unequal homopolymers: a run of one base in both sequences, 1 to 70 bases apart in length. Every word generates, none
    propagates -- and inside the run itself Eq is all ones, which makes Xh all ones whatever the carry: it is the flanks'
    words, meeting the run's base, that need the generated carries. The cases therefore carry random flanks.
  * Tandem repeats: periods 2 to 6 with different copy numbers in query and target.

The model (column_model) restates a column step as the kernels do it -- each word's own sum, gen ("my addition
overflowed") and prp ("my sum is all ones"), and a ripple for the carries -- on the whole query column, word w = query
bases 32 w .. 32 w + 31. The kernels' layouts (64 words per round or chunk, groups, segments) cut that column into pieces;
"boundary w" below is the hand-over of the carry out of word w into word w + 1."""
import random

import numpy as np

WORD = 32
M32 = np.uint32(0xFFFFFFFF)

RUN_LENGTHS = [31, 32, 33, 63, 64, 65, 95, 96, 127]            # straddle the word boundary
GROUP_RUN_LENGTHS = {6: 223, 8: 287, 16: 543}                  # 32 (G + 1) - 1: a whole group plus one word
START_OFFSETS = [0, 1, 31, 32, 33]                             # bit offsets of a run's first base in its word

_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


# ---- the families -----------------------------------------------------------------------------------------------------
def draw(rng, alphabet, n):
    return "".join(rng.choice(alphabet) for _ in range(n))


def edited(rng, s, rate, alphabet):
    """About rate * len(s) unit edits with bases of `alphabet` (none when rate is 0)."""
    out = list(s)
    for _ in range(int(len(s) * rate)):
        kind, at = rng.randrange(3), rng.randrange(len(out))
        if kind == 0:
            out[at] = rng.choice([b for b in alphabet if b != out[at]])
        elif kind == 1:
            out.insert(at, rng.choice(alphabet))
        elif len(out) > 1:
            del out[at]
    return "".join(out)


def absent_runs(rng, target_len, runs, edits=False, run_base="A", query_len=None):
    """(query, target): a target of target_len bases over the other three letters, and the query = that target (with 2 %
    edits of the same letters when `edits`) with runs of `run_base` inserted. `runs` = [(start, length), ...] in query
    coordinates, ascending; start "end" puts the run behind the query's last base. query_len, if given, is the query's
    exact length: the edited copy is cut or extended at its end by the few bases the edits moved it."""
    alphabet = "".join(b for b in "ACGT" if b != run_base)
    target = draw(rng, alphabet, target_len)
    base = edited(rng, target, 0.02, alphabet) if edits else target
    if query_len is not None:
        want = query_len - sum(length for _, length in runs)
        base = (base + draw(rng, alphabet, max(0, want - len(base))))[:want]
    out, used, cur = [], 0, 0
    for start, length in runs:
        take = len(base) - used if start == "end" else start - cur
        assert 0 <= take <= len(base) - used, (start, length, len(base))
        out.append(base[used:used + take])
        out.append(run_base * length)
        used, cur = used + take, cur + take + length
    out.append(base[used:])
    return "".join(out), target


def unequal_homopolymers(rng, n_query, n_target, flank=0, base="A"):
    """(query, target): `base` n_query / n_target times between the same random flanks."""
    left, right = draw(rng, "ACGT", flank), draw(rng, "ACGT", flank)
    return left + base * n_query + right, left + base * n_target + right


def tandem_repeats(rng, period, copies_query, copies_target, flank=0):
    """(query, target): a random unit of `period` bases (not a shorter repeat), copied a different number of times."""
    while True:
        unit = draw(rng, "ACGT", period)
        if all(unit != unit[:d] * (period // d) for d in range(1, period) if period % d == 0):
            break
    left, right = draw(rng, "ACGT", flank), draw(rng, "ACGT", flank)
    return left + unit * copies_query + right, left + unit * copies_target + right


def suite_style_pair(rng):
    """A pair of the kind the other GPU aligner tests draw: a uniformly random query of 33 .. 1 500 bases, the target by
    random unit edits at the suite's rates."""
    n = rng.choice([33, 64, 65, 100, 150, 255, 300, 400, 512, 777, 1000, 1500])
    q = draw(rng, "ACGT", n)
    t = list(q)
    for _ in range(rng.choice([0, 1, 3, n // 25 + 1, n // 8 + 1, n // 6 + 1])):
        op, p = rng.random(), rng.randrange(max(1, len(t)))
        if op < 0.4 and t:
            t[p] = rng.choice("ACGT")
        elif op < 0.7:
            t.insert(p, rng.choice("ACGT"))
        elif len(t) > 1:
            del t[p]
    return q, "".join(t)


# ---- the model --------------------------------------------------------------------------------------------------------
class Count:
    """What column_model saw: `events` = (column, word) pairs where a carry-in of 1 met a propagating word, `longest` = the
    longest chain of consecutive such words in one column, `crossed[w]` = propagated carries handed from word w to word
    w + 1, `top_out` = columns in which the column's last word produced a carry (generated or propagated) that no word takes."""

    def __init__(self):
        self.events, self.longest, self.crossed, self.top_out = 0, 0, {}, 0
        self.generated = None     # generated[w] = carries that word w generated itself (handed to word w + 1, if there is one)


def propagating_words(query, target):
    """Query words (32 bases from a multiple of 32) that can pass a carry on in some column: none of their bases occurs in the
    target, a lower word holds a base that does (that word generates while its Pv is all ones, as in column 1), and a
    higher word is there to receive it."""
    seen = {"ACTG"[(ord(c) >> 1) & 3] for c in target}
    out, below = [], False
    for w in range(0, len(query) - WORD + 1, WORD):
        word = query[w:w + WORD]
        if below and not set(word) & seen and w + WORD < len(query):
            out.append(w // WORD)
        below = below or bool(set(word) & seen)
    return out


def pattern_words(query):
    """eq[c][w] for c the index of "ACTG" (the kernels' (char >> 1) & 3): bit b = (query[32 w + b] == "ACTG"[c])."""
    n_words = max(1, (len(query) + WORD - 1) // WORD)
    eq = np.zeros((4, n_words), np.uint32)
    for i, ch in enumerate(query):
        c = "ACTG".find(ch)
        if c >= 0:
            eq[c, i // WORD] |= np.uint32(1 << (i % WORD))
    return eq


def column_model(query, target, top=1, drop=None, count=None, cut=None):
    """The bottom row D[n][0 .. m] of query against target, column by column over the query's words. `top` is the bit
    shifted into word 0 (1: global / prefix, 0: infix). drop = None, "all" (no propagating word passes its carry-in on) or
    a word index w (word w does not). cut = a word index w: word w + 1 receives no carry at all, generated or propagated (a
    chain cut in the wrong place, or a hand-over lost altogether). count = a Count to fill in."""
    n = len(query)
    assert n > 0
    eq = pattern_words(query)
    n_words = eq.shape[1]
    pv = np.full(n_words, M32, np.uint32)
    mv = np.zeros(n_words, np.uint32)
    cin = np.zeros(n_words, np.uint32)
    lo = np.zeros(n_words, np.uint32)
    one, s31 = np.uint32(1), np.uint32(31)
    own_w, own_b = (n - 1) // WORD, np.uint32((n - 1) % WORD)
    score = n
    row = [score]
    for ch in target:
        e = eq[(ord(ch) >> 1) & 3]
        xv = e | mv
        a = e & pv
        s0 = a + pv                                   # uint32: wraps
        gen = s0 < a
        prp = s0 == M32
        cin[0] = 0
        cin[1:] = gen[:-1]
        if cut is not None and cut + 1 < n_words:
            cin[cut + 1] = 0
        if count is not None:
            count.generated = gen.astype(np.int64) if count.generated is None else count.generated + gen
        chain, prev = 0, -2
        for w in np.flatnonzero(prp).tolist():        # the ripple: only a propagating word can hand on what it received
            if not cin[w]:
                continue
            passes = not (drop == "all" or drop == w or cut == w)
            if count is not None:
                count.events += 1
                chain = chain + 1 if w == prev + 1 else 1
                count.longest = max(count.longest, chain)
                if passes and w + 1 < n_words:
                    count.crossed[w] = count.crossed.get(w, 0) + 1
            prev = w if passes else -2
            if passes and w + 1 < n_words:
                cin[w + 1] = 1
        if count is not None and (gen[-1] or (prp[-1] and cin[-1])):
            count.top_out += 1
        total = s0 + cin
        xh = (total ^ pv) | e
        ph = mv | ~(xh | pv)
        mh = pv & xh
        score += int((ph[own_w] >> own_b) & one) - int((mh[own_w] >> own_b) & one)
        row.append(score)
        lo[0] = top
        lo[1:] = ph[:-1] >> s31
        phs = (ph << one) | lo
        lo[0] = 0
        lo[1:] = mh[:-1] >> s31
        mhs = (mh << one) | lo
        pv = mhs | ~(xv | phs)
        mv = phs & xv
    return row


def global_distance(query, target, **kw):
    return column_model(query, target, 1, **kw)[-1]


def ends(query, target, mode, **kw):
    """(d, te, tb) as the ends scan computes them (the scan model of tests/test_semiglobal_scan_model.py on column_model):
    forward pass, then for infix the anchored pass over both sequences reversed, within n + d columns."""
    n = len(query)
    if n == 0 or not target:
        return n, 0, 0
    row = column_model(query, target, 1 if mode == "prefix" else 0, **kw)
    d = min(row)
    te = row.index(d)
    if mode == "prefix":
        return d, te, 0
    if d == n:
        return d, te, te
    back = column_model(query[::-1], target[:te][::-1][:n + d], 1, **kw)
    return d, te, (te - back.index(d)) if d in back else -1


def hirschberg_halves(query, target):
    """The two full-column problems at the top of Hirschberg's tree: (forward half, target) and (second half reversed,
    target reversed). Deeper parts are the same computation on slices."""
    mid = len(query) // 2
    return (query[:mid], target), (query[mid:][::-1], target[::-1])


# ---- the cases --------------------------------------------------------------------------------------------------------
# Every function returns a list of (name, query, target); the names appear in assertion messages.

def banded_pairs():
    """Banded Myers, groups of 6 / 8 / 16 lanes: queries of 300 .. 1 200 bases. Every run length at every start offset (the
    run starts at word 4 + that offset, clear of the diagonal's first words), a run at the first base, one ending at the
    last base, two runs in one query; unequal homopolymers; tandem repeats. The length difference is at most 543 + edits."""
    rng = random.Random(20260101)
    out = []
    for k, length in enumerate(RUN_LENGTHS + sorted(GROUP_RUN_LENGTHS.values())):
        for j, off in enumerate(START_OFFSETS):
            t_len = rng.choice([300, 333, 450, 600])
            start = 4 * WORD + off + WORD * ((k + j) % 3)
            q, t = absent_runs(rng, t_len, [(start, length)], edits=(k + j) % 2 == 1)
            out.append(("run%d@%d%s" % (length, start, "+edits" if (k + j) % 2 else ""), q, t))
    for length in (33, 96, 287):
        q, t = absent_runs(rng, 400, [(0, length)])
        out.append(("run%d@first" % length, q, t))
        q, t = absent_runs(rng, 400, [("end", length)])
        out.append(("run%d@last" % length, q, t))
    for a, b in ((64, 127), (96, 65), (223, 33)):
        q, t = absent_runs(rng, 500, [(100, a), (100 + a + 161, b)], edits=True)
        out.append(("runs%d+%d" % (a, b), q, t))
    for nq, nt, flank in ((300, 301, 33), (330, 300, 40), (300, 370, 17), (700, 633, 100), (1000, 1070, 25), (64, 97, 150)):
        out.append(("homopolymer%dv%d" % (nq, nt),) + unequal_homopolymers(rng, nq, nt, flank, rng.choice("ACGT")))
    for period, cq, ct, flank in ((2, 200, 230, 0), (2, 310, 300, 33), (3, 150, 171, 10), (4, 100, 90, 64), (5, 130, 150, 0),
                                  (6, 160, 131, 31), (3, 400, 380, 0)):
        out.append(("tandem%dx%dv%d" % (period, cq, ct),) + tandem_repeats(rng, period, cq, ct, flank))
    return out


def banded_long_pairs():
    """Banded Myers, groups of 32 / 64 lanes: a short target (300 bases) and a run of about 1 000 or 2 010 bases, so that the
    first band attempt (length difference + 5 % of the shorter sequence) is 32 resp. 64 words wide, the group keeps it, and
    the run reaches the band's last words while the window slides past it."""
    rng = random.Random(20260102)
    out = []
    for length, start, edits in ((1000, 150, False), (995, 129, True), (2010, 150, False), (2005, 97, True), (2010, "end", False)):
        q, t = absent_runs(rng, 300, [(start, length)], edits=edits)
        out.append(("run%d@%s%s" % (length, start, "+edits" if edits else ""), q, t))
    return out


NEIGHBOUR_TOTAL = 1400   # query + target length of every pair of the neighbour batch
# max_bandwidth of the banded batches: every pair's length difference is below each (checked against the oracle on the CPU)
BANDED_WIDTHS = (2048, 600)
BANDED_LONG_WIDTHS = (4096, 2100)
NEIGHBOUR_WIDTH = 1024


def _fixed_total(q, t, total, rng, alphabet):
    """The pair with its target cut or extended at the end so that the two lengths add up to `total` (the banded aligner runs
    a batch longest pair first, in a stable order: equal totals keep the input order, slot = index)."""
    want = total - len(q)
    assert want > 0
    return q, (t + draw(rng, alphabet, max(0, want - len(t))))[:want]


def neighbour_batch():
    """(pairs, probes): 126 pairs of equal total length. probes = {name: [slots]}: three run-heavy pairs -- one whose band's
    top word propagates (an absent run of 543 bases), one whose words all generate (unequal homopolymers), one tandem
    repeat -- each 18 times, between plain random pairs and further run-heavy ones, which are shuffled once with a fixed seed.
    A group kernel puts 10, 8, 4, 2 or 1 pairs side by side in a wavefront; the probes' slots cover every residue of each."""
    rng = random.Random(20260103)
    cgt = "CGT"
    probe_pairs = {
        "absent543": _fixed_total(*absent_runs(rng, 260, [(130, 543)]), NEIGHBOUR_TOTAL, rng, cgt),
        "homopolymer": _fixed_total(*unequal_homopolymers(rng, 700, 650, 20, "G"), NEIGHBOUR_TOTAL, rng, "ACGT"),
        "tandem2": _fixed_total(*tandem_repeats(rng, 2, 360, 330, 5), NEIGHBOUR_TOTAL, rng, "ACGT"),
    }
    fillers = []
    for k in range(72):
        if k % 2 == 0:
            q = draw(rng, "ACGT", rng.choice([600, 690, 700, 733]))
            q, t = _fixed_total(q, edited(rng, q, 0.05, "ACGT"), NEIGHBOUR_TOTAL, rng, "ACGT")
        else:
            length = rng.choice([65, 127, 223, 287])
            q, t = _fixed_total(*absent_runs(rng, rng.choice([560, 600]), [(rng.randrange(64, 300), length)], edits=True),
                                NEIGHBOUR_TOTAL, rng, cgt)
        fillers.append(("filler%d" % k, q, t))
    rng.shuffle(fillers)
    # slots 7 k, 7 k + 2, 7 k + 4 hold the probes: 7 is prime to 10 and to 8, so 18 copies meet every residue; the shuffled
    # fillers stand between them
    names = list(probe_pairs)
    slots = [(names[(i % 7) // 2],) + probe_pairs[names[(i % 7) // 2]] if i % 7 in (0, 2, 4) else fillers.pop() for i in range(126)]
    probes = {name: [i for i, s in enumerate(slots) if s[0] == name] for name in probe_pairs}
    return [(q, t) for _, q, t in slots], probes


def wide_band_pairs():
    """algorithm="myers" with a band of more than 64 words: queries of about 4 400 bases against targets of 2 300 with a run
    of about 2 100 'A' from query word 21 .. 23 on. The length difference makes the first attempt's band 70 words (the run
    + 5 % of the target); the run covers 64 whole words of any window, and query words 63 and 64 for every column that lies
    left of the run."""
    rng = random.Random(20260104)
    out = []
    for length, start, edits in ((2100, 21 * WORD, False), (2111, 23 * WORD + 17, True)):
        q, t = absent_runs(rng, 2300, [(start, length)], edits=edits)
        out.append(("run%d@%d%s" % (length, start, "+edits" if edits else ""), q, t))
    return out


def hirschberg_threshold_pairs():
    """The default aligner around kHbSwitchToMyers (63): the three families at query lengths 40 .. 100. A part of fewer than
    63 query bases is a leaf (one lane, word after word: no look-ahead), and no carry passes through a column of fewer than
    three words -- these pairs choose the kernels' paths, the witnessed pairs below carry the chains."""
    rng = random.Random(20260105)
    out = []
    for n, length in ((60, 31), (62, 32), (63, 33), (64, 33), (66, 32), (100, 65)):
        q, t = absent_runs(rng, n - length, [(rng.choice([0, 1, 5]), length)])
        out.append(("run%d in %d" % (length, n), q, t))
    for nq, nt in ((40, 41), (62, 64), (63, 70), (64, 62), (70, 100), (97, 33)):
        out.append(("homopolymer%dv%d" % (nq, nt),) + unequal_homopolymers(rng, nq, nt, 0, rng.choice("ACGT")))
    for period, cq, ct in ((2, 31, 33), (3, 21, 25), (5, 13, 11), (6, 11, 16)):
        out.append(("tandem%dx%dv%d" % (period, cq, ct),) + tandem_repeats(rng, period, cq, ct))
    return out


def hirschberg_short_pairs():
    """The default aligner, queries and targets of up to 2 048 bases (the level-by-level kernel's range): the banded pairs
    (300 .. 1 200 bases), and the families at query lengths 2 040 .. 2 048."""
    rng = random.Random(20260106)
    out = banded_pairs()
    for n, length, start in ((2047, 127, 900), (2048, 287, 31), (2048, 96, "end"), (2040, 543, 1000)):
        q, t = absent_runs(rng, n - length, [(start, length)], edits=True, query_len=n)
        out.append(("run%d in %d" % (length, len(q)), q, t))
    out.append(("homopolymer1990v1920",) + unequal_homopolymers(rng, 1990, 1920, 29, "C"))
    out.append(("homopolymer1900v1933",) + unequal_homopolymers(rng, 1900, 1933, 57, "T"))
    out.append(("tandem2x1024v1000",) + tandem_repeats(rng, 2, 1024, 1000))
    out.append(("tandem6x340v333",) + tandem_repeats(rng, 6, 340, 333, 3))
    return out


def hirschberg_long_pairs():
    """The default aligner beyond 2 048 bases (the depth-first kernel alone, or the span path on top of it): the families at
    2 049 .. 2 600 bases, and four queries of 4 400 bases and more whose halves are 69 words and more -- two chunks of 64 -- with
    a run across word 64 of the forward half resp. (the same construction, both sequences reversed) of the reversed second half.
    A dropped carry raises the whole bottom row of such a half by about one per column, and Hirschberg's split, the column of
    the smallest sum, shrugs that off where the sums fall by two per column towards it; the targets of these four are
    therefore unrelated to the query beyond their first 500 bases, or end after 1 000, which flattens the sums -- there the
    split moves (hirschberg_split; tests/test_carry_chain_cases.py) and the alignment with it."""
    rng = random.Random(20260107)
    out = []
    for n, length, start in ((2049, 127, 1000), (2050, 96, 0), (2300, 543, 1200), (2600, 287, "end")):
        q, t = absent_runs(rng, n - length, [(start, length)], edits=True, query_len=n)
        out.append(("run%d in %d" % (length, len(q)), q, t))
    out.append(("homopolymer2049v2100",) + unequal_homopolymers(rng, 2049, 2100, 21, "G"))
    out.append(("homopolymer2500v2430",) + unequal_homopolymers(rng, 2500, 2430, 40, "A"))
    out.append(("tandem3x700v720",) + tandem_repeats(rng, 3, 700, 720))
    out.append(("tandem5x500v470",) + tandem_repeats(rng, 5, 500, 470, 9))
    for k, kind in enumerate(("unrelated tail", "short target")):
        q, t = absent_runs(rng, 4200, [(1950 + 50 * k, 200 + 60 * k)], edits=True, query_len=4400 + 60 * k)
        t = t[:500] + draw(rng, "CGT", 3000) if kind == "unrelated tail" else t[:1000]
        out.append(("forward half word 64, " + kind, q, t))
        q, t = absent_runs(rng, 4200, [(1950 + 50 * k, 200 + 60 * k)], edits=True, query_len=4400 + 60 * k)
        t = t[:500] + draw(rng, "CGT", 3000) if kind == "unrelated tail" else t[:1000]
        out.append(("reversed half word 64, " + kind, q[::-1], t[::-1]))
    return out


def hirschberg_split(forward_row, reverse_row):
    """The target column at which the kernels split a part: the minimum of forward_row[t] + reverse_row[tn - t], taken as the
    reference's 32 lanes take it (lane l sees t = l, l + 32, ... and keeps its first minimum; among lanes the lowest wins)."""
    tn = len(forward_row) - 1
    best = None
    for lane in range(32):
        for t in range(lane, tn + 1, 32):
            total = forward_row[t] + reverse_row[tn - t]
            if best is None or total < best[0]:
                best = (total, t)
    return best[1]


# name: (half, boundary) -- the half (0 forward, 1 reversed) whose chain crosses that boundary
HIRSCHBERG_BOUNDARY = {"%s half word 64, %s" % (h, k): (i, 63) for i, h in enumerate(("forward", "reversed"))
                       for k in ("unrelated tail", "short target")}


def semiglobal_pairs():
    """Infix / prefix (the ends scan): (name, query, target, boundaries, generated). Queries of 2 047, 2 048, 2 049 and 4 100 bases with
    runs across word 64 (bases 1 950 .. 2 149) and, at 4 100, across word 128 (to the last base); targets = the query's
    other bases with 2 % edits between random flanks. The homopolymer pairs of the scan model's own test. One query beyond
    16 384 bases (the workspace variant) against a short target. `boundaries` are the hand-overs that a propagated carry of
    the pair is meant to cross: 63 and 127 are the carries out of lane 63 into the next round. `generated` are those that
    the homopolymer and tandem pairs reach with carries that word 63 generates itself (their words seldom propagate); None
    for the two pairs of one base alone, which the scan model's test names: every word generates in every column, but where
    Eq is all ones Xh is all ones whatever the carry, so they witness nothing -- they run on the GPU all the same."""
    rng = random.Random(20260108)

    def flanked(q, t, flank):
        return q, draw(rng, "CGT", flank) + t + draw(rng, "CGT", flank)

    out = []
    for n, runs, boundaries in ((2047, [(1900, 147)], ()), (2048, [(1500, 127), ("end", 65)], ()),
                                (2049, [(1949, 100)], (63,)), (2049, [(700, 543)], ()),
                                (4100, [(1950, 200)], (63,)), (4100, [(3890, 210)], (127,)),
                                (4100, [(1990, 96), (3999, 101)], (63, 127))):
        total = sum(length for _, length in runs)
        q, t = absent_runs(rng, n - total, runs, edits=True, query_len=n)
        out.append(("runs %s in %d" % (runs, n),) + flanked(q, t, 100) + (boundaries, ()))
    out.append(("A2049 infix", "A" * 2049, "C" + "A" * 2049, (), None))
    out.append(("A2049 prefix", "A" * 2049, "A" * 2048 + "C", (), None))
    q, t = unequal_homopolymers(rng, 2049, 2100, 10, "T")
    out.append(("homopolymer2049v2100", q, t, (), (63,)))
    q, t = tandem_repeats(rng, 3, 700, 720, 20)
    out.append(("tandem3x700v720", q, t, (), (63,)))
    q, t = absent_runs(rng, 600, [(300, 1800), (2300, 2000), (4350, 12000)])
    out.append(("16 400 bases", q, t, (63, 127), ()))
    return out


def mapper_reads():
    """(query reads, target reads, overlap rows): two hand-built overlaps, one per strand, whose query slices carry a 300-base
    absent run. rows = (query read, target read, query start, query end, target start, target end, strand). On '-' the
    aligner sees the reverse complement of the target slice, so that target read is the reverse complement of a C / G / T
    sequence."""
    rng = random.Random(20260109)
    q0, t0 = absent_runs(rng, 1500, [(700, 300)], edits=True)
    q1, t1 = absent_runs(rng, 1400, [(333, 300)], edits=True)
    pad = lambda s: draw(rng, "CGT", 50) + s + draw(rng, "CGT", 70)
    queries = [pad(q0), pad(q1)]
    targets = [pad(t0), revcomp(pad(t1))]
    rows = [(0, 0, 50, 50 + len(q0), 50, 50 + len(t0), "+"),
            (1, 1, 50, 50 + len(q1), 70, 70 + len(t1), "-")]
    return queries, targets, rows


def fuzz_pair(rng, max_diff=None):
    """One pair drawn from the three families (tools/fuzz_gpu_vs_oracle.py): 100 .. 1 500 bases; max_diff bounds the length
    difference (the Ukkonen class refuses more than 10 % of its target limit)."""
    family = rng.choice(["absent", "absent", "homopolymer", "tandem"])
    cap = max_diff if max_diff is not None else 600
    if family == "absent":
        lengths = [x for x in RUN_LENGTHS + sorted(GROUP_RUN_LENGTHS.values()) if x + 8 <= cap] or [cap // 2]
        length = rng.choice(lengths)
        t_len = rng.choice([200, 400, 800, 1200])
        if max_diff is not None:
            t_len = max(t_len, 12 * length)
        start = rng.choice([0, "end", rng.randrange(0, t_len - 40)])    # (the edits move the length by a few bases)
        return absent_runs(rng, t_len, [(start, length)], edits=rng.random() < 0.5, run_base=rng.choice("ACGT"))
    if family == "homopolymer":
        n = rng.choice([100, 300, 700, 1200])
        d = rng.randint(1, min(70, cap, n // 11 if max_diff is not None else 70))
        nq, nt = (n, n + d) if rng.random() < 0.5 else (n + d, n)
        return unequal_homopolymers(rng, nq, nt, rng.choice([0, 17, 64]), rng.choice("ACGT"))
    period = rng.randint(2, 6)
    copies = rng.choice([60, 150, 240])
    d = rng.randint(1, max(1, min(12, copies // 11)))
    cq, ct = (copies, copies + d) if rng.random() < 0.5 else (copies + d, copies)
    return tandem_repeats(rng, period, cq, ct, rng.choice([0, 10, 33]))
