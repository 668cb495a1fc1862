"""tests/oracle_semiglobal.py against the definition of the infix / prefix alignment types spelled out by brute force:
every slice of the target, a textbook edit distance in plain Python. All pairs over {A, C} with n <= 4 and m <= 5."""
import itertools

import oracle_semiglobal as S


def levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(row[j - 1] + (x != y), row[j] + 1, cur[j - 1] + 1))
        row = cur
    return row[-1]


def brute_force(q, t, mode):
    begins = lambda e: [0] if mode == "prefix" else range(e + 1)
    best = {e: min(levenshtein(q, t[b:e]) for b in begins(e)) for e in range(len(t) + 1)}
    d = min(best.values())
    te = min(e for e in best if best[e] == d)
    tb = max(b for b in begins(te) if levenshtein(q, t[b:te]) == d)
    return d, te, tb


def words(max_len):
    for k in range(max_len + 1):
        for w in itertools.product("AC", repeat=k):
            yield "".join(w)


def test_dp_equals_the_definition_on_all_small_pairs():
    checked = 0
    for q in words(4):
        for t in words(5):
            for mode in ("infix", "prefix"):
                assert S.semiglobal(q, t, mode) == brute_force(q, t, mode), (q, t, mode)
                checked += 1
    assert checked == 31 * 63 * 2


def test_known_cases():
    assert S.semiglobal("AAAA", "CCCC", "infix") == (4, 0, 0)
    assert S.semiglobal("ACG", "ACGACG", "infix") == (0, 3, 0)
    assert S.semiglobal("GAC", "TTAC", "infix") == (1, 4, 2)       # TAC and AC are both at distance 1: the largest begin
    assert S.semiglobal("ACGT", "TTTTACGT", "infix")[0] == 0
    assert S.semiglobal("ACGT", "TTTTACGT", "prefix")[0] > 0
    assert S.semiglobal("", "ACGT", "infix") == (0, 0, 0)
    assert S.semiglobal("ACGT", "", "prefix") == (4, 0, 0)
    assert S.global_distance("ACGT", "AGT") == 1


def test_match_predicate_is_the_default_aligners():
    # a target base is read as "ACTG"[(t >> 1) & 3]: N (0x4e) reads as G, as in the default global aligner
    assert S.semiglobal("G", "N", "infix")[0] == 0
    assert S.semiglobal("N", "N", "infix")[0] == 1
