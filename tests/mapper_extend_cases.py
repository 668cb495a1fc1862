"""Cases of cudamapper.extend_overlaps' tests: a 2 kbp draft and twelve reads of both strands whose overlap records have
their ends pulled in."""
import random

import numpy as np

from affine_cases import mutate, random_sequence

OVERLAP = np.dtype({"names": ["query_read_id", "target_read_id", "query_start_position_in_read",
                              "target_start_position_in_read", "query_end_position_in_read",
                              "target_end_position_in_read", "relative_strand", "num_residues", "overlap_complete"],
                    "formats": ["<u4"] * 6 + ["u1", "<u4", "u1"],
                    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32], "itemsize": 36})


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def case(seed, pulls=(50, 120), read_error=0.0, tail=0, reads=12, draft_length=2000):
    """(reads, [draft], records, truth): read k is draft[a:b] (odd k: its reverse complement) with read_error errors and
    `tail` unrelated bases on either side; record k has the true ends -- truth[k] = (qs, qe, ts, te), exact for error-free
    reads -- pulled in by pulls[k % len(pulls)] bases per end. Read 0 starts at the draft's first base and read 1 ends at its
    last."""
    r = random.Random(seed)
    draft = random_sequence(r, draft_length)
    out, records, truth = [], np.zeros(reads, OVERLAP), []
    for k in range(reads):
        length = r.randrange(400, 700)
        a = 0 if k == 0 else draft_length - length if k == 1 else r.randrange(0, draft_length - length)
        b = a + length
        body = draft[a:b]
        if k % 2:
            body = rc(body)
        if read_error:
            body = mutate(r, body, read_error)
        read = random_sequence(r, tail) + body + random_sequence(r, tail)
        out.append(read)
        pull = pulls[k % len(pulls)]
        truth.append((tail, tail + len(body), a, b))
        records[k] = (k, 0, tail + pull, a + pull, tail + len(body) - pull, b - pull, ord("-" if k % 2 else "+"), 10 + k, k % 2)
    return out, [draft], records, truth
