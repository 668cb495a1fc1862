"""cudamapper.extend_overlaps in Python: the overlap rule on top of oracle_extend.extend().
Everything happens in the target's strand coordinates: T' is the target on '+', its reverse complement by the aligner's
table on '-', and [ts', te') = [Lt - te, Lt - ts) there."""
import numpy as np

import oracle_extend as O


def aligner_rc(s):
    """the reverse complement as cudaaligner takes it: "TGAC"[(c >> 1) & 3] for every byte, back to front"""
    return "".join("TGAC"[(ord(c) >> 1) & 3] for c in reversed(s))


def extend_overlap(x, q, t, extension=O.DEFAULT + (64, 200), max_extension=1024):
    """One record `x` (any mapping with the OVERLAP fields) over its reads q and t:
    ((qs, qe, ts, te) after the extension, [head i*, head j*, tail i*, tail j*], [head score, tail score])"""
    qs, qe = int(x["query_start_position_in_read"]), int(x["query_end_position_in_read"])
    ts, te = int(x["target_start_position_in_read"]), int(x["target_end_position_in_read"])
    minus = chr(int(x["relative_strand"])) == "-"
    M = max_extension
    if M == 0:
        return (qs, qe, ts, te), [0, 0, 0, 0], [0, 0]
    strand = aligner_rc(t) if minus else t
    if minus:
        ts, te = len(t) - te, len(t) - ts
    tail = O.extend(q[qe:qe + M], strand[te:te + M], *extension)
    head = O.extend(q[max(0, qs - M):qs][::-1], strand[max(0, ts - M):ts][::-1], *extension)
    qs, ts = qs - head["query_end"], ts - head["target_end"]
    qe, te = qe + tail["query_end"], te + tail["target_end"]
    if minus:
        ts, te = len(t) - te, len(t) - ts
    return (qs, qe, ts, te), [head["query_end"], head["target_end"], tail["query_end"], tail["target_end"]], \
        [head["score"], tail["score"]]


def extend_overlaps(overlaps, query_reads, target_reads, extension=O.DEFAULT + (64, 200), max_extension=1024):
    """(records, extensions [n][4], scores [n][2]) as cudamapper.extend_overlaps returns them"""
    out = np.array(overlaps, copy=True)
    moved, scores = np.zeros((len(out), 4), np.int32), np.zeros((len(out), 2), np.int32)
    for k, x in enumerate(overlaps):
        ends, moved[k], scores[k] = extend_overlap(x, query_reads[int(x["query_read_id"])], target_reads[int(x["target_read_id"])],
                                                   extension, max_extension)
        (out[k]["query_start_position_in_read"], out[k]["query_end_position_in_read"],
         out[k]["target_start_position_in_read"], out[k]["target_end_position_in_read"]) = ends
    return out, moved, scores
