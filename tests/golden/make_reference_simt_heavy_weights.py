"""Writes tests/golden/reference_simt_heavy_weights.json: what the REFERENCE ITSELF answers for the heavy-edge-weight windows of
tests/poa_int16_edge_cases.py (weight_cases: base weights of 127 on up to 359 reads, edge weights past 32767 and past the
uint16 wrap at 65536) -- its cudapoa library run on the CPU by the SIMT emulator of oracle/simt
(`make -C oracle -f Makefile.ref ref_cudapoa_simt`, tests/ref_cudapoa.py), the route of make_reference_simt_goldens.py.
Data only: the reads are regenerated from the seed by poa_int16_edge_cases.py; the file holds, per case id, the reference's
status, consensus and coverage and a digest of the reads they belong to.
usage: python tests/golden/make_reference_simt_heavy_weights.py"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_simt_heavy_weights.json")


def digest(case):
    h = hashlib.sha256()
    for r, w in zip(case["reads"], case["weights"]):
        h.update(r.encode() + b"\0" + bytes(w) + b"\0")
    return h.hexdigest()


def run_reference(case):
    import poa_int16_edge_cases as E
    import ref_cudapoa as R
    c = case["config"]
    with R.RefBatch(c["max_seq"], c["max_seqs"], c["band_width"], E.BAND_MODES[c["band_mode"]], graph_factor=c["graph_factor"], gap=c["gap"],
                    mismatch=c["mismatch"], match=c["match"], output_mask=1) as b:
        add_status, read_status = b.add_poa_group(case["reads"], case["weights"])
        assert add_status == 0 and not any(read_status), (case["id"], add_status, read_status)
        b.generate_poa()
        return b.get_consensus()[0]


def main():
    import poa_int16_edge_cases as E
    rows = {}
    for case in E.weight_cases():
        t = time.time()
        ref = run_reference(case)
        rows[case["id"]] = dict(reads_sha256=digest(case), status=ref["status"], consensus=ref["consensus"], coverage=ref["coverage"])
        print(case["id"], "status", ref["status"], "consensus is", "r" if ref["consensus"] == case["r"] else "v" if ref["consensus"] == case["v"] else "?",
              "%.1f s" % (time.time() - t), flush=True)
    write(rows)


def write(rows):
    """One line per window."""
    with open(OUT, "w") as f:
        f.write('{"generator":"tests/golden/make_reference_simt_heavy_weights.py",\n"source":"the reference\'s cudapoa library on oracle/simt",\n"windows":{\n')
        f.write(",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in rows.items()))
        f.write("\n}}\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
