"""Writes tests/golden/cudamapper_reference_simt.npz and .json: the cases of tests/mapper_cases.reference_simt_cases()
answered by the REFERENCE's own cudamapper kernels on the CPU emulator (oracle/_ref/libref_cudamapper_simt.so, built by
`make -C oracle all` where the reference checkout exists). Every case is answered three times, each in a process of its
own: in the default lane order, with SIMT_ORDER=reverse (the answers must be equal: oracle/simt/README.md) and with
SIMT_MALLOC_FILL=165 (a case whose answer changes reads memory the reference never wrote: it is recorded as
fill_dependent in the JSON and is no parity target). No case drops out silently: the script asserts that every case asked
for was answered. usage: python tests/golden/make_mapper_reference_simt_goldens.py"""
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mapper_cases as MC  # noqa: E402


def answer(case):
    """the reference's outputs of one case, as the fixture's entries"""
    import ref_cudamapper as R
    out, p = {}, case["name"] + "/"
    if case["stage"] == "index":
        reads = MC.index_case_reads(case["cls"], case["k"], case["w"], case["seed"])
        MC.fixture_put(out, p + "bases", np.frombuffer(b"".join(reads) or b"", np.uint8))
        out["__meta__"][p + "lengths"] = [len(r) for r in reads]
        MC.fixture_put_index(out, p, R.index(reads, case["k"], case["w"], case["hash"], case["F"], case["first_read_id"]))
    elif case["stage"] == "matcher":
        q, t = MC.matcher_case_inputs(case["cls"], case["k"], case["w"], case["hash"], case["seed"])
        side = {}
        for name, s in (("query", q), ("target", t)):
            if s is None:
                side[name] = side["query"]
            elif "index" in s:
                side[name] = s["index"]
            else:
                side[name] = R.index(s["reads"], case["k"], case["w"], case["hash"], 1.0, s["first_read_id"])
            MC.fixture_put_index(out, p + name + "/", side[name], whole=True)
            assert all((p + name + "/" + a) in out for a in MC.INDEX_ARRAY_NAMES), "a matcher case's index is stored whole"
        MC.fixture_put(out, p + "anchors", R.anchors(side["query"], side["target"]))
    elif case["stage"] == "map":
        queries, targets = MC.map_case_reads(case)
        MC.fixture_put(out, p + "bases", np.frombuffer("".join(queries + (targets or [])).encode(), np.uint8))
        q = R.index(queries, case["k"], case["w"], True, case["F"])
        t = q if targets is None else R.index(targets, case["k"], case["w"], True, case["F"])
        o = R.overlaps(R.anchors(q, t), targets is None, **MC.OVERLAPPER_FILTERS[case["filter"]])
        MC.fixture_put(out, p + "overlaps", np.frombuffer(MC.overlap_bytes(o), np.uint8))
        out["__meta__"][p + "n_overlaps"] = len(o)
    else:
        anchors = MC.overlapper_case_input(case)
        MC.fixture_put(out, p + "anchors", anchors)
        o = R.overlaps(anchors, case["all_to_all"], **MC.OVERLAPPER_FILTERS[case["filter"]])
        MC.fixture_put(out, p + "overlaps", np.frombuffer(MC.overlap_bytes(o), np.uint8))
        out["__meta__"][p + "n_overlaps"] = len(o)
    return out


def answer_all(path):
    out = {"__meta__": {}}
    for case in MC.reference_simt_cases():
        one = answer(case)
        out["__meta__"].update(one.pop("__meta__"))
        out.update(one)
    with open(path, "wb") as f:
        pickle.dump(out, f)


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def of_case(answers, prefix):
    out = {k: v for k, v in answers.items() if k.startswith(prefix)}
    out.update(("meta " + k, np.array(v)) for k, v in answers["__meta__"].items() if k.startswith(prefix))
    return out


def main():
    import ref_cudamapper as R
    assert R.available(), "build oracle/_ref/libref_cudamapper_simt.so first (make -C oracle all, with the reference checkout)"
    t0 = time.time()
    answers = {}
    with tempfile.TemporaryDirectory() as tmp:
        for mode, env in (("default", {}), ("reverse", {"SIMT_ORDER": "reverse"}), ("fill", {"SIMT_MALLOC_FILL": "165"})):
            path = os.path.join(tmp, mode + ".pkl")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--answer", path], check=True, env=dict(os.environ, **env))
            with open(path, "rb") as f:
                answers[mode] = pickle.load(f)
    cases = MC.reference_simt_cases()
    described = []
    for case in cases:
        p = case["name"] + "/"
        per_mode = {m: of_case(a, p) for m, a in answers.items()}
        assert per_mode["default"], "no answer for " + case["name"]
        assert same(per_mode["default"], per_mode["reverse"]), "the lane order changes the answer of " + case["name"]
        described.append(dict(case, fill_dependent=not same(per_mode["default"], per_mode["fill"])))
    assert len(described) == len(cases) and len(set(c["name"] for c in cases)) == len(cases)
    fixture = {k: v for k, v in answers["default"].items() if k != "__meta__"}
    fixture["__meta__"] = np.str_(json.dumps(answers["default"]["__meta__"], sort_keys=True))
    np.savez_compressed(MC.REFERENCE_SIMT_NPZ, **fixture)
    with open(MC.REFERENCE_SIMT_JSON, "w") as f:
        json.dump(dict(source="reference cudamapper (minimizer.cu, index_gpu.cu/.cuh, matcher_gpu.cu, overlapper_triggered.cu) on oracle/simt",
                       lane_orders="default and SIMT_ORDER=reverse answer every case identically",
                       cases=described), f, indent=1)
        f.write("\n")
    by = {}
    for c in described:
        by[(c["stage"], c["cls"])] = by.get((c["stage"], c["cls"]), 0) + 1
    for key in sorted(by):
        print("%-10s %-22s %d" % (key[0], key[1], by[key]))
    print("fill dependent:", [c["name"] for c in described if c["fill_dependent"]])
    print("%d cases, %.1f s, %d bytes" % (len(described), time.time() - t0, os.path.getsize(MC.REFERENCE_SIMT_NPZ)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--answer":
        answer_all(sys.argv[2])
    else:
        main()
