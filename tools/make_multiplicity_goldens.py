"""Golden panel multiplicities, from the UNMODIFIED reference in Philox verification mode.

Runs only where the reference tree exists (make_goldens.REF); it is imported at run time, driven through
make_goldens.PhiloxHarness, and only its OUTPUTS are written, as tests/golden/multiplicity_<case>.json
(no ``philox_`` prefix: conftest.PHILOX_CASES globs that).

Per case the reference's own legacy_probabilities runs once; a Counter over its panel sequence (each
panel the sorted positions legacy_find returned) gives, per distinct panel in first-occurrence order,
the panel, the index of its first draw and its count.  The script asserts that the packed sequence
hashes to the existing philox_<case>.json's ``panels_sha256`` and that the Counter is as long as its
``unique``, so the file describes the same run as that golden.

Usage:  python tools/make_multiplicity_goldens.py [case ...]
"""
import json
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import CASES, GOLD, INST, PhiloxHarness, import_reference, pack, sha  # noqa: E402

MULT_CASES = ("couples_s0", "pathological_5_s0", "rejecty_6_s3")


def make(legacy, analysis, case, inst_dir, k, S, seed):
    d = os.path.join(INST, inst_dir)
    inst = analysis.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)
    n = len(inst.agents)
    with PhiloxHarness(legacy, analysis, seed) as h:
        _, found, _ = analysis.legacy_probabilities(inst, S, seed)
    panels = [tuple(sorted(p)) for p in h.picks]
    assert len(panels) == S
    counts = Counter(panels)                     # insertion order: first occurrence
    first = {}
    for i, p in enumerate(panels):
        first.setdefault(p, i)
    with open(os.path.join(GOLD, "philox_%s.json" % case)) as fh:
        g = json.load(fh)
    assert (g["S"], g["seed"], g["k"], g["n"]) == (S, seed, k, n)
    assert sha(pack(panels, n)) == g["panels_sha256"], "not the run of philox_%s.json" % case
    assert len(counts) == g["unique"] == len(found)
    assert list(counts) == sorted(counts, key=first.get) and sum(counts.values()) == S
    return {"case": case, "instance": inst_dir, "k": k, "S": S, "seed": seed, "n": n,
            "generator": "tools/make_multiplicity_goldens.py driving the unmodified reference",
            "panels_sha256": g["panels_sha256"], "unique": len(counts),
            "panels": [list(p) for p in counts],
            "first": [first[p] for p in counts],
            "count": [counts[p] for p in counts]}


def main(argv):
    legacy, analysis = import_reference()
    want = set(argv)
    for case, inst_dir, k, S, seed in CASES:
        if case not in MULT_CASES or (want and case not in want):
            continue
        g = make(legacy, analysis, case, inst_dir, k, S, seed)
        with open(os.path.join(GOLD, "multiplicity_%s.json" % case), "w") as fh:
            json.dump(g, fh, separators=(",", ":"))
        print("%-20s S=%-6d distinct=%-5d max=%d" % (case, S, g["unique"], max(g["count"])), file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
