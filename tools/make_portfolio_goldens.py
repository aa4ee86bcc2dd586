"""Golden vectors for the LEXIMIN / XMIN analysis side, from the UNMODIFIED reference.

Runs only where the reference tree exists (make_goldens.REF); it is imported at run time and only
its OUTPUTS are written, as tests/golden/portfolio_<instance>.json.  The solvers need Gurobi, so
analysis.find_distribution_leximin / find_distribution_xmin are set to a function that returns a
fixed ``(portfolio, probabilities, [])``; the reference's own leximin_probabilities and
xmin_probabilities (analysis.py:194-228) then do everything after the solver.

Portfolio: P panels drawn by the reference's legacy_find after random.seed(5), as frozensets (what
the solvers return).  Probabilities: RandomState(7) uniforms x 2^-randint(0, 12) (12 binades, so the
float64 sums depend on their order), one exact 0.0, one 1e-13 (below LEXIMIN's 1e-11 threshold),
the rest scaled so that all sum to 1.

Stored per case, in portfolio_<instance>.json: the weights as JSON floats (repr round-trips
float64), the pair values as the SHA-256 of the little-endian float64 triangle in key order, and the
sizes of both returned sets (as the reference holds them -- tuples in frozenset iteration order --
and as distinct panels).  The bulky arrays go to portfolio_<instance>.npz beside it, exact and out of
the text diff: ``portfolio`` (uint16[P, k], each panel's sorted positions), ``alloc`` (float64[n])
and, for n <= 200, ``pairs`` (the float64 triangle itself).

Usage:  python tools/make_portfolio_goldens.py [instance ...]
"""
import hashlib
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import GOLD, INST, import_reference  # noqa: E402

# (file name, instance dir, k, P)
CASES = [
    ("couples", "couples_panel_from_twenty_people_no_constraints_2", 2, 97),
    ("example_small_20", "example_small_20", 20, 300),
    ("sf_e_110", "sf_e_110", 110, 130),
]


def weights_for(P):
    rs = np.random.RandomState(7)
    w = rs.uniform(size=P) * 2.0 ** -rs.randint(0, 13, size=P).astype(np.float64)
    zero, tiny = P // 3, (2 * P) // 3
    rest = np.ones(P, bool)
    rest[[zero, tiny]] = False
    w[rest] *= (1.0 - 1e-13) / w[rest].sum()
    w[zero], w[tiny] = 0.0, 1e-13
    return [float(x) for x in w]


def make(analysis, name, inst_dir, k, P):
    d = os.path.join(INST, inst_dir)
    inst = analysis.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)
    n = len(inst.agents)
    random.seed(5)
    portfolio = [frozenset(sorted(analysis.legacy_find(inst.categories, inst.agents, k))) for _ in range(P)]
    weights = weights_for(P)

    def solver(categories, agents, columns_data, number_people_wanted, check_same_address, columns):
        return list(portfolio), list(weights), []

    analysis.find_distribution_leximin = analysis.find_distribution_xmin = solver
    lex_alloc, lex_set, lex_hist = analysis.leximin_probabilities(inst)
    x_alloc, x_set, x_hist = analysis.xmin_probabilities(inst)
    ids = list(inst.agents)
    assert ids == list(range(n))
    assert lex_hist.get_dict() == x_hist.get_dict() and lex_alloc == x_alloc
    tri = np.array([float(v) for v in x_hist.get_dict().values()], "<f8")     # key order: i < j row-major
    assert len(tri) == n * (n - 1) // 2
    out = {
        "instance": inst_dir, "k": k, "n": n, "P": P, "panel_seed": 5, "weight_seed": 7,
        "distinct_panels": len(set(portfolio)),
        "weights": weights,
        "pairs_sha256": hashlib.sha256(tri.tobytes()).hexdigest(),
        "leximin_set_size": len(lex_set), "leximin_distinct": len({frozenset(t) for t in lex_set}),
        "xmin_set_size": len(x_set), "xmin_distinct": len({frozenset(t) for t in x_set}),
    }
    arrays = {"portfolio": np.array([sorted(p) for p in portfolio], np.uint16),
              "alloc": np.array([float(x_alloc[a]) for a in ids], "<f8")}
    assert arrays["portfolio"].shape == (P, k)
    if n <= 200:
        arrays["pairs"] = tri
    np.savez_compressed(os.path.join(GOLD, "portfolio_%s.npz" % name), **arrays)
    path = os.path.join(GOLD, "portfolio_%s.json" % name)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("%s: n=%d P=%d distinct=%d leximin set %d xmin set %d -> %s (%d bytes)"
          % (name, n, P, out["distinct_panels"], out["leximin_set_size"], out["xmin_set_size"], path,
             os.path.getsize(path)))


def main():
    _, analysis = import_reference()
    want = set(sys.argv[1:])
    for name, inst_dir, k, P in CASES:
        if not want or name in want:
            make(analysis, name, inst_dir, k, P)


if __name__ == "__main__":
    main()
