"""Golden vectors for the intersectional-representation numbers, from the UNMODIFIED reference.

Runs only where the reference tree exists (make_goldens.REF); it is imported at run time and only
its OUTPUTS are written, as tests/golden/intersections_sf_e_110.json.  The reference's own
plot_intersectional_representation (analysis.py:474-530) is called in a temporary working directory
that holds ``data/sf_e_110/intersections.csv`` (tests/golden/sf_e_110_intersections.csv, the
reference's input table) and ``analysis/``.  The seaborn stub gets a no-op ``set_style`` and a
``jointplot`` that keeps the data frame it is handed: that frame holds the five shares per row, which
the function itself never returns.

Inputs: the committed synthetic sf_e_110 pool; ``legacy_alloc`` = counts / S of
philox_sf_e_110_s0.json; ``leximin_alloc`` = the ``alloc`` of portfolio_sf_e_110.npz.

Stored: per share column the 346 values in table order, and the seven MSEs under
"<share 1> - <share 2>" in the reference's order.  JSON floats (repr) round-trip float64.

Usage:  python tools/make_intersection_goldens.py
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import GOLD, INST, import_reference  # noqa: E402

SHARES = ("population share", "panel share LEGACY", "panel share LEXIMIN", "pool share", "quota share")


class _Joint:
    """What the reference does with jointplot's result: two axis limits and a savefig."""

    class _Axis:
        def set_xlim(self, *a):
            pass

        def set_ylim(self, *a):
            pass

    ax_joint = _Axis()

    def savefig(self, path):
        pass


def main():
    _, analysis = import_reference()
    frames = []

    def jointplot(data=None, **kw):
        frames.append(data)
        return _Joint()

    analysis.sns.set_style = lambda *a, **kw: None
    analysis.sns.jointplot = jointplot

    d = os.path.join(INST, "sf_e_110")
    inst = analysis.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), 110)
    ids = list(inst.agents)
    with open(os.path.join(GOLD, "philox_sf_e_110_s0.json")) as fh:
        g = json.load(fh)
    legacy_alloc = {aid: c / g["S"] for aid, c in zip(ids, g["counts"])}
    lex = np.load(os.path.join(GOLD, "portfolio_sf_e_110.npz"))["alloc"]
    leximin_alloc = {aid: float(x) for aid, x in zip(ids, lex)}

    cwd = os.getcwd()
    tmp = tempfile.mkdtemp()
    try:
        os.makedirs(os.path.join(tmp, "data", "sf_e_110"))
        os.makedirs(os.path.join(tmp, "analysis"))
        shutil.copy(os.path.join(GOLD, "sf_e_110_intersections.csv"),
                    os.path.join(tmp, "data", "sf_e_110", "intersections.csv"))
        os.chdir(tmp)
        errors = analysis.plot_intersectional_representation("sf_e", inst, legacy_alloc, leximin_alloc)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    assert errors is not None and len(errors) == 7 and len(frames) == 1
    df = frames[0]
    out = {
        "instance": "sf_e_110", "k": 110, "n": len(ids), "rows": int(len(df)),
        "legacy_alloc": "philox_sf_e_110_s0.json counts / S", "leximin_alloc": "portfolio_sf_e_110.npz alloc",
        "shares": {name: [float(x) for x in df[name]] for name in SHARES},
        "mse": [[a, b, float(v)] for (a, b), v in errors.items()],
    }
    path = os.path.join(GOLD, "intersections_sf_e_110.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("%d rows, 7 MSEs -> %s (%d bytes)" % (len(df), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
