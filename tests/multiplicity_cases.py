"""What the panel-multiplicity tests share (tests/test_multiplicity_host.py on the CPU,
tests/test_gpu_multiplicity.py on the device): the reference's panel counts
(tests/golden/multiplicity_<case>.json, written by tools/make_multiplicity_goldens.py) and the C oracle's
panels of the same runs."""
import json
import os

import numpy as np

from conftest import GOLD, inst_paths

CASES = ["couples_s0", "pathological_5_s0", "rejecty_6_s3"]


def mult_golden(case):
    with open(os.path.join(GOLD, "multiplicity_%s.json" % case)) as fh:
        return json.load(fh)


def oracle_panels(instance, k, seed, S):
    """uint64[S, W]: the C oracle's panels of (instance, k, seed)."""
    from oracle import coracle
    from oracle.legacy_oracle import read_instance as oracle_read
    cat, resp = inst_paths(instance)
    rc, panels, _, _ = coracle.draw(oracle_read(cat, resp, k), k, seed, 0, S)
    assert rc == 0
    return panels


def pack(panels, n):
    """Lists of positions -> uint64[len, W] rows."""
    W = (n + 63) // 64
    out = np.zeros((len(panels), W), np.uint64)
    for i, panel in enumerate(panels):
        for p in panel:
            out[i, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    return out


def expected_top(g, m):
    """The m most frequent panels of a golden as (tuple, count), ties by first index."""
    order = sorted(range(len(g["count"])), key=lambda e: (-g["count"][e], g["first"][e]))[:m]
    return [(tuple(g["panels"][e]), g["count"][e]) for e in order]
