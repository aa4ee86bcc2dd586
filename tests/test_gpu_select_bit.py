"""select_bit's nibble table on the device: pools whose every word is dense.

tests/test_select_bit_host.py checks the table's construction on the host; here the draw kernels use it.  The
pools are tests/test_gpu_pick_drop.py's draw-everyone instances (k = n = 64 W, one category, maxima = holder
counts) with EVERY word given to one feature of its own: the masked word the select works on starts as all
64 agents of a word and loses one agent per pick, so every nibble of it is met full at ranks 1 to 4 and in
every sparser state on the way to empty, in both lanes' orders (the second lane's pool is mirrored).  The
remaining features of the category have no holders (minimum = maximum = 0: removed from the tables), which
keeps F where the kernel family needs it.  Pick lists in pick order, panels, hashes, attempts and the draw
statistics are compared bit for bit with the C oracle, through the row pick lists and the fused pack.
"""
import numpy as np
import pytest

import test_gpu_pick_drop as pick_drop
from conftest import pkg

W = 4
CASES = [pick_drop._case("lane", W, (17,), single=range(W)), pick_drop._case("solo", W, (8,), single=range(W)),
         pick_drop._case("solo", W, (16,), single=range(W))]
IDS = ["%s-F%d" % (c.kernel, sum(c.cats)) for c in CASES]


def test_every_word_is_one_features_holders():
    """On the oracle alone: the instances are what the docstring says, and every panel picks everyone at the
    first attempt."""
    for case in CASES:
        _, _, o = pick_drop.instance(case)
        pf = np.asarray(o.person_feat)[:, 0]
        assert o.n == 64 * W and [set(pf[64 * w: 64 * w + 64].tolist()) for w in range(W)] == [{w} for w in range(W)]
        assert o.fmax[:W] == [64] * W and not any(o.fmax[W:])
        ref = pick_drop.reference(case)
        assert np.all(ref.attempts == 1) and np.all(np.sort(ref.picks, axis=1) == np.arange(o.n))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dense_words_match_oracle(gpu_available, case):
    cats, agents, o = pick_drop.instance(case)
    ref = pick_drop.reference(case)
    enc = pkg().encode(cats, agents)
    try:
        name = pick_drop._kernel_name(enc, o.k)
        want = "draw_lane_kernel<32, %d," % W if case.kernel == "lane" else "draw_solo_kernel<%d, %d," % (sum(case.cats), W)
        assert name.startswith(want), name
        pick_drop._check_picks(enc, ref, o.k, pick_drop.S, pick_drop.SEED, pick_drop.BEGIN)
        pick_drop._check_fused(enc, ref, o.k, pick_drop.S, pick_drop.SEED, pick_drop.BEGIN)
    finally:
        enc.close()
