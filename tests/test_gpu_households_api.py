"""The household keywords of the Monte Carlo calls against the reference's own check_same_address runs
(tests/golden/address_*.json, "philox" and "mt" sections: tools/make_goldens.py drove the unmodified
find_random_sample_legacy with check_same_address=True in a legacy_find-shaped restart loop).

legacy_probabilities(inst, S, seed, columns_data=cols, check_same_address_columns=columns) must return the
golden's counts / S, as many found panels as the golden has distinct ones and exactly its panels, and leave
the golden's attempts in LAST_RUN_STATS; no pair of ring mates ever shares a panel (pair histogram and
stats.household_groups composition); legacy_panel_distribution with the keywords counts the same distinct
panels; and a call without the keywords right after draws the ring-free golden again (the rings and the
route are off the handle).  In Philox mode a spy on DevicePipeline.draw_xt sees a household kernel and the
fused XT.
"""
import csv
import json
import os

import numpy as np
import pytest

from conftest import GOLD, REPO, golden, inst_paths, pkg

pytestmark = pytest.mark.gpu

ADDR = sorted(f[:-5] for f in os.listdir(GOLD) if f.startswith("address_") and f.endswith(".json"))
RING_FREE = {"sf_e_tight_110": "sf_e_tight_110_s1", "example_small_20": "example_small_20_s0"}


def _load(case, section):
    with open(os.path.join(GOLD, case + ".json")) as fh:
        g = json.load(fh)[section]
    with open(os.path.join(REPO, g["addresses"]), encoding="utf-8") as fh:
        cols = {i: dict(r) for i, r in enumerate(csv.DictReader(fh))}
    return g, cols


def _pack(picks, pos, W):
    """Pick lists (agent ids) -> sorted distinct uint64[D, W] rows, as PanelSet.rows() sorts them."""
    rows = np.zeros((len(picks), W), np.uint64)
    for i, panel in enumerate(picks):
        for aid in panel:
            p = pos[aid]
            rows[i, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    return np.unique(rows, axis=0)


@pytest.mark.parametrize("section", ["philox", "mt"])
@pytest.mark.parametrize("case", ADDR)
def test_legacy_probabilities_with_households(gpu_available, monkeypatch, case, section):
    P, A, S_, Lg, Dv = pkg(), pkg("analysis"), pkg("stats"), pkg("legacy"), pkg("device")
    g, cols = _load(case, section)
    columns, S, seed, k = g["columns"], g["S"], g["seed"], g["k"]
    inst = P.read_instance(*inst_paths(g["instance"]), k)
    enc = pkg("instance").encode_cached(inst.categories, inst.agents)
    ids = list(enc.agent_ids)
    pos = {aid: p for p, aid in enumerate(ids)}
    ring = Lg.address_rings(ids, cols, columns)
    mates = np.array([(p, int(ring[p])) for p in range(enc.n) if ring[p] != p])
    assert len(mates) > 10

    calls = []
    draw_xt = Dv.DevicePipeline.draw_xt

    def spy(self, *a, **kw):
        name = self.draw_kernel_name()
        done = draw_xt(self, *a, **kw)
        calls.append((name, done))
        return done
    monkeypatch.setattr(Dv.DevicePipeline, "draw_xt", spy)

    kw = dict(columns_data=cols, check_same_address_columns=columns, rng=section)
    alloc, found, hist = A.legacy_probabilities(inst, S, seed, **kw)
    assert [alloc[a] for a in ids] == (np.array(g["counts"], np.int64) / S).tolist()
    assert len(found) == g["unique"]
    assert np.array_equal(found.rows(), _pack(g["picks"], pos, enc.W))
    assert A.LAST_RUN_STATS["attempts"] == sum(g["attempts"])
    if section == "philox":
        assert len(calls) == 1 and calls[0][1] is True, calls
        assert calls[0][0].startswith(("draw_solo_hh_kernel<", "draw_lane_hh_kernel<")), calls
        assert calls[0][0] in pkg("_native").household_kernel_list()
    else:
        assert calls == []
    # no two ring mates in one panel: the pair histogram ...
    full = np.zeros((enc.n, enc.n))
    full[np.triu_indices(enc.n, 1)] = hist.upper()
    full += full.T
    assert full.sum() > 0 and not full[mates[:, 0], mates[:, 1]].any()
    # ... and the composition over the households
    groups = S_.household_groups(ids, cols, columns)
    assert len(groups) > 5
    alloc2, found2, _, comp = A.legacy_composition(inst, S, seed, groups, **kw)
    assert alloc2 == alloc and len(found2) == len(found)
    assert comp.counts.shape == (len(groups), k + 1)
    assert (comp.counts.sum(axis=1) == S).all() and not comp.counts[:, 2:].any() and comp.counts[:, 1].any()
    # the panel distribution of the same run
    calls.clear()
    dist = A.legacy_panel_distribution(inst, S, seed, **kw)[3]
    assert dist.distinct == g["unique"]
    if section == "philox":
        assert calls and calls[0][0].startswith(("draw_solo_hh_kernel<", "draw_lane_hh_kernel<")) and calls[0][1]
    # without the keywords, right after: the ring-free run, on the ring-free kernel
    calls.clear()
    g0 = golden(RING_FREE[g["instance"]])
    alloc0, found0, _ = A.legacy_probabilities(inst, g0["S"], g0["seed"])
    assert [alloc0[a] for a in ids] == (np.array(g0["counts"], np.int64) / g0["S"]).tolist()
    assert len(found0) == g0["unique"]
    assert len(calls) == 1 and calls[0][0].startswith(("draw_solo_kernel<", "draw_lane_kernel<")) and calls[0][1]
