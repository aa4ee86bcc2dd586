"""The oracles' same-address deletion (check_same_address; legacy.py:78-113), without a GPU.

  * Both oracles reproduce the "philox" section of tests/golden/address_*.json -- runs of the unmodified
    reference with check_same_address=True (tools/make_goldens.py) -- with the rings of
    legacy.address_rings over the committed addresses.csv: pick orders, attempts, per-person counts,
    distinct panels, the panels' sha256 and, for every recorded single attempt, its status, picks,
    selected / remaining counters and the people left.  These records pin the oracles.
  * Both reproduce tests/golden/cell_address_g64_1_2.json as well: the reference on the regenerated pool of
    the draw_kernel<64, 1, 2, true> cell (n = 4133) with the 70-member household, across panel 2^32.
  * On the GENERAL cells of tests/test_gpu_draw_matrix.py with the households of tests/address_cases.py,
    the C oracle (the only one fast enough for n = 8229) equals the Python oracle, which deletes person by
    person and feature by feature in the reference's order, on panels at both ends of each batch and on
    both sides of panel 2^32.
  * The conditions of tests/address_cases.py hold on the oracle alone, before any GPU is asked.
"""
import csv
import hashlib
import json
import os

import numpy as np
import pytest

import address_cases as AC
from conftest import GOLD, REPO, inst_paths, pkg
from oracle import coracle
from oracle.legacy_oracle import (FAIL, OK, PhiloxRng, draw_attempt, legacy_find, legacy_probabilities, pack_panels,
                                  read_instance)
from test_gpu_draw_matrix import BY_NAME, SEED, cell_S, oracle_instance, recipe_of

ADDR = sorted(f[:-5] for f in os.listdir(GOLD) if f.startswith("address_") and f.endswith(".json"))


def _load(case):
    with open(os.path.join(GOLD, case + ".json")) as fh:
        g = json.load(fh)["philox"]
    with open(os.path.join(REPO, g["addresses"]), encoding="utf-8") as fh:
        cols = {i: dict(r) for i, r in enumerate(csv.DictReader(fh))}
    inst = read_instance(*inst_paths(g["instance"]), g["k"])
    ring = pkg("legacy").address_rings(list(range(inst.n)), cols, g["columns"])
    assert (ring != np.arange(inst.n)).any()
    return g, inst, ring


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("case", ADDR)
def test_c_oracle_reproduces_the_reference_with_addresses(case):
    g, inst, ring = _load(case)
    S = g["S"]
    rc, panels, attempts, picks = coracle.draw(inst, g["k"], g["seed"], 0, S, want_picks=True, addr_next=ring)
    assert rc == 0
    assert attempts.tolist() == g["attempts"]
    assert picks[:len(g["picks"])].tolist() == g["picks"]
    assert coracle.counts(panels, inst.n).tolist() == g["counts"]
    assert coracle.unique(panels, inst.n) == g["unique"]
    assert _sha(panels) == g["panels_sha256"]
    # the rings matter: the ring-free draw of the same stream is another one
    assert _sha(coracle.draw(inst, g["k"], g["seed"], 0, S)[1]) != g["panels_sha256"]


@pytest.mark.parametrize("case", ADDR)
def test_python_oracle_reproduces_the_reference_with_addresses(case):
    g, inst, ring = _load(case)
    res = legacy_probabilities(inst, g["S"], g["seed"], mode="philox", want_pairs=False, addr_next=ring.tolist())
    assert res.attempts == g["attempts"]
    assert res.picks[:len(g["picks"])] == g["picks"]
    assert res.counts.tolist() == g["counts"]
    assert res.unique == g["unique"]
    assert _sha(pack_panels(res.panels, inst.n)) == g["panels_sha256"]


@pytest.mark.parametrize("case", ADDR)
def test_oracles_reproduce_the_reference_single_attempts(case):
    """find_random_sample_legacy(..., True, columns) at the golden's (panel, attempt) positions: the
    Python oracle's status, picks, counters and people left; the C oracle's restart loop fails and
    accepts at the same positions."""
    g, inst, ring = _load(case)
    src = PhiloxRng(g["seed"])
    statuses = {}
    for rec in g["single_attempts"]:
        status, picks, sel, rem, present = draw_attempt(inst, g["k"], src.for_attempt(rec["panel"], rec["attempt"]),
                                                        addr_next=ring.tolist())
        statuses.setdefault(rec["panel"], []).append(rec["status"])
        if rec["status"] == "SelectionError":
            assert status == FAIL
            continue
        assert status == OK and picks == rec["picks"]
        assert [[c, f, sel[j], rem[j]] for j, (c, f) in enumerate(inst.feat_names)] == rec["selected"]
        assert [p for p in range(inst.n) if present[p]] == rec["people_left"]
    # the C oracle's restart loop raised a SelectionError at each position where the reference did: the
    # records of a panel are its attempts 0, 1, ..., and its attempt count is past every failed one
    _, _, attempts, _ = coracle.draw(inst, g["k"], g["seed"], 0, 1 + max(statuses), addr_next=ring)
    for panel, s in statuses.items():
        assert attempts[panel] > max([a for a, st in enumerate(s) if st == "SelectionError"], default=-1)


def test_oracles_reproduce_the_reference_on_a_cell_pool():
    """tests/golden/cell_address_g64_1_2.json: the unmodified reference with check_same_address=True on
    draw_kernel<64, 1, 2, true>'s regenerated pool (n = 4133: 65 words), the households of
    tests/address_cases.py as its address column, 36 panels across panel 2^32."""
    with open(os.path.join(GOLD, "cell_address_g64_1_2.json")) as fh:
        g = json.load(fh)
    cell = BY_NAME[g["cell"]]
    _, o = oracle_instance(recipe_of(cell))
    ring = AC.ring_of(o.n)[0]
    assert (g["n"], g["k"], g["seed"]) == (o.n, cell.k, SEED)
    assert _sha(np.asarray(o.person_feat, np.int32)) == g["person_feat_sha256"]
    assert ring.tolist() == g["ring"]
    S, begin = g["S"], g["panel_begin"]
    assert begin < 2 ** 32 < begin + S
    rc, _, attempts, picks = coracle.draw(o, o.k, SEED, begin, S, want_picks=True, addr_next=ring)
    assert rc == 0 and attempts.tolist() == g["attempts"] and picks.tolist() == g["picks"]
    src = PhiloxRng(SEED)
    for i in range(S):
        assert legacy_find(o, o.k, src, begin + i, addr_next=g["ring"]) == (g["picks"][i], g["attempts"][i])
    for rec in g["single_attempts"]:
        status, picks, sel, rem, present = draw_attempt(o, o.k, src.for_attempt(rec["panel"], rec["attempt"]),
                                                        addr_next=g["ring"])
        if rec["status"] == "SelectionError":
            assert status == FAIL
            continue
        assert status == OK and picks == rec["picks"]
        assert [[c, f, sel[j], rem[j]] for j, (c, f) in enumerate(o.feat_names)] == rec["selected"]
        left = np.flatnonzero(present).astype(np.int32)
        assert (len(left), _sha(left)) == (rec["people_left_count"], rec["people_left_sha256"])


def test_python_oracle_refuses_a_chain_that_is_no_ring():
    _, o = oracle_instance(recipe_of(AC.LAUNCHABLE[0]))
    chain = list(range(o.n))
    chain[0], chain[1], chain[2] = 1, 2, 1          # 0 -> 1 -> 2 -> 1: never back at 0
    rng = PhiloxRng(SEED)
    with pytest.raises(ValueError):
        for panel in range(64):                     # some attempt picks agent 0
            draw_attempt(o, o.k, rng.for_attempt(panel, 0), addr_next=chain)


@pytest.mark.parametrize("cell", AC.LAUNCHABLE, ids=[c.name for c in AC.LAUNCHABLE])
def test_c_oracle_equals_python_oracle_with_households(cell):
    """Both ends of the batch and both sides of panel 2^32 (test_oracle_carries_the_panel_index's rows)."""
    _, o = oracle_instance(recipe_of(cell))
    ref = AC.reference_of(cell)
    ring = AC.ring_of(o.n)[0].tolist()
    S, carry = cell_S(cell), ref.carry
    for i in (0, carry - 2, carry - 1, carry, carry + 1, S - 1):
        picks, attempts = legacy_find(o, o.k, PhiloxRng(SEED), ref.begin + i, addr_next=ring)
        assert attempts == ref.attempts[i] and list(picks) == ref.picks[i].tolist(), i
    # the ring-free entry still draws the ring-free panels
    base = coracle.draw(o, o.k, SEED, ref.begin, 8, want_picks=True)
    assert not np.array_equal(base[3], ref.picks[:8])


def test_tally_is_optional_and_per_call():
    cell = AC.LAUNCHABLE[3]
    _, o = oracle_instance(recipe_of(cell))
    ring, ref = AC.ring_of(o.n)[0], AC.reference_of(cell)
    tally = np.full(2, 12345, np.uint64)
    rc, panels, attempts, _ = coracle.draw(o, o.k, SEED, ref.begin, 64, addr_next=ring, ring_tally=tally, threads=3)
    assert rc == 0 and np.array_equal(panels, ref.panels[:64]) and np.array_equal(attempts, ref.attempts[:64])
    assert 0 < tally[0] <= ref.ring_failures and 0 < tally[1] <= ref.cross_word
    # without rings nothing is tallied, and the panels are oracle_draw's
    rc, panels, _, _ = coracle.draw(o, o.k, SEED, ref.begin, 64, ring_tally=tally)
    assert rc == 0 and tally.tolist() == [0, 0]
    assert np.array_equal(panels, coracle.draw(o, o.k, SEED, ref.begin, 64)[1])
    bad = ring.copy()
    bad[5] = o.n
    assert coracle.draw(o, o.k, SEED, ref.begin, 4, addr_next=bad)[0] == 1      # OR_E_INVALID


def test_household_cells_meet_the_conditions():
    """Every launchable GENERAL cell with its households, on the oracle alone (the GPU cells assert the
    same again before they compare anything)."""
    for cell in AC.LAUNCHABLE:
        AC.check_conditions(cell)
    AC.check_ring_failures()
    assert len(AC.LAUNCHABLE) == 6 and len(AC.REFUSED) == 3
