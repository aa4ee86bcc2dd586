"""Households in the Monte Carlo run, everything that needs no GPU: the list of household kernels
(csa_draw_household_kernel_list) against the register cells of tests/household_cases.py, the route's argument
check, the household keywords' validation and refusals (which raise before an encoding or a device is
touched), stats.household_groups, and the cells' conditions on the C oracle alone.
"""
import csv
import ctypes
import os

import numpy as np
import pytest

import household_cases as HC
from conftest import REPO, inst_paths, pkg


def test_household_kernel_list_is_the_thirty_names():
    N = pkg("_native")
    built = N.household_kernel_list()
    want = ["draw_solo_hh_kernel<%d, %d, %s>" % (fn, wn, k8) for fn in (8, 16) for wn in (4, 8, 16, 28, 32)
            for k8 in ("true", "false")]
    want += ["draw_lane_hh_kernel<32, %d, %d, %s>" % (wn, wn // 2, k8) for wn in (4, 8, 16, 28, 32)
             for k8 in ("true", "false")]
    assert len(built) == 30 and sorted(built) == sorted(want)
    assert sorted(built) == HC.HOUSEHOLD_KERNELS             # every one has a cell that routes to it
    assert not set(built) & set(N.draw_kernel_list())        # a table of their own
    assert len(N.draw_kernel_list()) == 115


def test_household_kernel_list_reports_needed_size():
    N = pkg("_native")
    L = N.lib()
    need = len("\n".join(N.household_kernel_list())) + 2
    small = ctypes.create_string_buffer(need - 1)
    assert L.csa_draw_household_kernel_list(small, need - 1) == N.CSA_E_INVALID
    assert str(need) in N.last_error()
    assert L.csa_draw_household_kernel_list(None, 0) == N.CSA_E_INVALID
    exact = ctypes.create_string_buffer(need)
    assert L.csa_draw_household_kernel_list(exact, need) == N.CSA_OK
    assert exact.value.decode().splitlines() == N.household_kernel_list()


def test_route_arguments_are_checked_on_the_host():
    N = pkg("_native")
    L = N.lib()
    assert (N.CSA_ADDRESS_GENERAL, N.CSA_ADDRESS_BATCH) == (0, 1)
    # the route is checked before the handle is read
    for route in (-1, 2, 7):
        assert L.csa_instance_set_address_route(None, route) == N.CSA_E_INVALID
        assert "unknown address route %d" % route in N.last_error()
    assert L.csa_instance_set_address_route(None, N.CSA_ADDRESS_BATCH) == N.CSA_E_INVALID
    assert "null instance" in N.last_error()


def _small():
    P = pkg()
    inst = P.read_instance(*inst_paths("example_small_20"), 20)
    with open(os.path.join(REPO, "tests/golden/instances/example_small_20/addresses.csv"), encoding="utf-8") as fh:
        cols = {i: dict(r) for i, r in enumerate(csv.DictReader(fh))}
    return inst, cols


def _columns():
    import json
    with open(os.path.join(REPO, "tests/golden/address_example_small_20_s2.json")) as fh:
        return json.load(fh)["philox"]["columns"]


CALLS = ("legacy_probabilities", "legacy_composition", "legacy_panel_distribution", "legacy_panel_comparison",
         "legacy_maximin", "legacy_initial_committees")


def _call(name, inst, **kw):
    A = pkg("analysis")
    fn = getattr(A, name)
    if name == "legacy_composition":
        return fn(inst, 10, 0, object(), **kw)       # (the groups are checked after the keywords)
    if name == "legacy_panel_comparison":
        return fn(inst, 10, **kw)
    return fn(inst, 10, 0, **kw)


@pytest.fixture
def no_device(monkeypatch):
    """Nothing is encoded (an encoding creates the device handle) and the library is not asked."""
    A, I, N = pkg("analysis"), pkg("instance"), pkg("_native")

    def refuse(*a, **k):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(A, "encode_cached", refuse)
    monkeypatch.setattr(I, "encode_cached", refuse)
    monkeypatch.setattr(N, "lib", refuse)


@pytest.mark.parametrize("name", CALLS)
def test_keyword_validation_raises_before_any_device_call(no_device, name):
    inst, cols = _small()
    columns = _columns()
    with pytest.raises(ValueError, match="go together"):
        _call(name, inst, columns_data=cols)
    with pytest.raises(ValueError, match="go together"):
        _call(name, inst, check_same_address_columns=columns)
    with pytest.raises(ValueError, match="two columns"):
        _call(name, inst, columns_data=cols, check_same_address_columns=columns[:1])
    short = {a: r for a, r in cols.items() if a != next(iter(inst.agents))}
    with pytest.raises(ValueError, match="agent"):
        _call(name, inst, columns_data=short, check_same_address_columns=columns)
    with pytest.raises(ValueError, match="agent"):
        _call(name, inst, columns_data=cols, check_same_address_columns=[columns[0], "no such column"])


@pytest.mark.parametrize("name", CALLS)
def test_sharded_worlds_are_refused_by_name(no_device, monkeypatch, name):
    inst, cols = _small()
    monkeypatch.setattr(pkg("distributed"), "world_size", lambda: 2)
    with pytest.raises(ValueError, match=r"sharded runs \(world size 2\) are not offered"):
        _call(name, inst, columns_data=cols, check_same_address_columns=_columns())


def test_devices_are_refused_by_name(no_device):
    inst, cols = _small()
    with pytest.raises(ValueError, match="devices= is not offered"):
        pkg("analysis").legacy_probabilities(inst, 10, 0, devices=[0, 0], columns_data=cols,
                                             check_same_address_columns=_columns())


def test_price_and_cache_stay_without_the_keywords():
    import inspect
    A, C = pkg("analysis"), pkg("cache")
    for fn in (A.legacy_price, C.run_legacy_or_retrieve):
        assert "columns_data" not in inspect.signature(fn).parameters
    for name in CALLS:
        p = inspect.signature(getattr(A, name)).parameters
        assert p["columns_data"].default is None and p["check_same_address_columns"].default is None
        assert p["columns_data"].kind is p["check_same_address_columns"].kind is inspect.Parameter.KEYWORD_ONLY


def test_household_groups_are_the_rings_of_two_and_more():
    S, Lg = pkg("stats"), pkg("legacy")
    inst, cols = _small()
    columns = _columns()
    ids = list(inst.agents)
    ring = Lg.address_rings(ids, cols, columns)
    groups = S.household_groups(ids, cols, columns)
    n = len(ids)
    seen = np.zeros(n, bool)
    rings = []
    for p in range(n):
        if not seen[p]:
            members, q = [p], int(ring[p])
            while q != p:
                members.append(q)
                q = int(ring[q])
            seen[members] = True
            if len(members) >= 2:
                rings.append(sorted(members))
    assert len(groups) == len(rings) > 0 and groups.W == (n + 63) // 64
    assert groups.sizes.tolist() == [len(r) for r in rings]
    for g, members in enumerate(rings):
        bits = [p for p in range(n) if (int(groups.masks[g, p >> 6]) >> (p & 63)) & 1]
        assert bits == members
        assert groups.labels[g] == (cols[ids[members[0]]][columns[0]], cols[ids[members[0]]][columns[1]])


def test_light_ring_is_the_recipe():
    ring, label = HC.light_ring_of(250)
    order = np.random.default_rng(7).permutation(250)
    sizes = np.bincount(np.bincount(label))
    assert sizes[6] == 1 and sizes[2] == 40 and sizes[1] == 250 - 86 and sizes.sum() == 1 + 40 + 250 - 86
    assert set(np.flatnonzero(label == 0)) == set(order[:6].tolist())
    assert (ring[ring] == np.arange(250))[order[6:86]].all()          # the couples
    assert (ring == np.arange(250))[order[86:]].all()                  # the rest alone
    assert sorted(c.n for c in HC.REGISTER if c.name in HC.LIGHT) == [250] * 5
    assert all(c.k == 150 for c in HC.REGISTER if c.name in HC.LIGHT)
    assert [c.name for c in HC.REGISTER if c.n == 250 and c.k == 150] == sorted(
        HC.LIGHT, key=[c.name for c in HC.REGISTER].index)


def test_cells_meet_the_conditions_on_the_oracle():
    assert len(HC.REGISTER) == 70
    for cell in HC.REGISTER:
        HC.check_conditions(cell)
    HC.check_ring_failures()
    assert HC.reference_of(HC.BY_NAME[HC.SCARCE_SOLO]).ring_failures >= 20
    for name in HC.LIGHT:
        assert "  " + name + "\n" in HC.__doc__
    assert HC.SCARCE_SOLO in HC.__doc__
