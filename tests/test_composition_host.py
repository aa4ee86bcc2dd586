"""Group composition, host side: the group builders, the numpy implementation of csa_group_hist_async's
contract, CompositionHistogram, and the intersectional-representation numbers against the reference's
own outputs (tests/golden/intersections_sf_e_110.json).  No GPU."""
import ctypes
import json
import os
import pickle
import re

import numpy as np
import pytest

from conftest import GOLD, golden, inst_paths, pkg

FIXTURE = os.path.join(GOLD, "sf_e_110_intersections.csv")


def _instance(name, k):
    cat, resp = inst_paths(name)
    return pkg().read_instance(cat, resp, k)


@pytest.fixture(scope="module")
def sf_e():
    return _instance("sf_e_110", 110)


@pytest.fixture(scope="module")
def small():
    return _instance("example_small_20", 20)


def _mask_of(members, W):
    """Brute force: one bit per member, set one at a time with Python ints."""
    words = [0] * W
    for p in members:
        words[p >> 6] |= 1 << (p & 63)
    return np.array(words, np.uint64)


def _check_groups(gs, expected_members, n):
    W = (n + 63) // 64
    assert gs.masks.shape == (len(expected_members), W) and gs.masks.dtype == np.uint64
    assert len(gs) == len(gs.labels) == len(expected_members)
    for g, members in enumerate(expected_members):
        assert np.array_equal(gs.masks[g], _mask_of(members, W)), gs.labels[g]
        assert int(gs.sizes[g]) == len(members)
    if n & 63:      # padding bits of the last word are zero
        assert not np.any(gs.masks[:, -1] >> np.uint64(n & 63))


def _rows(path):
    S = pkg("stats")
    return S.read_intersections(path)


@pytest.mark.parametrize("which", ["small", "sf_e"])
def test_feature_groups_brute_force(which, request):
    inst = request.getfixturevalue(which)
    S = pkg("stats")
    gs = S.feature_groups(inst)
    enc = pkg().encode(inst.categories, inst.agents)
    assert gs.labels == enc.feat_keys
    ids = list(inst.agents)
    expected = [[p for p, aid in enumerate(ids) if inst.agents[aid][cat] == feat] for cat, feat in gs.labels]
    _check_groups(gs, expected, len(ids))
    # every agent holds one feature per category
    assert int(gs.sizes.sum()) == len(ids) * len(inst.categories)


def test_intersection_groups_fixture(sf_e):
    S = pkg("stats")
    gs = S.intersection_groups(sf_e, FIXTURE)
    rows = _rows(FIXTURE)
    assert len(gs) == len(rows) == 346
    ids = list(sf_e.agents)
    n = len(ids)
    expected = [[p for p, aid in enumerate(ids)
                 if sf_e.agents[aid][a[0]] == a[1] and sf_e.agents[aid][b[0]] == b[1]] for a, b, _ in rows]
    _check_groups(gs, expected, n)
    assert gs.labels == [(a, b) for a, b, _ in rows]
    assert int((gs.sizes == 0).sum()) == 12                     # empty groups are kept
    assert int(gs.sizes.min()) == 0 and int(gs.sizes.max()) == 1095
    # the same from an iterable of pairs
    again = S.intersection_groups(sf_e, [(a, b) for a, b, _ in rows])
    assert np.array_equal(again.masks, gs.masks) and again.labels == gs.labels
    # the last agent (bit n - 1 of the last word) is in the groups its two features name
    last = sf_e.agents[ids[-1]]
    bit = np.uint64(1) << np.uint64((n - 1) & 63)
    holds = [bool(gs.masks[g, -1] & bit) for g in range(len(gs))]
    assert holds == [last[a[0]] == a[1] and last[b[0]] == b[1] for a, b, _ in rows]
    assert any(holds)


def test_intersection_groups_small(small):
    S = pkg("stats")
    cats = list(small.categories)
    pairs = [((cats[0], f0), (cats[1], f1)) for f0 in small.categories[cats[0]] for f1 in small.categories[cats[1]]]
    gs = S.intersection_groups(small, pairs)
    ids = list(small.agents)
    expected = [[p for p, aid in enumerate(ids) if small.agents[aid][a[0]] == a[1] and small.agents[aid][b[0]] == b[1]]
                for a, b in pairs]
    _check_groups(gs, expected, len(ids))
    assert int(gs.sizes.sum()) == len(ids)      # the cells of two categories partition the pool


def test_unknown_feature_or_category_raises(sf_e):
    S = pkg("stats")
    cat = next(iter(sf_e.categories))
    feat = next(iter(sf_e.categories[cat]))
    with pytest.raises(KeyError):
        S.intersection_groups(sf_e, [((cat, feat), (cat, "no such feature"))])
    with pytest.raises(KeyError):
        S.intersection_groups(sf_e, [(("no such category", feat), (cat, feat))])
    with pytest.raises(KeyError):
        S.agent_groups(sf_e, {"x": ["no such agent"]})


def test_agent_groups_and_concatenation(sf_e):
    S = pkg("stats")
    ids = list(sf_e.agents)
    n = len(ids)
    sets = {"first": [ids[0]], "last": [ids[-1]], "ends": [ids[0], ids[63], ids[64], ids[-1]], "none": [],
            "all": ids}
    gs = S.agent_groups(sf_e, sets)
    _check_groups(gs, [[0], [n - 1], [0, 63, 64, n - 1], [], list(range(n))], n)
    assert gs.labels == list(sets)
    assert gs.masks[1, -1] == np.uint64(1) << np.uint64((n - 1) & 63) and not gs.masks[1, :-1].any()
    both = S.feature_groups(sf_e) + gs
    assert len(both) == len(S.feature_groups(sf_e)) + 5 and both.labels[-5:] == list(sets)
    assert np.array_equal(both.masks[-5:], gs.masks) and np.array_equal(both.sizes[-5:], gs.sizes)
    with pytest.raises(ValueError):
        both + S.GroupSet(["x"], np.zeros((1, gs.W + 1), np.uint64))


def _pack(panels, W):
    return np.stack([_mask_of(p, W) for p in panels]) if len(panels) else np.zeros((0, W), np.uint64)


@pytest.mark.parametrize("case,name,k", [("example_small_20_s0", "example_small_20", 20),
                                         ("sf_e_110_s0", "sf_e_110", 110)])
def test_host_group_composition_brute_force(case, name, k):
    S = pkg("stats")
    inst = _instance(name, k)
    first = golden(case)["first_panels"]
    n = len(inst.agents)
    groups = S.feature_groups(inst)
    if name == "sf_e_110":
        groups = groups + S.intersection_groups(inst, FIXTURE)
    packed = _pack(first, groups.W)
    comp = S.group_composition(groups, packed, k)
    assert comp.counts.shape == (len(groups), k + 1) and comp.counts.dtype == np.int64
    assert comp.S == len(first) and comp.k == k and comp.labels == groups.labels
    expect = np.zeros((len(groups), k + 1), np.int64)
    member_sets = [set(pkg("instance").unpack_panel(m, n)) for m in groups.masks]
    for panel in first:
        for g, members in enumerate(member_sets):
            expect[g, sum(1 for p in panel if p in members)] += 1
    assert np.array_equal(comp.counts, expect)
    assert np.array_equal(comp.counts.sum(axis=1), np.full(len(groups), len(first)))


def test_host_group_hist_contract():
    S, N = pkg("stats"), pkg("_native")
    masks = np.array([[0x0F, 0], [0, 0], [0xFFFFFFFFFFFFFFFF, 0xFF]], np.uint64)
    panels = np.array([[0x03, 0x01], [0, 0], [0x03, 0x01], [0xF0, 0xFF]], np.uint64)
    hist = S.group_hist_host(masks, panels, 13)
    expect = np.zeros((3, 13), np.int64)
    for a, b, c in ((2, 0, 3), (0, 0, 0), (2, 0, 3), (0, 0, 12)):
        expect[0, a] += 1
        expect[1, b] += 1
        expect[2, c] += 1
    assert np.array_equal(hist, expect)
    assert S.group_hist_host(masks, panels[:0], 5).shape == (3, 5)
    assert S.group_hist_host(masks[:0], panels, 5).shape == (0, 5)
    with pytest.raises(N.CsaError) as e:           # count 12 with 12 bins: refused, as the device does
        S.group_hist_host(masks, panels, 12)
    assert e.value.code == N.CSA_E_INVALID


def test_composition_histogram_values_merge_pickle():
    S = pkg("stats")
    counts = np.array([[2, 0, 6, 0], [0, 0, 0, 8], [8, 0, 0, 0], [1, 3, 3, 1]], np.int64)
    h = S.CompositionHistogram(["a", "b", "c", "d"], counts, 8, 3)
    assert np.array_equal(h.probabilities(), counts / 8)
    assert h.mean().tolist() == [1.5, 3.0, 0.0, 1.5]
    assert h.panel_share().tolist() == [0.5, 1.0, 0.0, 0.5]
    assert h.variance().tolist() == [0.75, 0.0, 0.0, 0.75]
    assert h.prob_absent().tolist() == [0.25, 0.0, 1.0, 0.125]
    lo, hi = h.support()
    assert lo.tolist() == [0, 3, 0, 0] and hi.tolist() == [2, 3, 0, 3]
    other = S.CompositionHistogram(["a", "b", "c", "d"], counts[::-1].copy(), 8, 3)
    both = h + other
    assert np.array_equal(both.counts, counts + counts[::-1]) and both.S == 16 and both.k == 3
    assert both.counts.dtype == np.int64
    with pytest.raises(ValueError):
        h + S.CompositionHistogram(["a", "b", "c", "e"], counts, 8, 3)
    with pytest.raises(ValueError):
        h + S.CompositionHistogram(["a", "b", "c", "d"], np.zeros((4, 5), np.int64), 8, 4)
    back = pickle.loads(pickle.dumps(both))
    assert back.labels == both.labels and back.S == 16 and back.k == 3
    assert isinstance(back.counts, np.ndarray) and np.array_equal(back.counts, both.counts)
    empty = S.CompositionHistogram(["a"], np.zeros((1, 4), np.int64), 0, 3)
    assert [x.tolist() for x in empty.support()] == [[-1], [-1]]


def test_intersectional_representation_bit_equal(sf_e):
    S = pkg("stats")
    with open(os.path.join(GOLD, "intersections_sf_e_110.json")) as fh:
        gold = json.load(fh)
    g = golden("sf_e_110_s0")
    ids = list(sf_e.agents)
    legacy_alloc = {aid: c / g["S"] for aid, c in zip(ids, g["counts"])}
    lex = np.load(os.path.join(GOLD, "portfolio_sf_e_110.npz"))["alloc"]
    leximin_alloc = {aid: float(x) for aid, x in zip(ids, lex)}
    table, errors = S.intersectional_representation(sf_e, legacy_alloc, leximin_alloc, FIXTURE)
    assert len(table["labels"]) == gold["rows"] == 346
    assert set(gold["shares"]) == set(S.INTERSECTION_SHARES)
    for name in S.INTERSECTION_SHARES:
        assert table[name].dtype == np.float64
        assert table[name].tolist() == gold["shares"][name], name         # every share, bit for bit
    assert [[a, b] for a, b in errors] == [[a, b] for a, b, _ in gold["mse"]]   # the reference's keys and order
    assert [errors[(a, b)] for a, b, _ in gold["mse"]] == [v for _, _, v in gold["mse"]]
    assert len(errors) == 7
    # rows given directly answer the same
    table2, errors2 = S.intersectional_representation(sf_e, legacy_alloc, leximin_alloc, _rows(FIXTURE))
    assert errors2 == errors and all(np.array_equal(table2[c], table[c]) for c in S.INTERSECTION_SHARES)


def test_intersectional_representation_missing_path(sf_e, tmp_path):
    S = pkg("stats")
    assert S.intersectional_representation(sf_e, {}, {}, str(tmp_path / "intersections.csv")) is None


C_TYPES = {"const uint64_t *": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32,
           "int64_t *": ctypes.c_void_p, "uint32_t *": ctypes.c_void_p, "void *": ctypes.c_void_p}


def test_group_hist_symbol_declared_as_bound():
    N = pkg("_native")
    with open(N.HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+csa_group_hist_async\s*\(([^)]*)\)\s*;", text)
    assert m, "csa_group_hist_async is not declared in include/csa_legacy.h"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        args.append(C_TYPES[re.match(r"(.*?)\w+$", a).group(1).strip()])
    res, bound = N.SIGNATURES["csa_group_hist_async"]
    assert res is ctypes.c_int and bound == args and len(args) == 9
    assert hasattr(N.lib(), "csa_group_hist_async")
    # host-side argument checks, before any device call
    L = N.lib()
    assert L.csa_group_hist_async(None, 5, 0, None, 1, 3, None, None, None) == N.CSA_E_INVALID
    assert L.csa_group_hist_async(None, 5, 2, None, 1, 0, None, None, None) == N.CSA_E_INVALID
    assert L.csa_group_hist_async(None, 5, 2, None, -1, 3, None, None, None) == N.CSA_E_INVALID
    assert L.csa_group_hist_async(None, 0, 2, None, 4, 3, None, None, None) == N.CSA_OK      # no panels: no-op
    assert L.csa_group_hist_async(None, 5, 2, None, 0, 3, None, None, None) == N.CSA_OK      # no groups: no-op
    assert L.csa_group_hist_async(None, 5, 2, None, 4, 3, None, None, None) == N.CSA_E_INVALID
    one = ctypes.c_uint64(0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)
    assert L.csa_group_hist_async(p, 5, 8193, p, 4, 3, p, p, None) == N.CSA_E_UNSUPPORTED      # refused before launch
    assert "8192" in N.last_error()
