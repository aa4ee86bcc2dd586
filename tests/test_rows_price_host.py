"""The pricing contracts in numpy (stats.rows_score_host, rows_price_host, rows_mw_cover_host,
rows_first_holder_host) against plain Python loops over unpacked member lists (price_cases), on the C oracle's
panels; PanelDistribution.price and initial_committees on host panels through HostRowTables; the argument checks
of the C entry points, which need no device.  Every assertion is integer or bit-for-bit float64 equality."""
import ctypes

import numpy as np
import pytest

import price_cases as P
from conftest import pkg

SMALL = ("example_small_20", 20, 0, 300)      # (instance, k, seed, S): 300 distinct rows of W = 4, n = 200


def _oracle(case=SMALL):
    name, k, seed, S = case
    _, ids = P.instance(name, k)
    panels, rows, first, mult = P.oracle_table(name, k, seed, S)
    return panels, rows, first, mult, ids


@pytest.mark.parametrize("kind", P.WEIGHTS)
@pytest.mark.parametrize("case", [SMALL, (P.COUPLES, 2, 0, 500), ("sf_e_110", 110, 0, 60)])
def test_score_mirror_is_the_loop(case, kind):
    """The score of every row, and the best row with ties, bit for bit; the order-sensitive weights do
    distinguish summation orders on these rows (asserted on the input)."""
    St = pkg("stats")
    _, rows, _, _, ids = _oracle(case)
    n = len(ids)
    w = P.weights(kind, n)
    if kind == "order" and case[1] > 2:
        P.assert_order_sensitive(rows, n, w)
    want = P.score_loop(P.members(rows, n), w)
    got = St.rows_score_host(rows, w)
    assert np.array_equal(P.bits(got), P.bits(want))
    at, value, sc = St.rows_price_host(rows, w)
    assert (at, P.bits1(value)) == (P.best_loop(want)[0], P.bits1(P.best_loop(want)[1]))
    assert np.array_equal(P.bits(sc), P.bits(want))
    if kind == "equal":
        assert at == 0 and len(set(P.bits(want).tolist())) == 1       # every score ties: row 0 wins
    assert St.rows_price_host(rows, w, 1 << 40)[0] == at + (1 << 40)


def test_price_mirror_empty_and_checks():
    St = pkg("stats")
    assert St.rows_price_host(np.zeros((0, 2), np.uint64), np.ones(100))[:2] == (P.PRICE_NONE, -np.inf)
    assert St.rows_price_host(np.zeros((0, 2), np.uint64), np.ones(100), 7, (12, 3.5))[:2] == (12, 3.5)
    with pytest.raises(ValueError):
        St.rows_score_host(np.zeros((3, 2), np.uint64), np.ones(129))
    with pytest.raises(ValueError):
        St.rows_score_host(np.zeros((3, 2), np.uint64), np.ones(0))


@pytest.mark.parametrize("kind", ["normal", "equal"])
def test_accumulate_gives_the_same_answer_for_any_cut(kind):
    """The oracle's 300 draws (not deduplicated: equal panels tie) priced in chunks from PRICE_NONE: every cut
    gives the whole's (index, value), the lowest draw index among ties."""
    St = pkg("stats")
    panels, _, _, _, ids = _oracle()
    w = P.weights(kind, len(ids))
    whole = St.rows_price_host(panels, w)[:2]
    assert whole == P.best_loop(P.score_loop(P.members(panels, len(ids)), w))
    for chunk in (1, 7, 100, 299, 300, 1000):
        best = (P.PRICE_NONE, -np.inf)
        for off in range(0, len(panels), chunk):
            best = St.rows_price_host(panels[off:off + chunk], w, off, best)[:2]
        assert best == whole, chunk
    # a carried best yields only to a strictly greater score
    tie = St.rows_price_host(panels, w, 1000, whole)[:2]
    assert tie == whole
    assert St.rows_price_host(panels, w, 1000, (5, -1e300))[:2] == (whole[0] + 1000, whole[1])


@pytest.mark.parametrize("case", [SMALL, (P.COUPLES, 2, 0, 500), ("sf_e_110", 110, 0, 60)])
def test_first_holder_mirror_is_the_loop(case):
    St = pkg("stats")
    _, rows, _, _, ids = _oracle(case)
    n = len(ids)
    want = P.first_holder_loop(P.members(rows, n), n)
    assert np.array_equal(St.rows_first_holder_host(rows, n), want)
    if case[0] == "sf_e_110":
        assert (want == P.NO_ROW).any() and (want != P.NO_ROW).any()
    assert St.rows_first_holder_host(rows[:0], n).tolist() == [P.NO_ROW] * n


@pytest.mark.parametrize("case,rounds", [((P.COUPLES, 2, 0, 500), 60), (SMALL, 40), (("sf_e_110", 110, 0, 60), 8)])
def test_mw_cover_mirror_is_the_transcription(case, rounds):
    """rows_mw_cover_host against the dict-based transcription of the update order: picks, final weight bits,
    chosen flags, pick scores; couples takes both branches (asserted); a second call continues the first."""
    St = pkg("stats")
    _, rows, _, _, ids = _oracle(case)
    n, W = len(ids), rows.shape[1]
    mem = P.members(rows, n)
    picks, w, chosen, scores, repeats = P.mw_cover_loop(mem, n, W, rounds)
    if case[0] == P.COUPLES:
        assert repeats > 0 and len(chosen) > 1
    got = St.rows_mw_cover_host(rows, np.ones(n), np.zeros(len(rows), np.uint8), rounds)
    assert got[0].tolist() == picks and np.array_equal(P.bits(got[1]), P.bits(w))
    assert set(np.flatnonzero(got[2]).tolist()) == chosen and np.array_equal(P.bits(got[3]), P.bits(scores))
    a = rounds // 3
    first = St.rows_mw_cover_host(rows, np.ones(n), np.zeros(len(rows), np.uint8), a)
    second = St.rows_mw_cover_host(rows, first[1], first[2], rounds - a)
    assert first[0].tolist() + second[0].tolist() == picks and np.array_equal(P.bits(second[1]), P.bits(w))
    assert np.array_equal(second[2], got[2])
    none = St.rows_mw_cover_host(rows, w, got[2], 0)
    assert len(none[0]) == 0 and np.array_equal(P.bits(none[1]), P.bits(w)) and np.array_equal(none[2], got[2])
    empty = St.rows_mw_cover_host(rows[:0], w, np.zeros(0, np.uint8), 3)
    assert empty[0].tolist() == [P.NO_ROW] * 3 and np.array_equal(P.bits(empty[1]), P.bits(w))


def test_weight_sum_is_lane_strided():
    """n = 1727 (a ragged last 64-block): the mirror's sum is the lane-strided one, and differs from a
    left-to-right sum in the bits for these weights."""
    St = pkg("stats")
    w = P.weights("normal", 1727)
    partial = [0.0] * 64
    for j in range(27):
        for lane in range(64):
            partial[lane] = partial[lane] + (float(w[64 * j + lane]) if 64 * j + lane < 1727 else 0.0)
    total = 0.0
    for x in partial:
        total = total + x
    flat = 0.0
    for x in w.tolist():
        flat = flat + x
    assert P.bits1(St.weights_sum_host(w, 27)) == P.bits1(total) != P.bits1(flat)


def _distribution(panels, n, ids):
    St = pkg("stats")
    first, mult = St.panel_multiplicities_host(panels)
    return St.PanelDistribution(len(panels), first, mult, panels, n, ids)


@pytest.mark.parametrize("kind", ["normal", "equal", "order"])
def test_distribution_price_on_host_panels(kind):
    St = pkg("stats")
    panels, rows, first, mult, ids = _oracle()
    n = len(ids)
    dist = _distribution(panels, n, ids)
    w = P.weights(kind, n)
    mem = P.members(rows, n)
    scores = P.score_loop(mem, w)
    at, value = P.best_loop(scores)
    for given in (w.tolist(), dict(zip(ids, w.tolist()))):
        got, sc = dist.price(given, scores=True)
        assert isinstance(got, St.PanelPrice) and dist.price(given) == got
        assert got.panel == frozenset(ids[i] for i in mem[at]) and P.bits1(got.value) == P.bits1(value)
        assert (got.row, got.first, got.multiplicity) == (at, first[at], mult[at])
        assert np.array_equal(P.bits(sc), P.bits(scores))
    assert not St._is_device_tensor(dist.table().rows)


def test_distribution_price_refusals():
    St = pkg("stats")
    panels, _, _, _, ids = _oracle()
    dist = _distribution(panels, len(ids), ids)
    w = P.weights("normal", len(ids))
    for bad in (np.nan, np.inf, -np.inf):
        broken = w.copy()
        broken[17] = bad
        with pytest.raises(ValueError):
            dist.price(broken)
    with pytest.raises(ValueError):
        dist.price(w[:-1])
    missing = dict(zip(ids, w.tolist()))
    del missing[ids[5]]
    with pytest.raises(KeyError):
        dist.price(missing)
    empty = St.PanelDistribution(0, np.zeros(0, np.int64), np.zeros(0, np.int64), panels[:0], len(ids), ids)
    assert empty.price(w) == St.PanelPrice(frozenset(), -np.inf, None, None, 0)
    lines = ["Agent %s not contained in any drawn panel." % (a,) for a in ids]
    assert empty.initial_committees(5) == (set(), frozenset(), lines)


@pytest.mark.parametrize("case,rounds", [((P.COUPLES, 2, 0, 500), None), (SMALL, 40), (("sf_e_110", 110, 0, 60), 8)])
def test_distribution_initial_committees_on_host_panels(case, rounds):
    """The reference's return shape from the transcription's picks: committees, covered set, lines; couples runs
    the default 3 n rounds and covers everyone, sf_e's 60 draws leave agents no panel holds."""
    panels, rows, _, _, ids = _oracle(case)
    n = len(ids)
    mem = P.members(rows, n)
    picks = P.mw_cover_loop(mem, n, rows.shape[1], 3 * n if rounds is None else rounds)[0]
    want = P.committees_loop(mem, n, ids, picks)
    got = _distribution(panels, n, ids).initial_committees(rounds)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert isinstance(got[0], set) and isinstance(got[1], frozenset) and all(isinstance(c, frozenset) for c in got[0])
    if case[0] == "sf_e_110":
        assert any("not contained" in line for line in got[2]) and len(got[0]) > len(set(picks))
    else:
        assert got[2] == ["All agents are contained in some drawn panel."]


def test_entry_points_refuse_bad_arguments_without_a_device():
    """n > 64 W, n <= 0, a short scratch, a NULL length: an error code and csa_last_error, before any device call."""
    N = pkg("_native")
    L = N.lib()
    T = int(L.csa_rows_price_tile())
    assert T >= 64 and int(L.csa_rows_price_scratch_bytes(3 * T + 5, 2)) >= 4 * 16
    assert N.CSA_PRICE_NONE == 2 ** 64 - 1 and N.CSA_PRICE_ACCUMULATE == 1
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = int(L.csa_rows_price_scratch_bytes(4, 2))
    for n in (129, 0, -3):
        assert L.csa_rows_price_async(p, p, 4, 2, n, p, 0, 0, None, p, p, need, None) == N.CSA_E_INVALID
        assert "rows price" in N.last_error()
        assert L.csa_rows_mw_cover_async(p, p, 4, 2, n, 1, p, p, p, None, p, need, None) == N.CSA_E_INVALID
        assert "rows mw cover" in N.last_error()
        assert L.csa_rows_first_holder_async(p, p, 4, 2, n, p, None) == N.CSA_E_INVALID
        assert "rows first holder" in N.last_error()
    assert L.csa_rows_price_async(p, p, 4, 2, 100, p, 0, 0, None, p, p, need - 1, None) == N.CSA_E_INVALID
    assert "scratch" in N.last_error()
    assert L.csa_rows_mw_cover_async(p, p, 4, 2, 100, 1, p, p, p, None, p, need - 1, None) == N.CSA_E_INVALID
    assert L.csa_rows_price_async(p, None, 4, 2, 100, p, 0, 0, None, p, p, need, None) == N.CSA_E_INVALID
    assert L.csa_rows_price_async(p, p, 4, 2, 100, p, 0, 2, None, p, p, need, None) == N.CSA_E_INVALID
    assert L.csa_rows_price_async(p, p, 2 ** 32, 2, 100, p, 0, 0, None, p, p, 1 << 40, None) == N.CSA_E_UNSUPPORTED


def test_world_beyond_one_is_refused(monkeypatch):
    A, D = pkg("analysis"), pkg("distributed")
    inst, ids = P.instance("example_small_20", 20)
    monkeypatch.setattr(D, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size 2"):
        A.legacy_price(inst, [1.0] * len(ids), 10, 0)
    with pytest.raises(NotImplementedError, match="world size 2"):
        A.legacy_initial_committees(inst, 10, 0)


def test_names_are_exported():
    top = pkg()
    for name in ("legacy_initial_committees", "legacy_price", "PanelPrice", "rows_score_host", "rows_price_host",
                 "rows_mw_cover_host", "rows_first_holder_host"):
        assert name in top.__all__ and hasattr(top, name)
