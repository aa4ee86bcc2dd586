"""Pricing on the device: csa_rows_price_async (rp_score_kernel, rp_best_kernel), csa_rows_mw_cover_async
(rp_round_kernel between score passes) and csa_rows_first_holder_async through the C ABI, and the product paths
on them -- PanelDistribution.price / initial_committees over a run's device table, legacy_initial_committees,
legacy_price over fresh draws.

Expected values come from the numpy mirrors (stats.rows_*_host, themselves checked against plain Python loops in
test_rows_price_host.py) and the C oracle's panels.  Every assertion is integer or bit-for-bit float64 equality;
every buffer the calls read or write carries guard words behind it."""
import numpy as np
import pytest

import price_cases as P
import rows_cases as R
from conftest import pkg
from test_gpu_rows_sort import GUARD, GUARD32, GUARD64, _dev64, _guards_ok

pytestmark = pytest.mark.gpu

NEG_INF_BITS = 0xFFF0000000000000
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _tile():
    return int(pkg("_native").lib().csa_rows_price_tile())


def _lengths(T):
    return [0, 1, 2, T - 1, T, T + 1, 3 * T + 5]


def _shapes(W):
    return [64 * W, 64 * W - 37 if W > 1 else 27]


def _table(rows, length, cap, W):
    """The first ``length`` rows in a table of ``cap`` rows whose other rows are all ones (scoring one would
    win, holding one would count), guard words behind; and the length word."""
    full = np.full((cap, W), ONES, np.uint64)
    full[:length] = rows[:length]
    return (_dev64(full, GUARD) if cap else None), _dev64(np.array([length], np.uint64), GUARD)


def _scratch(cap, W):
    import torch
    need = int(pkg("_native").lib().csa_rows_price_scratch_bytes(cap, W))
    assert need % 8 == 0
    return torch.full((need // 8 + GUARD,), GUARD64, dtype=torch.int64, device="cuda"), need


def _price(rows, length, cap, W, n, w, index_base=0, best=None, scores=True):
    """One csa_rows_price_async call; ``best`` = a stored (index, value): accumulate onto it.  Returns
    (index, value bits, score bits of the valid rows or None) after checking every guard, that no score past the
    length was written, and that the inputs are unchanged."""
    import torch
    N = pkg("_native")
    L = N.lib()
    d_rows, d_len = _table(rows, length, cap, W)
    d_w = _dev64(P.bits(w), GUARD)
    scratch, need = _scratch(cap, W)
    d_scores = torch.full((cap + GUARD,), GUARD64, dtype=torch.int64, device="cuda") if scores else None
    stored = np.array([0x1111, 0x2222] if best is None else [best[0], P.bits1(best[1])], np.uint64)
    d_best = _dev64(stored, GUARD)
    N.check(L.csa_rows_price_async(N.ptr(d_rows), N.ptr(d_len), cap, W, n, N.ptr(d_w), index_base,
                                   0 if best is None else N.CSA_PRICE_ACCUMULATE, N.ptr(d_scores), N.ptr(d_best),
                                   N.ptr(scratch), need, None))
    torch.cuda.synchronize()
    assert _guards_ok(scratch, need // 8, GUARD64) and _guards_ok(d_best, 2, GUARD64)
    assert _guards_ok(d_len, 1, GUARD64) and int(d_len[0].item()) == length
    assert np.array_equal(d_w.cpu().numpy()[:n].view(np.uint64), P.bits(w)) and _guards_ok(d_w, n, GUARD64)
    if cap:
        assert _guards_ok(d_rows, cap * W, GUARD64)
        assert np.array_equal(d_rows[:length * W].cpu().numpy().view(np.uint64).reshape(length, W), rows[:length])
    out = d_best[:2].cpu().numpy().view(np.uint64)
    sc = None
    if scores:
        assert _guards_ok(d_scores, length, GUARD64)          # nothing past the length, guards included
        sc = d_scores[:length].cpu().numpy().view(np.uint64)
    return int(out[0]), int(out[1]), sc


@pytest.mark.parametrize("W", R.WIDTHS)
def test_scores_and_best(gpu_available, W):
    """Every length around the tile, both agent counts, all four weight cases: the scores of the valid rows and
    the best (index, value) are the mirror's bits; rows past the length are all ones and never scored; a NULL
    d_scores gives the same best; all-equal weights make every score tie and row 0 win."""
    St = pkg("stats")
    T = _tile()
    for n in _shapes(W):
        rows = P.subset_rows(3 * T + 5, W, n)
        for kind in P.WEIGHTS:
            w = P.weights(kind, n)
            if kind == "order" and n > 27:
                P.assert_order_sensitive(rows[:64], n, w)
            want = St.rows_score_host(rows, w)
            for length in _lengths(T):
                at, value = P.best_loop(want[:length])
                got = _price(rows, length, length + 3, W, n, w)
                assert np.array_equal(got[2], P.bits(want[:length])), (W, n, kind, length)
                assert got[:2] == (at, P.bits1(value)), (W, n, kind, length)
                assert _price(rows, length, length + 3, W, n, w, scores=False)[:2] == got[:2], (W, n, kind, length)
                if kind == "equal" and length:
                    assert at == 0 and len(set(got[2].tolist())) == 1
                if length == 0:
                    assert got[:2] == (P.PRICE_NONE, NEG_INF_BITS)
        # cap == length, and an index base beyond 32 bits
        w = P.weights("normal", n)
        at, value = P.best_loop(St.rows_score_host(rows, w))
        assert _price(rows, len(rows), len(rows), W, n, w, index_base=1 << 40)[:2] == (at + (1 << 40), P.bits1(value))


def test_empty_capacity(gpu_available):
    """cap == 0 with NULL rows: CSA_PRICE_NONE and -inf; accumulating, the stored pair stays."""
    w = P.weights("normal", 100)
    none = np.zeros((0, 2), np.uint64)
    assert _price(none, 0, 0, 2, 100, w)[:2] == (P.PRICE_NONE, NEG_INF_BITS)
    assert _price(none, 0, 0, 2, 100, w, best=(77, 1.5))[:2] == (77, P.bits1(1.5))
    assert _price(none, 0, 5, 2, 100, w, best=(P.PRICE_NONE, 0.0))[0] == P.PRICE_NONE


@pytest.mark.parametrize("W", [1, 27])
def test_accumulate_over_chunks(gpu_available, W):
    """Three chunks priced in turn onto a carried best that starts as CSA_PRICE_NONE.  No random row holds agent
    0, whose weight dwarfs the others, so a row given agent 0 is the maximum: planted in the first chunk and in
    the third, each alone -- a carried best that is lost or wrongly replaced shows -- and as equal rows in the
    second and third, where the second must win.  Each equals the mirror over the whole, for these cuts."""
    St = pkg("stats")
    T = _tile()
    n = 64 * W - 5
    sizes = [T + 1, T - 1, 70]
    offs = [0, sizes[0], sizes[0] + sizes[1]]
    total = sum(sizes)
    base = P.subset_rows(total, W, n, low=1)
    w = P.weights("normal", n)
    w[0] = 1e6
    for name, plants in (("first", [(0, 17)]), ("third", [(2, 33)]), ("tie", [(1, T - 2), (2, 5)])):
        rows = base.copy()
        for c, r in plants:
            rows[offs[c] + r] = base[7]
            rows[offs[c] + r, 0] |= np.uint64(1)
        whole = St.rows_price_host(rows, w)[:2]
        assert whole[0] == offs[plants[0][0]] + plants[0][1], name
        best = (P.PRICE_NONE, -np.inf)
        for off, size in zip(offs, sizes):
            at, value_bits, _ = _price(rows[off:off + size], size, size + 2, W, n, w, index_base=off, best=best,
                                       scores=False)
            best = (at, float(np.array([value_bits], np.uint64).view(np.float64)[0]))
        assert best == whole, name
        # an index base of 2^40 carried through the same cuts
        best = (P.PRICE_NONE, -np.inf)
        for off, size in zip(offs, sizes):
            at, value_bits, _ = _price(rows[off:off + size], size, size, W, n, w, index_base=(1 << 40) + off, best=best,
                                       scores=False)
            best = (at, float(np.array([value_bits], np.uint64).view(np.float64)[0]))
        assert best == (whole[0] + (1 << 40), whole[1]), name
    # a stored best with a greater score survives a whole table
    assert _price(base, total, total, W, n, w, best=(123456789, 1e9), scores=False)[:2] == (123456789, P.bits1(1e9))


def _first_holder(rows, length, cap, W, n):
    import torch
    N = pkg("_native")
    d_rows, d_len = _table(rows, length, cap, W)
    out = torch.full((n + GUARD,), GUARD32, dtype=torch.int32, device="cuda")
    N.check(N.lib().csa_rows_first_holder_async(N.ptr(d_rows), N.ptr(d_len), cap, W, n, N.ptr(out), None))
    torch.cuda.synchronize()
    assert _guards_ok(out, n, GUARD32) and _guards_ok(d_len, 1, GUARD64)
    assert d_rows is None or _guards_ok(d_rows, cap * W, GUARD64)
    return out[:n].cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("W", R.WIDTHS)
def test_first_holder(gpu_available, W):
    """The same shapes.  Agent a0 is held by no valid row, a1 only by the last valid row, and the all-ones rows
    past the length hold everyone: a0 stays 0xFFFFFFFF, a1 is length - 1, the rest is the mirror's."""
    St = pkg("stats")
    T = _tile()
    for n in _shapes(W):
        a0, a1 = n - 1, n // 2
        base = P.subset_rows(3 * T + 5, W, n)
        for a in (a0, a1):
            base[:, a >> 6] &= ~(np.uint64(1) << np.uint64(a & 63))
        for length in _lengths(T):
            rows = base[:length].copy()
            if length:
                rows[length - 1, a1 >> 6] |= np.uint64(1) << np.uint64(a1 & 63)
            want = St.rows_first_holder_host(rows, n) if length else np.full(n, P.NO_ROW, np.int64)
            got = _first_holder(rows, length, length + 3, W, n)
            assert np.array_equal(got, want), (W, n, length)
            assert got[a0] == P.NO_ROW and got[a1] == (length - 1 if length else P.NO_ROW)
    assert _first_holder(base[:0], 0, 0, W, n).tolist() == [P.NO_ROW] * n


def _mw_cover(rows, cap, W, n, rounds, w, chosen, pick_scores=True, length=None):
    """One csa_rows_mw_cover_async call; returns (picks, weight bits, chosen, pick score bits or None)."""
    import torch
    N = pkg("_native")
    length = len(rows) if length is None else length
    d_rows, d_len = _table(rows, length, cap, W)
    d_w = _dev64(P.bits(w), GUARD)
    ch = np.zeros(cap, np.uint8)
    ch[:len(chosen)] = chosen
    d_ch = torch.full((cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    d_ch[:cap] = torch.from_numpy(ch)
    picks = torch.full((rounds + GUARD,), GUARD32, dtype=torch.int32, device="cuda")
    ps = torch.full((rounds + GUARD,), GUARD64, dtype=torch.int64, device="cuda") if pick_scores else None
    scratch, need = _scratch(cap, W)
    N.check(N.lib().csa_rows_mw_cover_async(N.ptr(d_rows), N.ptr(d_len), cap, W, n, rounds, N.ptr(d_w), N.ptr(d_ch),
                                            N.ptr(picks), N.ptr(ps), N.ptr(scratch), need, None))
    torch.cuda.synchronize()
    assert _guards_ok(d_w, n, GUARD64) and _guards_ok(d_ch, cap, 0x5A) and _guards_ok(picks, rounds, GUARD32)
    assert _guards_ok(scratch, need // 8, GUARD64) and _guards_ok(d_len, 1, GUARD64)
    assert ps is None or _guards_ok(ps, rounds, GUARD64)
    assert d_rows is None or _guards_ok(d_rows, cap * W, GUARD64)
    return (picks[:rounds].cpu().numpy().view(np.uint32).astype(np.int64), d_w[:n].cpu().numpy().view(np.uint64),
            d_ch[:cap].cpu().numpy(), None if ps is None else ps[:rounds].cpu().numpy().view(np.uint64))


def _check_cover(got, want, length):
    picks, w, chosen, scores = want
    assert got[0].tolist() == picks.tolist()
    assert np.array_equal(got[1], P.bits(w))
    assert np.array_equal(got[2][:length], chosen) and not got[2][length:].any()
    assert got[3] is None or np.array_equal(got[3], P.bits(scores))


@pytest.mark.parametrize("table", sorted(P.COVER_TABLES))
def test_mw_cover_on_oracle_tables(gpu_available, table):
    """Picks, final weight bits, chosen flags and pick scores equal the mirror's on the C oracle's distinct
    panels; rounds that re-pick a chosen row and rounds that pick a fresh one both occurred (asserted from the
    mirror); all-ones rows past the length are never picked."""
    c = P.cover(table)
    rows, n, rounds = c["rows"], c["n"], c["rounds"]
    assert len(rows) == {"example_small_20": 3000, "couples": 98, "sf_e_110": 300}[table]
    if table != "sf_e_110":       # sf_e's 60 rounds all pick fresh rows: it is here for W = 27 and the ragged n
        assert 0 < c["repeats"] < rounds
    D, W = rows.shape
    got = _mw_cover(rows, D + 3, W, n, rounds, np.ones(n), np.zeros(D, np.uint8))
    _check_cover(got, (c["picks"], c["weights"], c["chosen"], c["scores"]), D)


def test_mw_cover_pick_crosses_workgroups(gpu_available):
    """W = 2, 3 T + 5 rows: the picks come from more than one score tile (asserted from the mirror)."""
    St = pkg("stats")
    T = _tile()
    n, W, rounds = 128 - 37, 2, 40
    rows = P.subset_rows(3 * T + 5, W, n, k=9)
    want = St.rows_mw_cover_host(rows, np.ones(n), np.zeros(len(rows), np.uint8), rounds)
    assert len({p // T for p in want[0].tolist()}) > 1
    _check_cover(_mw_cover(rows, len(rows), W, n, rounds, np.ones(n), np.zeros(len(rows), np.uint8)), want, len(rows))
    got = _mw_cover(rows, len(rows), W, n, rounds, np.ones(n), np.zeros(len(rows), np.uint8), pick_scores=False)
    _check_cover(got, want, len(rows))


def test_mw_cover_continues_and_degenerates(gpu_available):
    """Two calls, the second from the first's weights and chosen flags, equal one call of the summed rounds;
    rounds = 0 changes nothing; an empty table leaves the weights alone and picks 0xFFFFFFFF."""
    c = P.cover("couples")
    rows, n, rounds = c["rows"], c["n"], c["rounds"]
    D, W = rows.shape
    a = 23
    first = _mw_cover(rows, D, W, n, a, np.ones(n), np.zeros(D, np.uint8))
    assert first[0].tolist() == c["picks"][:a].tolist()
    second = _mw_cover(rows, D, W, n, rounds - a, first[1].view(np.float64), first[2])
    assert first[0].tolist() + second[0].tolist() == c["picks"].tolist()
    assert np.array_equal(second[1], P.bits(c["weights"])) and np.array_equal(second[2], c["chosen"])
    assert np.array_equal(np.concatenate([first[3], second[3]]), P.bits(c["scores"]))
    w = P.weights("normal", n)
    none = _mw_cover(rows, D, W, n, 0, w, c["chosen"])
    assert len(none[0]) == 0 and np.array_equal(none[1], P.bits(w)) and np.array_equal(none[2], c["chosen"])
    for cap in (0, 4):
        empty = _mw_cover(rows[:0], cap, W, n, 3, w, np.zeros(0, np.uint8), length=0)
        assert empty[0].tolist() == [P.NO_ROW] * 3 and np.array_equal(empty[1], P.bits(w)) and not empty[2].any()
        assert empty[3].tolist() == [NEG_INF_BITS] * 3


# --- product paths ----------------------------------------------------------------------------------------

def _host_distribution(name, k, seed, S):
    St = pkg("stats")
    _, ids = P.instance(name, k)
    panels = P.oracle_table(name, k, seed, S)[0]
    first, mult = St.panel_multiplicities_host(panels)
    return St.PanelDistribution(S, first, mult, panels, len(ids), ids)


@pytest.mark.parametrize("table", ["example_small_20", "sf_e_110"])
def test_distribution_price_and_initial_committees(gpu_available, monkeypatch, table):
    """legacy_panel_distribution(...).price(w) and .initial_committees() on the device table against the mirror
    over the C oracle's panels: panel ids, value bits, row, first draw and multiplicity; committees, covered set
    and lines; legacy_initial_committees is the same triple.  sf_e's 300 draws leave agents that no panel holds
    and agents that only the first-holder pass covers (asserted)."""
    A, St = pkg("analysis"), pkg("stats")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    name, k, S, seed, rounds = P.COVER_TABLES[table]
    inst, ids = P.instance(name, k)
    n = len(ids)
    dist = A.legacy_panel_distribution(inst, S, seed)[3]
    host = _host_distribution(name, k, seed, S)
    assert dist.table().rows.is_cuda
    for kind in ("normal", "equal", "order"):
        w = P.weights(kind, n)
        want = host.price(w)
        got, scores = dist.price(dict(zip(ids, w.tolist())), scores=True)
        assert got.panel == want.panel and P.bits1(got.value) == P.bits1(want.value), kind
        assert got[2:] == want[2:], kind
        assert scores.is_cuda and np.array_equal(scores.cpu().numpy().view(np.uint64), P.bits(host.price(w, True)[1]))
        assert dist.price(w.tolist()) == got
    c = P.cover(table)
    default = rounds == 3 * n
    want = P.committees_loop(P.members(c["rows"], n), n, ids, c["picks"].tolist())
    if table == "sf_e_110":
        assert len(want[0]) > len(set(c["picks"].tolist())) and sum("not contained" in x for x in want[2]) == 10
    else:
        assert want[2] == ["All agents are contained in some drawn panel."]
    got = dist.initial_committees(None if default else rounds)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert isinstance(got[0], set) and isinstance(got[1], frozenset)
    again = A.legacy_initial_committees(inst, S, seed, None if default else rounds)
    assert again[0] == want[0] and again[1] == want[1] and again[2] == want[2]
    assert dist.initial_committees(0)[0] == host.initial_committees(0)[0]


@pytest.mark.parametrize("kind", ["normal", "equal"])
def test_legacy_price(gpu_available, kind):
    """Fresh draws priced chunk by chunk: chunk 1000 and chunk 3001 give the same (panel, value, index), the
    mirror's over the C oracle's 3001 panels with ties to the lowest draw index (all-equal weights: index 0)."""
    A, St = pkg("analysis"), pkg("stats")
    inst, ids = P.instance("example_small_20", 20)
    n, seed = len(ids), 4
    panels = P.oracle_table("example_small_20", 20, seed, 3001)[0]
    w = P.weights(kind, n)
    at, value, _ = St.rows_price_host(panels, w)
    assert kind != "equal" or at == 0
    want = (frozenset(ids[i] for i in P.members(panels[at:at + 1], n)[0]), value, at)
    for chunk in (1000, 3001):
        got = A.legacy_price(inst, w.tolist(), 3001, seed, chunk=chunk)
        assert got[0] == want[0] and P.bits1(got[1]) == P.bits1(want[1]) and got[2] == want[2], chunk
    assert A.legacy_price(inst, dict(zip(ids, w.tolist())), 3001, seed) == got
    assert A.legacy_price(inst, w, 0, seed) == (frozenset(), -np.inf, None)


def test_refusals(gpu_available, monkeypatch):
    A, D = pkg("analysis"), pkg("distributed")
    inst, ids = P.instance("example_small_20", 20)
    w = P.weights("normal", len(ids))
    dist = A.legacy_panel_distribution(inst, 50, 0)[3]
    for bad in (np.nan, np.inf):
        broken = w.copy()
        broken[3] = bad
        with pytest.raises(ValueError):
            dist.price(broken)
        with pytest.raises(ValueError):
            A.legacy_price(inst, broken, 50, 0)
    with pytest.raises(ValueError):
        A.legacy_price(inst, w[1:], 50, 0)
    missing = dict(zip(ids[1:], w.tolist()))
    with pytest.raises(KeyError):
        dist.price(missing)
    with pytest.raises(KeyError):
        A.legacy_price(inst, missing, 50, 0)
    monkeypatch.setattr(D, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size 2"):
        A.legacy_price(inst, w, 50, 0)
    with pytest.raises(NotImplementedError, match="world size 2"):
        A.legacy_initial_committees(inst, 50, 0)
