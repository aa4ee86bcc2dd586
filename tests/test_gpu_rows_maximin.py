"""The maximin lottery on the device: csa_rows_maximin_async (rm_start_kernel, rm_pick_kernel, rm_update_kernel,
rm_rescan_kernel, rm_bound_kernel around the unchanged rp_score_kernel) through the C ABI, and the product paths
on it -- PanelDistribution.maximin over a run's device table, legacy_maximin.

Expected values come from the numpy mirror stats.rows_maximin_host (itself checked against a plain Python loop in
test_rows_maximin_host.py), the C oracle's panels and, for the bounds, the LP through scipy's HiGHS.  State, picks
and the scores of all valid rows are compared bit for bit; every buffer the calls read or write carries guard
words behind it."""
from fractions import Fraction

import numpy as np
import pytest

import maximin_cases as M
import price_cases as P
from conftest import pkg
from test_gpu_rows_sort import GUARD, GUARD32, GUARD64, _dev64, _guards_ok

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = 0x7FF0000000000000


def _maximin(rows, n, rounds, shrink=0.8, resync=16, state=None, cap=None, length=None, fill=None, picks=True):
    """One csa_rows_maximin_async call over the first ``length`` rows in a table of ``cap`` rows whose other rows
    are all ones (scoring one would win).  ``state`` = a MaximinState (or the loop's dict) to continue, None to
    start on buffers whose used part holds ``fill`` (default: the guard patterns, i.e. dirty).  Returns (picks,
    MaximinState) after checking every guard, that nothing past the length was scored, and the inputs."""
    import torch
    N, St = pkg("_native"), pkg("stats")
    L = N.lib()
    W = rows.shape[1]
    length = len(rows) if length is None else length
    cap = length + 3 if cap is None else cap
    full = np.full((cap, W), ONES, np.uint64)
    full[:length] = rows[:length]
    d_rows = _dev64(full, GUARD) if cap else None
    d_len = _dev64(np.array([length], np.uint64), GUARD)
    i64 = lambda size, value: torch.full((size + GUARD,), value, dtype=torch.int64, device="cuda")
    i32 = lambda size, value: torch.full((size + GUARD,), value, dtype=torch.int32, device="cuda")
    d_w, d_sc, d_cover, d_count, d_state = i64(n, GUARD64), i64(cap, GUARD64), i32(n, GUARD32), i32(cap, GUARD32), \
        i64(4, GUARD64)
    if fill is not None:
        d_w[:n], d_sc[:length], d_cover[:n], d_count[:length], d_state[:4] = fill, fill, fill, fill, fill
    if state is not None:
        get = (lambda name: state[name]) if isinstance(state, dict) else (lambda name: getattr(state, name))
        d_w[:n] = torch.from_numpy(P.bits(get("weights")).view(np.int64))
        d_sc[:length] = torch.from_numpy(P.bits(get("scores")).view(np.int64))
        d_cover[:n] = torch.from_numpy(np.asarray(get("cover"), np.int64).astype(np.int32))
        d_count[:length] = torch.from_numpy(np.asarray(get("row_count"), np.int64).astype(np.int32))
        block = np.array([P.bits1(get("upper")), get("rounds"), get("best_row"), P.bits1(get("ratio"))], np.uint64)
        d_state[:4] = torch.from_numpy(block.view(np.int64))
        before = (d_w.clone(), d_sc.clone(), d_cover.clone(), d_count.clone(), d_state.clone())
    d_picks = i32(rounds, GUARD32) if picks else None
    need = int(L.csa_rows_maximin_scratch_bytes(cap, W))
    assert need % 8 == 0
    scratch = i64(need // 8, GUARD64)
    N.check(L.csa_rows_maximin_async(N.ptr(d_rows), N.ptr(d_len), cap, W, n, rounds, shrink, resync,
                                     N.CSA_MAXIMIN_START if state is None else 0, N.ptr(d_w), N.ptr(d_sc),
                                     N.ptr(d_cover), N.ptr(d_count), N.ptr(d_state), N.ptr(d_picks), N.ptr(scratch),
                                     need, None))
    torch.cuda.synchronize()
    assert _guards_ok(d_w, n, GUARD64) and _guards_ok(d_cover, n, GUARD32) and _guards_ok(d_state, 4, GUARD64)
    assert _guards_ok(d_count, cap, GUARD32) and _guards_ok(scratch, need // 8, GUARD64)
    assert _guards_ok(d_len, 1, GUARD64) and int(d_len[0].item()) == length
    assert d_picks is None or _guards_ok(d_picks, rounds, GUARD32)
    assert _guards_ok(d_sc, length, GUARD64)                # no score past the length, guards included
    if cap:
        assert _guards_ok(d_rows, cap * W, GUARD64)
        assert np.array_equal(d_rows[:cap * W].cpu().numpy().view(np.uint64).reshape(cap, W), full)
    if state is not None and (rounds == 0 or length == 0):   # nothing but the picks may have changed
        after = (d_w, d_sc, d_cover, d_count, d_state)
        assert all(bool((a == b).all().item()) for a, b in zip(after, before))
    block = d_state[:4].cpu().numpy().view(np.uint64)
    got = St.MaximinState(d_w[:n].cpu().numpy().view(np.float64), d_sc[:length].cpu().numpy().view(np.float64),
                          d_cover[:n].cpu().numpy().view(np.uint32).astype(np.int64),
                          d_count[:length].cpu().numpy().view(np.uint32).astype(np.int64),
                          float(block[0:1].view(np.float64)[0]), int(block[1]), int(block[2]),
                          float(block[3:4].view(np.float64)[0]))
    out = None if d_picks is None else d_picks[:rounds].cpu().numpy().view(np.uint32).astype(np.int64)
    return out, got


def _same(got, want):
    """(picks, MaximinState) from the device against the mirror's, bit for bit."""
    assert got[0].tolist() == want[0].tolist()
    assert M.same_state(got[1], M.state_dict(want[1])) is None, M.same_state(got[1], M.state_dict(want[1]))


def _shape(name):
    if name == "sf_e_110":
        inst, k, S, seed, _ = P.COVER_TABLES[name]
        _, ids = P.instance(inst, k)
        return P.oracle_table(inst, k, seed, S)[1], len(ids)
    D, n, k = {"W1": (300, 20, 5), "W2": (1000, 70, 9), "W3": (3000, 150, 20)}[name]
    return M.skewed_rows(D, n, k), n


@pytest.mark.parametrize("shrink", [0.8, 0.95])
@pytest.mark.parametrize("resync", [1, 7, 16])
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "sf_e_110"])
def test_rounds_equal_the_mirror(gpu_available, name, resync, shrink):
    """W = 1 (n = 20, 261 rows), W = 2 (n = 70, no multiple of 64), W = 3 (n = 150, 3000 rows) and the sf_e_110
    oracle table (W = 27: two staging passes, agents no row holds): 40 rounds -- no multiple of 7 or 16 -- of
    updates and fresh passes equal the mirror's weights, scores, cover, row counts, state block and picks."""
    St = pkg("stats")
    rows, n = _shape(name)
    assert rows.shape[1] == {"W1": 1, "W2": 2, "W3": 3, "sf_e_110": 27}[name]
    if name == "sf_e_110":
        assert len(rows) == 300 and len(M.covered(rows, n)) == n - 10
    _same(_maximin(rows, n, 40, shrink, resync), St.rows_maximin_host(rows, n, 40, shrink, resync))


@pytest.mark.parametrize("D", [1, 255, 256, 257, 1000])
def test_row_counts_around_the_tile(gpu_available, D):
    """One row, the tile boundary, several workgroups; the capacity exceeds the length and the rows past it are
    all ones.  A NULL d_picks gives the same state."""
    St = pkg("stats")
    assert int(pkg("_native").lib().csa_rows_price_tile()) == 256
    rows, n = M.skewed_rows(1000, 70, 9)[:D], 70
    want = St.rows_maximin_host(rows, n, 20, 0.8, 7)
    _same(_maximin(rows, n, 20, 0.8, 7, cap=D + 300), want)
    assert M.same_state(_maximin(rows, n, 20, 0.8, 7, picks=False)[1], M.state_dict(want[1])) is None
    if D == 1000:
        assert len({p // 256 for p in want[0].tolist()}) > 1          # the picks come from more than one tile


def test_ties_go_to_the_lowest_row(gpu_available):
    """Six disjoint panels under equal weights: every fresh pass is all ties; the picks cycle 0..5, both bounds
    are 1/6.  And 600 equal-weight subsets over three workgroups start at row 0."""
    St = pkg("stats")
    rows = M.partition_rows(24, 4)
    got = _maximin(rows, 24, 60, 0.8, 7)
    assert got[0].tolist() == list(range(6)) * 10 and got[1].cover.tolist() == [10] * 24
    assert M.lower_bound(got[1], 60) == Fraction(1, 6) and abs(got[1].upper - 1 / 6) <= 1e-15
    _same(got, St.rows_maximin_host(rows, 24, 60, 0.8, 7))
    rows = P.subset_rows(600, 2, 91, k=9)
    got = _maximin(rows, 91, 12, 0.8, 16)
    assert got[0][0] == 0
    _same(got, St.rows_maximin_host(rows, 91, 12, 0.8, 16))


def test_update_order_decides_a_pick(gpu_available):
    """The forged state of test_rows_maximin_host: ascending intersection sums cancel the scores to +0.0 and the
    second pick is row 0; another order would leave a residue and pick elsewhere (asserted from the loop)."""
    rows, n, p0 = M.skewed_rows(1000, 70, 9), 70, 17
    mem = P.members(rows, n)
    forged = M.forged_order_state(rows, n, p0)
    up_picks, up = M.maximin_loop(mem, n, 2, 2, 0.8, 16, state=forged)
    assert up_picks == [p0, 0] and M.maximin_loop(mem, n, 2, 2, 0.8, 16, state=forged, descending=True)[0][1] != 0
    picks, state = _maximin(rows, n, 2, 0.8, 16, state=forged)
    assert picks.tolist() == up_picks and M.same_state(state, up) is None


@pytest.mark.parametrize("a,resync", [(23, 16), (32, 16)])
def test_continuation(gpu_available, a, resync):
    """Two device calls, the second on the first's state with a scratch of its own, equal the mirror's two calls;
    with a a multiple of resync they also equal one call of a + b."""
    St = pkg("stats")
    rows, n, b = M.skewed_rows(1000, 70, 9), 70, 30
    w1 = St.rows_maximin_host(rows, n, a, 0.8, resync)
    w2 = St.rows_maximin_host(rows, n, b, 0.8, resync, state=w1[1])
    g1 = _maximin(rows, n, a, 0.8, resync)
    _same(g1, w1)
    g2 = _maximin(rows, n, b, 0.8, resync, state=g1[1])
    _same(g2, w2)
    assert g2[1].rounds == a + b
    if a % resync == 0:
        whole = St.rows_maximin_host(rows, n, a + b, 0.8, resync)
        assert g1[0].tolist() + g2[0].tolist() == whole[0].tolist()
        assert M.same_state(g2[1], M.state_dict(whole[1])) is None


def test_start_on_used_buffers_and_no_rounds(gpu_available):
    """START on buffers full of other values equals START on zeroed ones; rounds == 0 with START only
    initialises; without START it changes nothing."""
    St = pkg("stats")
    rows, n = M.skewed_rows(300, 20, 5), 20
    want = St.rows_maximin_host(rows, n, 25, 0.8, 7)
    _same(_maximin(rows, n, 25, 0.8, 7), want)
    _same(_maximin(rows, n, 25, 0.8, 7, fill=0), want)
    start = St.rows_maximin_host(rows, n, 0)
    _same(_maximin(rows, n, 0), start)
    assert start[1].rounds == 0 and start[1].upper == 5.0 / 19
    _same(_maximin(rows, n, 0, state=want[1]), (np.zeros(0, np.int64), want[1]))


def test_empty_table(gpu_available):
    """No valid row (capacity 0, and capacity 4 with length 0): the picks are 0xFFFFFFFF and a given state is
    untouched (checked inside the call helper); START gives (+inf, 0, none, +inf) and weights of +0.0."""
    rows, n = M.skewed_rows(300, 20, 5), 20
    state = pkg("stats").rows_maximin_host(rows[:0], n, 0)[1]
    state = state._replace(weights=P.weights("normal", n), cover=np.arange(n), upper=0.25, rounds=7, best_row=3, ratio=0.5)
    for cap in (0, 4):
        picks, got = _maximin(rows[:0], n, 3, 0.8, 1, state=state, cap=cap, length=0)
        assert picks.tolist() == [P.NO_ROW] * 3 and M.same_state(got, M.state_dict(state)) is None
        picks, got = _maximin(rows[:0], n, 3, cap=cap, length=0)
        assert picks.tolist() == [P.NO_ROW] * 3 and P.bits(got.weights).tolist() == [0] * n
        assert (P.bits1(got.upper), got.rounds, got.best_row, P.bits1(got.ratio)) == (INF_BITS, 0, P.PRICE_NONE, INF_BITS)
        assert not got.cover.any()


# --- product paths ----------------------------------------------------------------------------------------

def _host_distribution(name, k, seed, S):
    St = pkg("stats")
    _, ids = P.instance(name, k)
    panels = P.oracle_table(name, k, seed, S)[0]
    first, mult = St.panel_multiplicities_host(panels)
    return St.PanelDistribution(S, first, mult, panels, len(ids), ids)


def _fields(a, b):
    for name in ("rows", "counts", "rounds", "panels", "probabilities", "alloc", "covered_agents", "lower",
                 "output_lines"):
        assert getattr(a, name) == getattr(b, name), name
    assert P.bits1(a.upper) == P.bits1(b.upper)
    assert a == b and a.portfolio() == b.portfolio()


def test_distribution_maximin_on_a_device_table(gpu_available, monkeypatch):
    """example_small_20, S = 3000, 600 rounds: the run's device table gives what the same panels' host table
    gives, field for field; the portfolio's selection probabilities through portfolio_probabilities agree with
    alloc to 1e-12 absolute (at most a few hundred float64 adds of values <= 1)."""
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    name, k, S, seed, rounds = P.COVER_TABLES["example_small_20"]
    inst, ids = P.instance(name, k)
    dist = A.legacy_panel_distribution(inst, S, seed)[3]
    assert dist.table().rows.is_cuda and rounds == 600
    got = dist.maximin(rounds)
    _fields(got, _host_distribution(name, k, seed, S).maximin(rounds))
    assert got.rounds == 600 and got.lower > 0 and Fraction(got.lower) <= got.upper
    assert got.output_lines == ["All agents are contained in some drawn panel."]
    probs = A.portfolio_probabilities(inst, *got.portfolio())[0]
    assert set(probs) == set(got.alloc)
    assert max(abs(probs[a] - float(got.alloc[a])) for a in ids) <= 1e-12


def test_legacy_maximin(gpu_available, monkeypatch):
    """couples, S = 500, end to end with the default 3 n rounds and with other parameters."""
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    name, k, S, seed, _ = P.COVER_TABLES["couples"]
    inst, ids = P.instance(name, k)
    host = _host_distribution(name, k, seed, S)
    got = A.legacy_maximin(inst, S, seed)
    _fields(got, host.maximin())
    assert got.rounds == 3 * len(ids)
    _fields(A.legacy_maximin(inst, S, seed, 50, shrink=0.9, resync=4), host.maximin(50, 0.9, 4))
    _fields(A.legacy_maximin(inst, S, seed, 0), host.maximin(0))


def test_bounds_against_the_lp_through_the_device(gpu_available):
    """The 261-row skewed table as a device table under PanelDistribution.maximin: lower <= z* <= upper with
    HiGHS's 1e-9, z* below the trivial k / covered and lower positive (the conditions on the input)."""
    import torch
    St = pkg("stats")
    D, n, k, shrink, rounds = M.SKEWED[0]
    rows = M.skewed_rows(D, n, k)
    z = M.lp_optimum(D, n, k)
    assert len(rows) == 261 and z < k / len(M.covered(rows, n)) - 1e-6
    ids = list(range(n))
    dist = St.PanelDistribution(len(rows), np.arange(len(rows)), np.ones(len(rows), np.int64), rows, n, ids)
    host = dist.maximin(rounds, shrink)
    dist._table = St.RowTable(torch.from_numpy(rows.view(np.int64).copy()).cuda(), None, None,
                              torch.tensor([len(rows)], dtype=torch.int64, device="cuda"), len(rows), 1)
    got = dist.maximin(rounds, shrink)
    _fields(got, host)
    print("z*", z, "lower", float(got.lower), "upper", got.upper)
    assert got.lower > 0 and float(got.lower) <= z + 1e-9 and z <= got.upper + 1e-9
