"""The Nash-welfare lottery on the device: csa_rows_marginals_async (rn_marginal_kernel, rn_finish_kernel) and
csa_rows_nash_async (rn_start_kernel, rn_held_kernel, rn_step_kernel, rn_bound_kernel around them and the
unchanged rp_first_holder_kernel and rp_score_kernel) through the C ABI, and the product paths on them --
PanelDistribution.nash over a run's device table, legacy_nash.

Expected values come from the numpy mirrors stats.rows_marginals_host / stats.rows_nash_host (themselves checked
against a plain Python loop in test_rows_nash_host.py) and the C oracle's panels.  Everything is compared bit for
bit; every buffer the calls read or write carries guard words behind it, the rows past the length are all ones
and the outputs start dirty."""
import math

import numpy as np
import pytest

import maximin_cases as M
import nash_cases as C
import price_cases as P
from conftest import pkg
from test_gpu_rows_sort import GUARD, GUARD32, GUARD64, _dev32, _dev64, _guards_ok

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = 0x7FF0000000000000


def _table(rows, cap, length):
    W = rows.shape[1]
    full = np.full((cap, W), ONES, np.uint64)
    full[:length] = rows[:length]
    return full, (_dev64(full, GUARD) if cap else None), _dev64(np.array([length], np.uint64), GUARD)


def _table_untouched(full, d_rows, d_len, length):
    cap, W = full.shape
    assert _guards_ok(d_len, 1, GUARD64) and int(d_len[0].item()) == length
    if cap:
        assert _guards_ok(d_rows, cap * W, GUARD64)
        assert np.array_equal(d_rows[:cap * W].cpu().numpy().view(np.uint64).reshape(cap, W), full)


def _marginals(rows, prob, n, cap=None):
    """One csa_rows_marginals_async call over ``rows`` in a table of ``cap`` rows whose other rows are all ones and
    whose other probabilities are huge: (pi, psum) after checking every guard and the inputs."""
    import torch
    N = pkg("_native")
    L = N.lib()
    length, W = rows.shape
    cap = length + 3 if cap is None else cap
    full, d_rows, d_len = _table(rows, cap, length)
    p = np.full(cap, 1e300, np.float64)
    p[:length] = prob
    d_prob = _dev64(P.bits(p), GUARD)
    i64 = lambda size: torch.full((size + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    d_pi, d_psum = i64(n), i64(1)
    need = int(L.csa_rows_marginals_scratch_bytes(cap, W))
    assert need == ((cap + 1023) // 1024) * (64 * W + 1) * 8
    scratch = i64(need // 8)
    N.check(L.csa_rows_marginals_async(N.ptr(d_rows), N.ptr(d_len), cap, W, n, N.ptr(d_prob), N.ptr(d_pi), N.ptr(d_psum),
                                       N.ptr(scratch), need, None))
    torch.cuda.synchronize()
    assert _guards_ok(d_pi, n, GUARD64) and _guards_ok(d_psum, 1, GUARD64) and _guards_ok(scratch, need // 8, GUARD64)
    assert _guards_ok(d_prob, cap, GUARD64) and np.array_equal(d_prob[:cap].cpu().numpy().view(np.float64), p)
    _table_untouched(full, d_rows, d_len, length)
    return d_pi[:n].cpu().numpy().view(np.float64), float(d_psum[:1].cpu().numpy().view(np.float64)[0])


def _same_marginals(rows, prob, n, cap=None):
    St = pkg("stats")
    pi, psum = _marginals(rows, prob, n, cap)
    want = St.rows_marginals_host(rows, prob, n)
    assert np.array_equal(P.bits(pi), P.bits(want[0])) and P.bits1(psum) == P.bits1(want[1])


def _nash(rows, n, rounds, mult=None, total=0, state=None, cap=None, length=None, start=None):
    """One csa_rows_nash_async call over the first ``length`` rows in a table of ``cap`` rows whose other rows are
    all ones (their multiplicities huge).  ``state`` = a NashState to continue, None to start on buffers that hold
    the guard patterns, i.e. dirty.  Returns the NashState after checking every guard, that nothing past the
    length was written, and the inputs.  The scratch is fresh in every call."""
    import torch
    N, St = pkg("_native"), pkg("stats")
    L = N.lib()
    W = rows.shape[1]
    length = len(rows) if length is None else length
    cap = length + 3 if cap is None else cap
    start = state is None if start is None else start
    full, d_rows, d_len = _table(rows, cap, length)
    i64 = lambda size: torch.full((size + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    d_p, d_sc, d_pi, d_state = i64(cap), i64(cap), i64(n), i64(4)
    d_mult = None
    if mult is not None:
        mu = np.full(cap, 0xFFFFFFF0, np.int64)
        mu[:length] = mult[:length]
        d_mult = _dev32(mu, GUARD)
    if state is not None:
        d_p[:length] = torch.from_numpy(P.bits(state.prob).view(np.int64))
        d_sc[:length] = torch.from_numpy(P.bits(state.scores).view(np.int64))
        d_pi[:n] = torch.from_numpy(P.bits(state.marginals).view(np.int64))
        block = np.array([P.bits1(state.ratio), state.rounds, state.best_row, P.bits1(state.psum)], np.uint64)
        d_state[:4] = torch.from_numpy(block.view(np.int64))
    before = (d_p.clone(), d_sc.clone(), d_pi.clone(), d_state.clone())
    need = int(L.csa_rows_nash_scratch_bytes(cap, W))
    assert need % 8 == 0
    scratch = i64(need // 8)
    N.check(L.csa_rows_nash_async(N.ptr(d_rows), N.ptr(d_len), cap, W, n, rounds, N.CSA_NASH_START if start else 0,
                                  N.ptr(d_mult), total, N.ptr(d_p), N.ptr(d_sc), N.ptr(d_pi), N.ptr(d_state),
                                  N.ptr(scratch), need, None))
    torch.cuda.synchronize()
    assert _guards_ok(d_pi, n, GUARD64) and _guards_ok(d_state, 4, GUARD64) and _guards_ok(scratch, need // 8, GUARD64)
    assert _guards_ok(d_p, length, GUARD64) and _guards_ok(d_sc, length, GUARD64)   # nothing past the length
    assert d_mult is None or (_guards_ok(d_mult, cap, GUARD32) and d_mult[:length].cpu().tolist() == list(mult[:length]))
    _table_untouched(full, d_rows, d_len, length)
    if not start and (rounds == 0 or length == 0):           # nothing may have changed
        assert all(bool((a == b).all().item()) for a, b in zip((d_p, d_sc, d_pi, d_state), before))
    block = d_state[:4].cpu().numpy().view(np.uint64)
    f = lambda t, size: t[:size].cpu().numpy().view(np.float64)
    return St.NashState(f(d_p, length), f(d_sc, length), f(d_pi, n), float(block[0:1].view(np.float64)[0]), int(block[1]),
                        int(block[2]), float(block[3:4].view(np.float64)[0]))


def _same(got, want):
    assert C.same_state(got, want) is None, C.same_state(got, want)


def _shape(name):
    if name == "sf_e_110":
        inst, k, S, seed, _ = P.COVER_TABLES[name]
        _, ids = P.instance(inst, k)
        _, rows, _, mult = P.oracle_table(inst, k, seed, S)
        return rows, len(ids), mult, S
    rows, n = C.table(name)
    return (rows, n) + C.mults(len(rows))


# --- the marginal pass alone ------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("D", [1, 1023, 1024, 1025, 2049, 3000])
def test_marginals_around_the_tile(gpu_available, D, W):
    """One row, the tile boundary, a tile and a row, two tiles and a row, 3000 rows; one, two and three row words
    (the last wave of a workgroup idle) with an n that is no multiple of 64; the capacity exceeds the length and
    the rows past it are all ones with p = 1e300; the weights are spread over 2^-20 .. 2^20."""
    assert int(pkg("_native").lib().csa_rows_nash_tile()) == 1024
    n = {1: 20, 2: 70, 3: 150}[W]
    rows = P.subset_rows(D, W, n, salt=3)
    assert rows.shape == (D, W) and n % 64
    _same_marginals(rows, C.spread_prob(D, salt=W), n, cap=D + 700)


def test_marginals_follow_the_contract_order(gpu_available):
    """The order condition of test_rows_nash_host on the device: over the 3000-row table under spread weights the
    ascending loop and the descending loop differ in bits, and the device gives the ascending ones."""
    rows, n = C.table("W3")
    mem = P.members(rows, n)
    prob = C.spread_prob(len(rows))
    up, up_sum = C.marginals_loop(mem, prob, n)
    assert (P.bits(up) != P.bits(C.marginals_loop(mem, prob, n, descending=True)[0])).any()
    pi, psum = _marginals(rows, prob, n)
    assert np.array_equal(P.bits(pi), P.bits(up)) and P.bits1(psum) == P.bits1(up_sum)


def test_marginals_of_the_oracle_table_and_an_empty_one(gpu_available):
    """The 300-row sf_e_110 oracle table: W = 27 (four workgroups of words per tile, the last with three waves),
    ten agents no row holds, whose marginal is +0.0; p = multiplicities / S.  And an empty table (capacity 0, and
    capacity 5 with length 0) writes +0.0 everywhere."""
    rows, n, mult, S = _shape("sf_e_110")
    assert rows.shape == (300, 27) and len(M.covered(rows, n)) == n - 10
    prob = mult / np.float64(S)
    _same_marginals(rows, prob, n)
    pi, _ = _marginals(rows, prob, n, cap=300)
    assert (pi == 0.0).sum() == 10
    for cap in (0, 5):
        pi, psum = _marginals(rows[:0], prob[:0], n, cap=cap)
        assert P.bits(pi).tolist() == [0] * n and P.bits1(psum) == 0


# --- the rounds ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", ["legacy", "uniform"])
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "sf_e_110"])
def test_rounds_equal_the_mirror(gpu_available, name, start):
    """W = 1 (n = 20, 261 rows), W = 2 (n = 70), W = 3 (n = 150, three tiles) and the sf_e_110 oracle table
    (W = 27, agents no row holds): 40 rounds from the multiplicities and from the uniform start equal the
    mirror's prob, scores, marginals and state block."""
    St = pkg("stats")
    rows, n, mult, total = _shape(name)
    assert rows.shape[1] == {"W1": 1, "W2": 2, "W3": 3, "sf_e_110": 27}[name]
    if start == "uniform":
        mult, total = None, 0
    want = C.mirror(name, start, 40) if name in C.SHAPES else St.rows_nash_host(rows, n, 40, mult, total or None)
    got = _nash(rows, n, 40, mult, total)
    _same(got, want)
    assert got.rounds == 40 and abs(got.psum - 1.0) <= 1e-13


def test_start_alone_and_a_continued_call(gpu_available):
    """START with no rounds only starts; 25 rounds continued by 15 on a fresh scratch equal one call of 40 and the
    mirror; no START and no rounds changes nothing (checked inside the helper); START on a state restarts."""
    rows, n, mult, total = _shape("W2")
    start = _nash(rows, n, 0, mult, total)
    _same(start, C.mirror("W2", "legacy", 0))
    assert start.rounds == 0 and np.array_equal(start.prob, mult / np.float64(total))
    first = _nash(rows, n, 25, mult, total)
    second = _nash(rows, n, 15, state=first)
    _same(second, C.mirror("W2", "legacy", 40))
    _same(second, _nash(rows, n, 40, mult, total, cap=len(rows)))
    _same(_nash(rows, n, 0, state=second), second)
    _same(_nash(rows, n, 40, None, 0, state=second, start=True), C.mirror("W2", "uniform", 40))


def test_row_counts_around_the_tiles(gpu_available):
    """One row, the score pass's tile (256) and the marginal pass's (1024) and one past it, with a larger capacity."""
    St = pkg("stats")
    rows, n = C.table("W3")
    for D in (1, 257, 1024, 1025):
        mult, total = C.mults(D, salt=D)
        _same(_nash(rows[:D], n, 5, mult, total, cap=D + 1100), St.rows_nash_host(rows[:D], n, 5, mult, total))


def test_empty_table(gpu_available):
    """No valid row (capacity 0, and capacity 4 with length 0): START writes pi = +0.0 and (+inf, 0, none, +0.0);
    rounds on a given state change nothing (checked inside the helper)."""
    St = pkg("stats")
    rows, n = C.table("W1")
    state = St.NashState(np.zeros(0), np.zeros(0), P.weights("normal", n), 1.25, 7, 3, 0.5)
    for cap in (0, 4):
        got = _nash(rows[:0], n, 3, cap=cap, length=0)
        assert (P.bits1(got.ratio), got.rounds, got.best_row, P.bits1(got.psum)) == (INF_BITS, 0, P.PRICE_NONE, 0)
        assert P.bits(got.marginals).tolist() == [0] * n
        _same(got, St.rows_nash_host(rows[:0], n, 3))
        _same(_nash(rows[:0], n, 3, state=state, cap=cap, length=0), state)


def test_refusals_leave_the_buffers_alone(gpu_available):
    """The refusals of test_rows_nash_host with device buffers: the code comes back and nothing was written."""
    import torch
    N = pkg("_native")
    L = N.lib()
    rows, n, mult, total = _shape("W2")
    cap, W = len(rows), 2
    d_rows, d_len, d_mult = _dev64(rows), _dev64(np.array([cap], np.uint64)), _dev32(mult)
    need = int(L.csa_rows_nash_scratch_bytes(cap, W))
    bufs = [torch.full((size,), GUARD64, dtype=torch.int64, device="cuda") for size in (cap, cap, n, 4, need // 8)]
    p, sc, pi, state, scratch = bufs
    at = lambda t, off=0: None if t is None else N.ptr(t).value + off

    def call(rows=d_rows, length=d_len, cap=cap, W=W, n=n, rounds=3, flags=1, mult=d_mult, total=total, p=p, sc=sc,
             pi=pi, state=state, scratch=scratch, off=0, bytes_=need):
        return L.csa_rows_nash_async(at(rows), at(length), cap, W, n, rounds, flags, at(mult), total, at(p), at(sc),
                                     at(pi), at(state), at(scratch, off), bytes_, None)

    for bad in (dict(n=129), dict(n=0), dict(W=0), dict(length=None), dict(rows=None), dict(flags=2), dict(p=None),
                dict(sc=None), dict(pi=None), dict(state=None), dict(total=0), dict(scratch=None), dict(bytes_=need - 1),
                dict(off=4), dict(sc=p), dict(p=d_rows), dict(pi=scratch), dict(state=d_len), dict(p=d_mult)):
        assert call(**bad) == N.CSA_E_INVALID, bad
    assert call(cap=2 ** 32 - 1, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    assert call(W=4096, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    part = int(L.csa_rows_marginals_scratch_bytes(cap, W))
    for bad in (dict(n=129), dict(prob=None), dict(pi=None), dict(psum=None), dict(scratch=None), dict(bytes_=part - 1),
                dict(pi=p), dict(psum=d_len), dict(pi=scratch)):
        args = dict(n=n, prob=p, pi=pi, psum=state, scratch=scratch, bytes_=part)
        args.update(bad)
        assert L.csa_rows_marginals_async(at(d_rows), at(d_len), cap, W, args["n"], at(args["prob"]), at(args["pi"]),
                                          at(args["psum"]), at(args["scratch"]), args["bytes_"], None) == N.CSA_E_INVALID, bad
    torch.cuda.synchronize()
    assert all(bool((t == GUARD64).all().item()) for t in bufs)
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64).reshape(cap, W), rows)


# --- product paths ----------------------------------------------------------------------------------------

def _host_distribution(name, k, seed, S):
    St = pkg("stats")
    _, ids = P.instance(name, k)
    panels = P.oracle_table(name, k, seed, S)[0]
    first, mult = St.panel_multiplicities_host(panels)
    return St.PanelDistribution(S, first, mult, panels, len(ids), ids)


def _fields(a, b):
    assert np.array_equal(P.bits(a.probabilities), P.bits(b.probabilities))
    for name in ("alloc", "covered_agents", "output_lines", "geometric_mean", "start_geometric_mean", "gap", "upper",
                 "best_row", "best_panel", "rounds"):
        assert getattr(a, name) == getattr(b, name), name
    assert a == b and a.portfolio() == b.portfolio()


@pytest.mark.parametrize("table,S,rounds", [("sf_e_110", 3000, 40), ("example_small_20", 2000, 200)])
def test_legacy_nash_equals_the_host_table(gpu_available, monkeypatch, table, S, rounds):
    """legacy_nash end to end on the device equals PanelDistribution.nash over the same run's host-materialised
    table, field by field, from both starts; start_geometric_mean <= geometric_mean <= upper; the portfolio runs
    through portfolio_probabilities on the device and gives alloc back; alloc's geometric mean over the covered
    agents is geometric_mean (1e-12 relative)."""
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    name, k, _, seed, _ = P.COVER_TABLES[table]
    inst, ids = P.instance(name, k)
    run = A.legacy_panel_distribution(inst, S, seed)[3]
    assert run.table().rows.is_cuda
    host = _host_distribution(name, k, seed, S)
    got = A.legacy_nash(inst, S, seed, rounds)
    _fields(got, host.nash(rounds))
    _fields(run.nash(rounds, start="uniform"), host.nash(rounds, "uniform"))
    _fields(A.legacy_nash(inst, S, seed, 0), host.nash(0))
    assert got.rounds == rounds and len(got.probabilities) == run.distinct
    print(table, "start", got.start_geometric_mean, "gm", got.geometric_mean, "upper", got.upper, "gap", got.gap)
    assert 0 < got.start_geometric_mean <= got.geometric_mean <= got.upper
    again = math.exp(math.fsum(math.log(got.alloc[a]) for a in got.covered_agents) / len(got.covered_agents))
    assert abs(again - got.geometric_mean) <= 1e-12 * got.geometric_mean
    panels, probs = got.portfolio()
    assert abs(math.fsum(probs) - 1.0) <= 1e-12
    alloc = A.portfolio_probabilities(inst, panels, probs)[0]
    assert set(alloc) == set(got.alloc)
    dropped = 1.0 - math.fsum(float(x) for x in got.probabilities if x >= 1e-9)
    # the kept rows' mass is 1 - dropped, renormalised: each alloc moves by at most dropped / (1 - dropped), plus
    # the roundings of at most len(panels) adds of values <= 1 on either side (and of the sum that gives dropped)
    bound = abs(dropped) / (1.0 - abs(dropped)) + (len(panels) + len(got.probabilities)) * 2.0 ** -52
    assert max(abs(alloc[a] - got.alloc[a]) for a in ids) <= bound
