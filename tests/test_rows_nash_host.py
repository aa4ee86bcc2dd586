"""The Nash-welfare lottery over drawn panels on the host: stats.rows_marginals_host and stats.rows_nash_host
(the contracts of csa_rows_marginals_async and csa_rows_nash_async in numpy) against the plain Python loop of
nash_cases, closed forms, the iteration's properties and its certificate against exact rational arithmetic, the
product path PanelDistribution.nash over host tables, and the entry points' refusals, which need no device."""
import ctypes
import math
import pickle
import re

import numpy as np
import pytest

import maximin_cases as M
import nash_cases as C
import price_cases as P
from conftest import pkg

STARTS = ["legacy", "uniform"]


def _start(rows, start):
    return C.mults(len(rows)) if start == "legacy" else (None, None)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", ["W1", "W2", "W3"])
def test_mirror_is_the_loop(name, start):
    """prob, scores, marginals, ratio, best row, psum: bit for bit after 0, 1 and 40 rounds, from both starts; and
    25 rounds continued by 15 equal one call of 40."""
    St = pkg("stats")
    rows, n = C.table(name)
    assert rows.shape[1] == {"W1": 1, "W2": 2, "W3": 3}[name]
    mem = P.members(rows, n)
    mult, total = _start(rows, start)
    want = C.nash_loop(mem, n, 0, mult, total)
    for rounds in (0, 1, 40):
        if rounds:
            want = C.nash_loop(mem, n, rounds - want["rounds"], state=want)     # the loop continues itself
        got = C.mirror(name, start, rounds)
        assert C.same_state(got, want) is None, (rounds, C.same_state(got, want))
        assert got.rounds == rounds
    first = St.rows_nash_host(rows, n, 25, mult, total)
    keep = P.bits(first.prob).copy()
    second = St.rows_nash_host(rows, n, 15, state=first)
    assert np.array_equal(P.bits(first.prob), keep)                             # the input state is left alone
    assert C.same_state(second, C.mirror(name, start, 40)) is None and second.rounds == 40


def test_loop_continued_is_the_loop():
    """A self-check of the yardstick, not of the package: test_mirror_is_the_loop compares the mirror with the
    loop CONTINUED from its own state, so the loop's continuation must equal the loop in one call."""
    rows, n = C.table("W1")
    mem = P.members(rows, n)
    one = C.nash_loop(mem, n, 7)
    two = C.nash_loop(mem, n, 4, state=C.nash_loop(mem, n, 3))
    assert all(P.bits(one[k]).tolist() == P.bits(two[k]).tolist() for k in ("prob", "scores", "marginals"))
    assert (one["ratio"], one["rounds"], one["best_row"], one["psum"]) == (two["ratio"], 7, two["best_row"], two["psum"])


def test_marginal_order_shows_in_the_bits():
    """p spread over 2^-20 .. 2^20 on the 3000-row table (three tiles): the mirror equals the ascending loop bit
    for bit, and the descending loop gives other bits -- the condition that lets the order test fail."""
    St = pkg("stats")
    rows, n = C.table("W3")
    assert len(rows) > 2 * C.TILE
    mem = P.members(rows, n)
    prob = C.spread_prob(len(rows))
    up, up_sum = C.marginals_loop(mem, prob, n)
    down, down_sum = C.marginals_loop(mem, prob, n, descending=True)
    assert (P.bits(up) != P.bits(down)).any()
    pi, psum = St.rows_marginals_host(rows, prob, n)
    assert np.array_equal(P.bits(pi), P.bits(up)) and P.bits1(psum) == P.bits1(up_sum)
    exact_pi = C.exact(mem, n, prob)[0]
    assert max(abs(float(x) - y) / y for x, y in zip(exact_pi, up) if y) <= len(rows) * 2.0 ** -53


def test_marginals_of_short_and_ragged_tables():
    """One row, a tile and a row, an empty table, n below 64 W, agents nobody holds; bad shapes raise."""
    St = pkg("stats")
    rows, n = C.table("W2")
    for D in (1, 1024, 1025):
        sub = np.concatenate([rows, rows])[:D]
        prob = C.spread_prob(D, salt=D)
        want = C.marginals_loop(P.members(sub, n + 5), prob, n + 5)
        pi, psum = St.rows_marginals_host(sub, prob, n + 5)
        assert np.array_equal(P.bits(pi), P.bits(want[0])) and P.bits1(psum) == P.bits1(want[1])
        assert P.bits(pi[n:]).tolist() == [0] * 5
    pi, psum = St.rows_marginals_host(rows[:0], np.zeros(0), n)
    assert P.bits(pi).tolist() == [0] * n and P.bits1(psum) == 0
    for bad in ((rows, np.ones(3), n), (rows, np.ones(len(rows)), 129), (rows, np.ones(len(rows)), 0)):
        with pytest.raises(ValueError):
            St.rows_marginals_host(*bad)


@pytest.mark.parametrize("start", STARTS)
def test_disjoint_rows_closed_form(start):
    """Disjoint rows of sizes k_d: pi_i = p_d on row d, G_d = k_d / p_d, so one round gives p_d = k_d / m from any
    start with full support, and ratio = 1.  Each of p, G / m, the product and the ratio is a handful of float64
    roundings of at most 2^-53 relative: within 1e-14."""
    St = pkg("stats")
    sizes = [3, 1, 7, 2, 5, 4, 11, 1, 6]
    rows, n = C.disjoint_rows(sizes)
    mult, total = _start(rows, start)
    st = St.rows_nash_host(rows, n, 1, mult, total)
    assert st.rounds == 1
    for d, k in enumerate(sizes):
        assert abs(st.prob[d] - k / n) <= 1e-14 * (k / n)
    assert abs(st.ratio - 1.0) <= 1e-14 and abs(st.psum - 1.0) <= 1e-14
    assert max(abs(st.marginals[i] - 1.0 / n * k) for d, k in enumerate(sizes) for i in P.members(rows[d:d + 1], n)[0]) <= 1e-14
    start0 = St.rows_nash_host(rows, n, 0, mult, total)
    assert start0.rounds == 0 and start0.ratio > 1.5                     # the start is not the optimum
    if start == "uniform":                                               # pi = 1 / D, G_d = k_d D
        assert abs(start0.ratio - max(sizes) * len(sizes) / n) <= 1e-12
    # equal sizes: the uniform lottery, at once and after a round
    rows, n = M.partition_rows(24, 4), 24
    for rounds in (0, 1):
        st = St.rows_nash_host(rows, n, rounds, *(_start(rows, start) if rounds else (None, None)))
        assert max(abs(st.prob - 1 / 6)) <= 1e-14 / 6 and abs(st.ratio - 1.0) <= 1e-14


@pytest.mark.parametrize("name", ["W1", "W2"])
def test_properties_over_400_rounds(name):
    """Cover's iteration in float64 over 400 rounds from both starts: the geometric mean never falls by more than
    1e-15 relative between rounds, psum stays within 1e-13 of 1, every lower bound met at rounds 10, 50, 400
    under either start lies below every upper bound met there (they bound one optimum), and the reported ratio
    equals its exact-rational recomputation from the same p within 1e-12 relative."""
    rows, n = C.table(name)
    mem = P.members(rows, n)
    lowers, uppers = [], []
    for start in STARTS:
        states = C.trajectory(name, start, 400)
        gm = [C.geometric_mean(s.marginals, s.psum) for s in states]
        print(name, start, "gm", gm[0], gm[400], "ratio", [states[r].ratio for r in (0, 10, 50, 100, 200, 400)])
        assert [s.rounds for s in states] == list(range(401))
        assert all(b >= a * (1 - 1e-15) for a, b in zip(gm, gm[1:]))
        assert max(abs(s.psum - 1.0) for s in states) <= 1e-13
        for r in (10, 50, 400):
            lowers.append(gm[r])
            uppers.append(gm[r] * states[r].ratio)
            want = C.exact(mem, n, states[r].prob)[2]
            assert abs(states[r].ratio - float(want)) <= 1e-12 * float(want), (start, r)
        assert states[400].ratio < states[50].ratio < states[10].ratio < states[0].ratio and states[400].ratio < 1.01
        assert gm[400] > gm[0] * 1.05                                   # the condition: the start is not the optimum
    assert max(lowers) <= min(uppers)
    assert C.same_state(C.trajectory(name, "legacy", 400)[40], C.mirror(name, "legacy", 40)) is None


def test_scores_and_marginals_against_exact_arithmetic():
    """After 40 rounds on the W = 2 table: pi and G from the exact p agree with the reported ones to the sums'
    rounding (at most D adds for pi, k adds and a division for G)."""
    rows, n = C.table("W2")
    mem = P.members(rows, n)
    st = C.mirror("W2", "legacy", 40)
    pi, G, _ = C.exact(mem, n, st.prob)
    assert max(abs(float(x) - y) / y for x, y in zip(pi, st.marginals) if y) <= len(rows) * 2.0 ** -53
    assert max(abs(float(x) - y) / y for x, y in zip(G, st.scores)) <= (len(rows) + 12) * 2.0 ** -53
    assert st.best_row == int(np.argmax(st.scores))
    assert (st.marginals == 0.0).tolist() == [i not in M.covered(rows, n) for i in range(n)]


def test_start_arguments_and_empty_table():
    St = pkg("stats")
    rows, n = C.table("W1")
    mult, total = C.mults(len(rows))
    st = St.rows_nash_host(rows, n, 0, mult, total)
    assert np.array_equal(st.prob, mult / np.float64(total)) and st.rounds == 0
    assert C.same_state(St.rows_nash_host(rows, n, 0, mult), st) is None            # the total defaults to the sum
    assert np.array_equal(St.rows_nash_host(rows, n, 0).prob, np.full(len(rows), 1.0 / len(rows)))
    again = St.rows_nash_host(rows, n, 0, state=st)                                  # no start, no rounds: nothing
    assert C.same_state(again, st) is None
    empty = St.rows_nash_host(rows[:0], n, 3)
    assert C.same_state(empty, C.nash_loop([], n, 3)) is None
    assert (empty.ratio, empty.rounds, empty.best_row, empty.psum) == (np.inf, 0, P.PRICE_NONE, 0.0)
    assert len(empty.prob) == 0 and P.bits(empty.marginals).tolist() == [0] * n
    assert C.same_state(St.rows_nash_host(rows[:0], n, 2, state=empty), empty) is None
    for bad in (dict(rounds=-1), dict(n=65), dict(n=0), dict(mult=mult[:5]), dict(mult=mult, total=0),
                dict(state=empty)):
        args = dict(n=n, rounds=3)
        args.update(bad)
        with pytest.raises(ValueError):
            St.rows_nash_host(rows, **args)


C_TYPES = {"const uint64_t *": ctypes.c_void_p, "const uint32_t *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "double *": ctypes.c_void_p, "uint64_t *": ctypes.c_void_p, "void *": ctypes.c_void_p,
           "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32}


def _declared_args(text, res, name):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), text)
    assert m, name + " is not declared in include/csa_legacy.h"
    if m.group(1).strip() == "void":
        return []
    return [C_TYPES[re.match(r"(.*?)\w+$", " ".join(a.split())).group(1).strip()] for a in m.group(1).split(",")]


def test_symbols_declared_as_bound():
    N = pkg("_native")
    with open(N.HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, res, ctype, count in (("csa_rows_nash_async", "int", ctypes.c_int, 16),
                                    ("csa_rows_marginals_async", "int", ctypes.c_int, 11),
                                    ("csa_rows_nash_scratch_bytes", "uint64_t", ctypes.c_uint64, 2),
                                    ("csa_rows_marginals_scratch_bytes", "uint64_t", ctypes.c_uint64, 2),
                                    ("csa_rows_nash_tile", "uint32_t", ctypes.c_uint32, 0)):
        got, bound = N.SIGNATURES[name]
        assert got is ctype and bound == _declared_args(text, res, name) and len(bound) == count, name
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+CSA_NASH_START\s+0x1u", text) and N.CSA_NASH_START == 1
    assert int(N.lib().csa_rows_nash_tile()) == C.TILE == pkg("stats").NASH_TILE


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every refusal of csa_rows_nash_async and csa_rows_marginals_async comes before any device call: the
    pointers here are host memory."""
    N = pkg("_native")
    L = N.lib()
    cap, W, n = 4, 2, 100
    need = int(L.csa_rows_nash_scratch_bytes(cap, W))
    part = int(L.csa_rows_marginals_scratch_bytes(cap, W))
    assert need % 8 == 0 and part == (64 * W + 1) * 8
    assert need >= int(L.csa_rows_price_scratch_bytes(cap, W)) + part + 64 * W * 12
    bufs = [(ctypes.c_uint64 * 4096)() for _ in range(8)]
    rows, length, mult, prob, sc, pi, state, scratch = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    inside = lambda p, off: ctypes.c_void_p(p.value + off)

    def nash(rows=rows, length=length, cap=cap, W=W, n=n, rounds=3, flags=1, mult=mult, total=9, prob=prob, sc=sc,
             pi=pi, state=state, scratch=scratch, bytes_=need):
        return L.csa_rows_nash_async(rows, length, cap, W, n, rounds, flags, mult, total, prob, sc, pi, state, scratch,
                                     bytes_, None)

    for bad in (dict(n=129), dict(n=0), dict(n=-3), dict(W=0), dict(length=None), dict(rows=None), dict(flags=2),
                dict(flags=3), dict(prob=None), dict(sc=None), dict(pi=None), dict(state=None), dict(total=0),
                dict(scratch=None), dict(bytes_=need - 1), dict(scratch=inside(scratch, 4)), dict(sc=prob),
                dict(pi=inside(prob, 8)), dict(state=inside(sc, 8)), dict(prob=rows), dict(sc=length),
                dict(state=inside(scratch, need - 8)), dict(prob=mult), dict(pi=inside(mult, 4))):
        assert nash(**bad) == N.CSA_E_INVALID, bad
        assert "rows nash" in N.last_error(), bad
    assert nash(cap=2 ** 32 - 1, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    assert nash(W=4096, n=100, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    assert nash(rounds=0, flags=0) == N.CSA_OK                      # no start, no rounds: nothing is launched
    assert nash(rounds=0, flags=0, total=0) == N.CSA_OK             # the total matters under START alone

    def marginals(rows=rows, length=length, cap=cap, W=W, n=n, prob=prob, pi=pi, psum=state, scratch=scratch,
                  bytes_=part):
        return L.csa_rows_marginals_async(rows, length, cap, W, n, prob, pi, psum, scratch, bytes_, None)

    for bad in (dict(n=129), dict(n=0), dict(W=0), dict(length=None), dict(rows=None), dict(prob=None), dict(pi=None),
                dict(psum=None), dict(scratch=None), dict(bytes_=part - 1), dict(scratch=inside(scratch, 4)),
                dict(pi=prob), dict(psum=inside(pi, 16)), dict(pi=inside(rows, 8)), dict(psum=length),
                dict(pi=inside(scratch, 8))):
        assert marginals(**bad) == N.CSA_E_INVALID, bad
        assert "rows marginals" in N.last_error(), bad
    assert marginals(cap=2 ** 32 - 1, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    assert marginals(W=4096, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED


def _distribution(rows, n, ids, mult=None):
    St = pkg("stats")
    mult = np.ones(len(rows), np.int64) if mult is None else mult
    return St.PanelDistribution(int(mult.sum()), np.arange(len(rows)), mult, rows, n, ids)


def test_distribution_nash_on_a_host_table():
    """PanelDistribution.nash over a host table, before and after pickling: the fields from the mirror's run, and a
    portfolio that portfolio_probabilities' host-side packing accepts and that gives alloc back."""
    St, A = pkg("stats"), pkg("analysis")
    rows, n = C.table("W1")
    mult, total = C.mults(len(rows))
    ids = ["p%02d" % i for i in range(n)]
    st0, st = C.mirror("W1", "legacy", 0), C.mirror("W1", "legacy", 40)
    dist = pickle.loads(pickle.dumps(_distribution(rows, n, ids, mult)))
    got = dist.nash(40)
    assert isinstance(got, St.PanelNash) and not St._is_device_tensor(dist.table().rows) and dist.S == total
    held = M.covered(rows, n)
    assert np.array_equal(got.probabilities, st.prob / np.float64(st.psum)) and got.rounds == 40
    assert got.alloc == {ids[i]: float(st.marginals[i] / np.float64(st.psum)) for i in range(n)}
    assert got.covered_agents == frozenset(ids[i] for i in held) and len(held) == n - 1
    assert got.output_lines == ["Agent %s not contained in any drawn panel." % ids[i] for i in range(n) if i not in held]
    assert got.geometric_mean == C.geometric_mean(st.marginals, st.psum)
    assert got.start_geometric_mean == C.geometric_mean(st0.marginals, st0.psum)
    assert P.bits1(got.gap) == P.bits1(st.ratio) and got.upper == got.geometric_mean * got.gap
    assert got.start_geometric_mean < got.geometric_mean <= got.upper
    mem = P.members(rows, n)
    assert got.best_row == st.best_row and got.best_panel == frozenset(ids[i] for i in mem[st.best_row])
    # the portfolio
    panels, probs = got.portfolio()
    keep = [d for d in range(len(rows)) if got.probabilities[d] >= 1e-9]
    assert 0 < len(keep) < len(rows)                                        # the threshold drops some rows here
    assert panels == [frozenset(ids[i] for i in mem[d]) for d in keep]
    assert abs(math.fsum(probs) - 1.0) <= 1e-12 and min(probs) > 0
    assert probs == [float(got.probabilities[d]) / math.fsum(float(got.probabilities[d]) for d in keep) for d in keep]
    pos = {aid: i for i, aid in enumerate(ids)}
    x, packed = A._membership(panels, n, pos.__getitem__)
    assert np.array_equal(packed, rows[keep]) and np.array(probs, np.float64).shape == (len(keep),)
    every, all_probs = got.portfolio(0.0)
    assert len(every) == len(rows) and abs(math.fsum(all_probs) - 1.0) <= 1e-12
    again = pickle.loads(pickle.dumps(got))
    assert again == got and again.portfolio() == (panels, probs) and again != dist.nash(39)
    # the other start, no rounds, the defaults
    uniform = dist.nash(40, start="uniform")
    assert np.array_equal(uniform.probabilities, C.mirror("W1", "uniform", 40).prob / np.float64(C.mirror("W1", "uniform", 40).psum))
    none = dist.nash(0)
    assert none.rounds == 0 and none.geometric_mean == none.start_geometric_mean
    assert np.array_equal(none.probabilities, (mult / np.float64(total)) / np.float64(st0.psum))
    assert dist.nash().rounds == 200
    for bad in (dict(rounds=-1), dict(start="leximin"), dict(start=None)):
        with pytest.raises(ValueError):
            dist.nash(**bad)


def test_empty_run():
    St = pkg("stats")
    rows, n = C.table("W1")
    ids = list(range(n))
    empty = St.PanelDistribution(0, np.zeros(0, np.int64), np.zeros(0, np.int64), rows[:0], n, ids)
    none = empty.nash()
    assert len(none.probabilities) == 0 and none.rounds == 0 and none.best_row is None and none.best_panel == frozenset()
    assert none.covered_agents == frozenset() and len(none.output_lines) == n and none.portfolio() == ([], [])
    assert (none.geometric_mean, none.start_geometric_mean, none.gap, none.upper) == (0.0, 0.0, np.inf, np.inf)
    assert set(none.alloc.values()) == {0.0} and pickle.loads(pickle.dumps(none)) == none
    with pytest.raises(ValueError):
        empty.nash(-1)


def test_world_beyond_one_is_refused(monkeypatch):
    A, D = pkg("analysis"), pkg("distributed")
    inst, _ = P.instance("example_small_20", 20)
    monkeypatch.setattr(D, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size 2"):
        A.legacy_nash(inst, 10, 0)


def test_names_are_exported():
    top = pkg()
    for name in ("legacy_nash", "PanelNash", "NashState", "rows_nash_host", "rows_marginals_host"):
        assert name in top.__all__ and hasattr(top, name) and name in top.__doc__
    St = pkg("stats")
    for cls in (St.HostRowTables, St.DeviceRowTables):
        assert hasattr(cls, "nash") and hasattr(cls, "marginals")
    assert hasattr(St, "NashBuffers") and hasattr(St, "nash_buffers_host") and hasattr(St, "rows_nash_device")
    assert hasattr(St, "rows_marginals_device")
