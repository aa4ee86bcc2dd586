"""The maximin lottery over drawn panels on the host: stats.rows_maximin_host (csa_rows_maximin_async's contract
in numpy) against the plain Python loop of maximin_cases, its bounds against the LP itself (scipy's HiGHS, tests
only), the product path PanelDistribution.maximin over host tables, and the entry point's refusals, which need no
device."""
import ctypes
import pickle
from fractions import Fraction

import numpy as np
import pytest

import maximin_cases as M
import price_cases as P
from conftest import pkg


def _loop_and_mirror(rows, n, rounds, shrink, resync):
    St = pkg("stats")
    mem = P.members(rows, n)
    want = M.maximin_loop(mem, n, rows.shape[1], rounds, shrink, resync)
    got = St.rows_maximin_host(rows, n, rounds, shrink, resync)
    return got, want


@pytest.mark.parametrize("shrink", [0.8, 0.95])
@pytest.mark.parametrize("resync", [1, 7, 16])
def test_mirror_is_the_loop(resync, shrink):
    """Weights, scores, cover, row counts, picks, upper: bit for bit, with rounds that are no multiple of resync;
    random subsets at W = 2 with a ragged n, and a skewed table whose picks repeat."""
    for rows, n, rounds in ((P.subset_rows(300, 2, 91, k=9), 91, 45), (M.skewed_rows(300, 20, 5), 20, 75)):
        (picks, state), (want_picks, want) = _loop_and_mirror(rows, n, rounds, shrink, resync)
        assert picks.tolist() == want_picks
        assert M.same_state(state, want) is None, M.same_state(state, want)
        assert state.rounds == rounds and int(state.cover.sum()) == rounds * len(P.members(rows[:1], n)[0])
        assert len(set(want_picks)) < rounds or n == 91


@pytest.mark.parametrize("table", ["couples", "sf_e_110"])
def test_mirror_is_the_loop_on_oracle_tables(table):
    """The C oracle's tables: couples (W = 1, k = 2) and sf_e_110 (W = 27, S = 300, agents no panel holds)."""
    name, k, S, seed, _ = P.COVER_TABLES[table]
    _, ids = P.instance(name, k)
    rows = P.oracle_table(name, k, seed, S)[1]
    n = len(ids)
    rounds = 40 if table == "couples" else 10
    (picks, state), (want_picks, want) = _loop_and_mirror(rows, n, rounds, 0.8, 7)
    assert picks.tolist() == want_picks and M.same_state(state, want) is None
    if table == "sf_e_110":
        assert (state.weights == 0.0).sum() == 10 and not state.cover[state.weights == 0.0].any()


def test_update_order_shows_in_the_bits():
    """Every call ends on freshly summed scores, so the order of the update pass's sums shows only through a
    pick.  A forged state makes it: scores that the ascending sums cancel to +0.0 exactly, so the second pick is
    row 0, while the descending sums leave a last-bit residue and pick another row (the condition on the input,
    asserted).  The mirror continues that state as the ascending loop does."""
    St = pkg("stats")
    rows, n, p0 = M.skewed_rows(1000, 70, 9), 70, 17
    mem = P.members(rows, n)
    forged = M.forged_order_state(rows, n, p0)
    up_picks, up = M.maximin_loop(mem, n, 2, 2, 0.8, 16, state=forged)
    down_picks, _ = M.maximin_loop(mem, n, 2, 2, 0.8, 16, state=forged, descending=True)
    assert up_picks == [p0, 0] and down_picks[0] == p0 and down_picks[1] != 0
    picks, state = St.rows_maximin_host(rows, n, 2, 0.8, 16, state=St.MaximinState(**forged))
    assert picks.tolist() == up_picks and M.same_state(state, up) is None


@pytest.mark.parametrize("case", M.SKEWED)
def test_bounds_hold_against_the_lp(case):
    """lower <= z* <= upper with HiGHS's 1e-9 feasibility tolerance (far above the n 2^-53 rounding of a score
    and a sum), at resync 16; the smallest table also at 1 and 64.  Conditions on the inputs, asserted: z* lies
    below the trivial k / covered, and lower is positive."""
    D, n, k, shrink, rounds = case
    rows = M.skewed_rows(D, n, k)
    z = M.lp_optimum(D, n, k)
    held = len(M.covered(rows, n))
    assert held < n and z < k / held - 1e-6
    for resync in ((1, 16, 64) if n == 20 else (16,)):
        picks, state = M.mirror(D, n, k, shrink, rounds, resync)
        lower = M.lower_bound(state, rounds)
        print(case, "rows", len(rows), "covered", held, "resync", resync, "z*", z, "lower", float(lower), "upper",
              state.upper)
        assert lower > 0
        assert float(lower) <= z + 1e-9 and z <= state.upper + 1e-9
    if n == 20:
        assert len(rows) == 261 and held == 19 and abs(z - 0.2) < 1e-9


def test_invariants():
    """sum(counts) == rounds; cover sums to rounds k; lower is the portfolio's exact minimum selection
    probability recomputed from the row counts."""
    D, n, k, shrink, rounds = M.SKEWED[0]
    rows = M.skewed_rows(D, n, k)
    picks, state = M.mirror(D, n, k, shrink, rounds)
    assert int(state.row_count.sum()) == rounds == state.rounds and int(state.cover.sum()) == rounds * k
    assert np.array_equal(np.bincount(picks, minlength=len(rows)), state.row_count)
    mem = P.members(rows, n)
    again = [Fraction(sum(int(state.row_count[d]) for d, row in enumerate(mem) if i in row), rounds) for i in range(n)]
    assert again == [Fraction(int(c), rounds) for c in state.cover]
    assert M.lower_bound(state, rounds) == min(again[i] for i in M.covered(rows, n))


def test_partition_table():
    """Six disjoint panels of four: the picks cycle, every agent is covered 10 times, both bounds are 1/6."""
    St = pkg("stats")
    rows = M.partition_rows(24, 4)
    picks, state = St.rows_maximin_host(rows, 24, 60, 0.8, 7)
    assert picks.tolist() == list(range(6)) * 10
    assert state.cover.tolist() == [10] * 24 and state.row_count.tolist() == [10] * 6
    assert M.lower_bound(state, 60) == Fraction(1, 6) and abs(state.upper - 1 / 6) <= 1e-15
    want = M.maximin_loop(P.members(rows, 24), 24, 1, 60, 0.8, 7)
    assert picks.tolist() == want[0] and M.same_state(state, want[1]) is None


def test_uncovered_agents():
    """Three agents that no row holds keep weight +0.0 and cover 0 and leave the lower bound as it was."""
    St = pkg("stats")
    D, n, k, shrink, rounds = M.SKEWED[0]
    rows = M.skewed_rows(D, n, k)
    rounds = 100
    picks, state = St.rows_maximin_host(rows, n, rounds, shrink)
    more_picks, more = St.rows_maximin_host(rows, n + 3, rounds, shrink)
    assert P.bits(more.weights[n:]).tolist() == [0] * 3 and more.cover[n:].tolist() == [0] * 3
    assert M.lower_bound(more, rounds) == M.lower_bound(state, rounds)
    ids = ["a%d" % i for i in range(n + 3)]
    dist = St.PanelDistribution(len(rows), np.arange(len(rows)), np.ones(len(rows), np.int64), rows, n + 3, ids)
    result = dist.maximin(rounds, shrink)
    missing = set(ids[n:]) | {ids[i] for i in range(n) if i not in M.covered(rows, n)}
    assert result.covered_agents == frozenset(ids) - missing and len(missing) == 4
    assert result.output_lines == ["Agent %s not contained in any drawn panel." % a for a in ids if a in missing]
    assert result.lower == M.lower_bound(more, rounds) and all(result.alloc[a] == 0 for a in missing)


@pytest.mark.parametrize("a,resync", [(32, 16), (21, 7), (23, 16), (5, 7)])
def test_continuation(a, resync):
    """a rounds then b rounds: the mirror run the same way equals the loop run the same way; when a is a multiple
    of resync the fresh rounds fall where one call of a + b puts them, so the two equal that call too."""
    St = pkg("stats")
    rows, n, b = M.skewed_rows(300, 20, 5), 20, 30
    mem = P.members(rows, n)
    p1, s1 = St.rows_maximin_host(rows, n, a, 0.8, resync)
    keep = P.bits(s1.weights).copy()
    p2, s2 = St.rows_maximin_host(rows, n, b, 0.8, resync, state=s1)
    assert np.array_equal(P.bits(s1.weights), keep)                      # the input state is left alone
    l1, t1 = M.maximin_loop(mem, n, 1, a, 0.8, resync)
    l2, t2 = M.maximin_loop(mem, n, 1, b, 0.8, resync, state=t1)
    assert p1.tolist() + p2.tolist() == l1 + l2 and M.same_state(s2, t2) is None and s2.rounds == a + b
    whole_picks, whole = St.rows_maximin_host(rows, n, a + b, 0.8, resync)
    same = M.same_state(s2, M.state_dict(whole)) is None and p1.tolist() + p2.tolist() == whole_picks.tolist()
    assert same == (a % resync == 0)


def test_start_and_empty_table():
    St = pkg("stats")
    rows, n = M.skewed_rows(300, 20, 5), 20
    picks, state = St.rows_maximin_host(rows, n, 0)
    held = M.covered(rows, n)
    assert len(picks) == 0 and state.rounds == 0 and not state.cover.any() and not state.row_count.any()
    assert state.weights.tolist() == [1.0 if i in held else 0.0 for i in range(n)]
    assert state.scores.tolist() == [5.0] * len(rows) and state.best_row == 0
    assert state.upper == state.ratio == 5.0 / len(held)
    again_picks, again = St.rows_maximin_host(rows, n, 0, state=state)         # no start, no rounds: nothing
    assert len(again_picks) == 0 and M.same_state(again, M.state_dict(state)) is None
    empty_picks, empty = St.rows_maximin_host(rows[:0], n, 3)
    assert empty_picks.tolist() == [P.NO_ROW] * 3 and empty.rounds == 0 and empty.best_row == P.PRICE_NONE
    assert empty.upper == np.inf and not empty.weights.any() and len(empty.scores) == 0
    want = M.maximin_loop([], n, 1, 3)
    assert want[0] == [P.NO_ROW] * 3 and M.same_state(empty, want[1]) is None
    for bad in (dict(shrink=0.49), dict(shrink=1.0), dict(shrink=np.nan), dict(resync=0), dict(resync=65),
                dict(rounds=-1)):
        args = dict(rounds=3, shrink=0.8, resync=16)
        args.update(bad)
        with pytest.raises(ValueError):
            St.rows_maximin_host(rows, n, **args)
    with pytest.raises(ValueError):
        St.rows_maximin_host(rows, 65, 3)


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Every refusal of csa_rows_maximin_async comes before any device call: the pointers here are host memory."""
    N = pkg("_native")
    L = N.lib()
    assert N.CSA_MAXIMIN_START == 1
    cap, W, n = 4, 2, 100
    need = int(L.csa_rows_maximin_scratch_bytes(cap, W))
    assert need >= int(L.csa_rows_price_scratch_bytes(cap, W)) + 64 * W * 8 and need % 8 == 0
    bufs = [(ctypes.c_uint64 * 4096)() for _ in range(9)]
    rows, length, w, sc, cover, count, state, picks, scratch = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)

    def call(rows=rows, length=length, cap=cap, W=W, n=n, rounds=3, shrink=0.8, resync=16, flags=1, w=w, sc=sc,
             cover=cover, count=count, state=state, picks=picks, scratch=scratch, bytes_=need):
        return L.csa_rows_maximin_async(rows, length, cap, W, n, rounds, shrink, resync, flags, w, sc, cover, count,
                                        state, picks, scratch, bytes_, None)

    inside = lambda p, off: ctypes.c_void_p(p.value + off)
    for bad in (dict(n=129), dict(n=0), dict(n=-3), dict(W=0), dict(length=None), dict(rows=None),
                dict(shrink=0.4999), dict(shrink=1.0), dict(shrink=float("nan")), dict(resync=0), dict(resync=65),
                dict(flags=2), dict(flags=3), dict(w=None), dict(sc=None), dict(cover=None), dict(count=None),
                dict(state=None), dict(scratch=None), dict(bytes_=need - 1), dict(scratch=inside(scratch, 4)),
                dict(sc=w), dict(cover=inside(w, 8)), dict(state=inside(sc, 8)), dict(picks=inside(cover, 4)),
                dict(count=rows), dict(w=length), dict(state=inside(scratch, need - 8)), dict(picks=state)):
        assert call(**bad) == N.CSA_E_INVALID, bad
        assert "rows maximin" in N.last_error(), bad
    assert call(cap=2 ** 32 - 1, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    assert call(W=4096, n=100, bytes_=1 << 40) == N.CSA_E_UNSUPPORTED
    assert call(rounds=0, flags=0) == N.CSA_OK                      # no start, no rounds: nothing is launched


def _distribution(rows, n, ids):
    St = pkg("stats")
    return St.PanelDistribution(len(rows), np.arange(len(rows)), np.ones(len(rows), np.int64), rows, n, ids)


def test_distribution_maximin_on_a_host_table():
    """PanelDistribution.maximin over a host table, before and after pickling: the fields from the mirror's run."""
    St = pkg("stats")
    D, n, k, shrink, rounds = M.SKEWED[0]
    rows = M.skewed_rows(D, n, k)
    ids = ["p%02d" % i for i in range(n)]
    picks, state = M.mirror(D, n, k, shrink, rounds)
    dist = pickle.loads(pickle.dumps(_distribution(rows, n, ids)))
    got = dist.maximin(rounds, shrink)
    assert isinstance(got, St.PanelMaximin) and not St._is_device_tensor(dist.table().rows)
    mem = P.members(rows, n)
    assert got.rows == sorted(set(picks.tolist())) and got.rounds == rounds == sum(got.counts)
    assert got.counts == [int(state.row_count[d]) for d in got.rows]
    assert got.panels == [frozenset(ids[i] for i in mem[d]) for d in got.rows]
    assert got.probabilities == [c / rounds for c in got.counts]
    assert got.alloc == {ids[i]: Fraction(int(state.cover[i]), rounds) for i in range(n)}
    assert got.covered_agents == frozenset(ids[i] for i in M.covered(rows, n))
    assert got.lower == M.lower_bound(state, rounds) and P.bits1(got.upper) == P.bits1(state.upper)
    assert got.portfolio() == (got.panels, got.probabilities)
    assert len(got.output_lines) == 1 and "not contained" in got.output_lines[0]
    # the default number of rounds is 3 n
    assert dist.maximin().rounds == 3 * n
    with pytest.raises(ValueError):
        dist.maximin(10, shrink=0.3)
    empty = St.PanelDistribution(0, np.zeros(0, np.int64), np.zeros(0, np.int64), rows[:0], n, ids)
    none = empty.maximin()
    assert (none.panels, none.counts, none.rounds, none.rows, none.lower) == ([], [], 0, [], 0)
    assert none.covered_agents == frozenset() and len(none.output_lines) == n and none.portfolio() == ([], [])


def test_world_beyond_one_is_refused(monkeypatch):
    A, D = pkg("analysis"), pkg("distributed")
    inst, _ = P.instance("example_small_20", 20)
    monkeypatch.setattr(D, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size 2"):
        A.legacy_maximin(inst, 10, 0)


def test_names_are_exported():
    top = pkg()
    for name in ("legacy_maximin", "PanelMaximin", "MaximinState", "rows_maximin_host"):
        assert name in top.__all__ and hasattr(top, name)
    St = pkg("stats")
    assert hasattr(St.HostRowTables, "maximin") and hasattr(St.DeviceRowTables, "maximin")
