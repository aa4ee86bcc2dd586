"""Two sorted distinct-row tables side by side, without a GPU: the numpy mirrors of csa_rows_join_async and
csa_rows_find_async (stats.rows_join_host / rows_find_host) against np.unique and Counter arithmetic
(join_cases), the entry points' argument validation (refused on the host before any device call), and what
stands on them -- analysis.PanelSet's set algebra over host rows, stats.compare_panel_distributions and
stats.portfolio_overlap -- against Python's own set operators and integer arithmetic over the C oracle's
panels.  Every assertion is integer or bit-for-bit float equality."""
import ctypes
import operator
import pickle

import numpy as np
import pytest

import join_cases as J
import rows_cases as R
from conftest import pkg
from multiplicity_cases import oracle_panels

T_HOST = 64
IDS = ["agent%02d" % i for i in range(20)]       # couples: 20 agents, panels of 2


def _same(got, want):
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
    assert [int(x) for x in got[4]] == want[4]


@pytest.mark.parametrize("W", [1, 2, 27])
@pytest.mark.parametrize("name", R.MERGE_NAMES)
def test_join_mirror_equals_numpy(name, W):
    S = pkg("stats")
    a, b = R.merge_pairs(W, M=T_HOST)[name]
    for mults in (True, False):
        ta, tb = ((t[0], t[2] if mults else None) for t in (a, b))
        for select in J.SELECTS:
            scales = (int(a[2].sum()), int(b[2].sum())) if mults else (len(a[0]), len(b[0]))
            got, want = S.rows_join_host(ta, tb, select, scales), J.np_join(ta, tb, select, scales)
            _same(got, want)
            assert got[0].shape == (want[3], W) and got[0].dtype == np.uint64
            if name in ("interleaved", "a_below_b"):
                assert got[4][1:4] == [0, len(a[0]), len(b[0])]
            if name == "equal":
                assert got[4][1:4] == [len(a[0]), 0, 0]


def test_join_mirror_overflow_word():
    S = pkg("stats")
    rows = R.ascending(5, 2)
    big = np.full(5, 2 ** 32 - 1, np.int64)
    got = S.rows_join_host((rows, big), (rows, big), 4, (2 ** 32 - 1, 2 ** 32 - 1))
    _same(got, J.np_join((rows, big), (rows, big), 4, (2 ** 32 - 1, 2 ** 32 - 1)))
    assert got[4][10] == 1
    assert S.rows_join_host((rows, big), (rows, big), 4)[4][8:] == [5 * (2 ** 32 - 1) ** 2 % 2 ** 64, 5 * (2 ** 32 - 1), 1]
    with pytest.raises(ValueError):
        S.rows_join_host((rows, big), (rows, big), 8)
    with pytest.raises(ValueError):
        S.rows_join_host((rows, big), (rows, big), 4, (2 ** 32, 1))


@pytest.mark.parametrize("W", [1, 27])
def test_find_mirror_equals_numpy(W):
    S = pkg("stats")
    table = J.find_table(W)
    batches, want = J.query_batches(table)
    for name, q in batches.items():
        got = S.rows_find_host(table, q)
        assert got.dtype == np.int64 and np.array_equal(got, want[name]), name
    assert S.rows_find_host(table[:0], batches["present"]).tolist() == [J.MISSING] * 300
    assert S.FIND_MISSING == J.MISSING
    T = S.HostRowTables()
    t = S.RowTable(table, None, None, np.array([100], np.uint64), len(table), W)      # the length bounds the search
    assert np.array_equal(T.find(t, batches["ends"]), J.np_find(table[:100], batches["ends"]))


def test_argument_validation_without_a_device():
    N = pkg("_native")
    L = N.lib()
    T = L.csa_rows_sort_tile()
    for W in (1, 27):
        m = [L.csa_rows_join_scratch_bytes(n, 100, W) for n in (0, 1, T - 1, T, T + 1, 8 * T + 3, 1 << 20)]
        m2 = [L.csa_rows_join_scratch_bytes(100, n, W) for n in (0, 1, T - 1, T, T + 1, 8 * T + 3, 1 << 20)]
        assert m == sorted(m) and m2 == sorted(m2) and m[0] > 0
        assert all(L.csa_rows_join_scratch_bytes(n, 100, W) >= L.csa_rows_merge_scratch_bytes(n, 100, W) for n in (0, T))
    p = ctypes.c_void_p(0x1000)      # never dereferenced: every call below is refused before any device call
    q, r = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000)
    big = 1 << 40
    la, lb, lo = (ctypes.c_void_p(0x400000 + 8 * i) for i in range(3))
    rec, status = ctypes.c_void_p(0x500000), ctypes.c_void_p(0x600000)
    o = ctypes.c_void_p(0x300000)

    def join(a=(p, p, la, 10), b=(q, q, lb, 10), W=2, select=7, scales=(1, 1), scratch=r, sb=big, out=(o, o, o),
             cap_out=20, out_len=lo, record=rec, status=status):
        return L.csa_rows_join_async(*a, *b, W, select, *scales, scratch, sb, *out, cap_out, out_len, record, status,
                                     None)

    assert join(sb=L.csa_rows_join_scratch_bytes(10, 10, 2), a=(p, p, la, 1 << 31),
                b=(q, q, lb, 1 << 31)) == N.CSA_E_UNSUPPORTED          # refused for the capacities alone
    assert join(W=0) == N.CSA_E_INVALID
    assert join(a=(p, p, None, 10)) == N.CSA_E_INVALID
    assert join(b=(q, q, None, 10)) == N.CSA_E_INVALID
    assert join(out_len=None) == N.CSA_E_INVALID
    assert join(record=None) == N.CSA_E_INVALID
    assert join(status=None) == N.CSA_E_INVALID
    assert join(a=(None, p, la, 10)) == N.CSA_E_INVALID
    assert join(b=(None, None, lb, 10)) == N.CSA_E_INVALID
    assert join(scratch=None) == N.CSA_E_INVALID
    assert join(sb=L.csa_rows_join_scratch_bytes(10, 10, 2) - 1) == N.CSA_E_INVALID
    assert join(out=(p, None, None)) == N.CSA_E_INVALID                          # the output rows alias A
    assert join(out=(ctypes.c_void_p(0x100000 + 16), None, None)) == N.CSA_E_INVALID   # ... overlap B
    assert join(out=(None, p, None)) == N.CSA_E_INVALID                          # a mult output aliases A's mults
    assert join(out=(None, None, ctypes.c_void_p(0x100000 + 4))) == N.CSA_E_INVALID
    assert join(out_len=la) == N.CSA_E_INVALID
    assert join(record=ctypes.c_void_p(0x400000 - 80)) == N.CSA_E_INVALID       # the record's last word is A's length
    assert join(select=8) == N.CSA_E_INVALID
    assert join(scales=(1 << 32, 1)) == N.CSA_E_INVALID
    assert join(scales=(1, 1 << 32)) == N.CSA_E_INVALID
    assert join(a=(p, p, la, 1 << 31), b=(q, q, lb, 1 << 31)) == N.CSA_E_UNSUPPORTED
    assert "rows join" in N.last_error()

    def find(rows=p, ln=la, cap=10, W=2, queries=q, n=5, out=r):
        return L.csa_rows_find_async(rows, ln, cap, W, queries, n, out, None)

    assert find(W=0) == N.CSA_E_INVALID
    assert find(ln=None) == N.CSA_E_INVALID
    assert find(rows=None) == N.CSA_E_INVALID
    assert find(queries=None) == N.CSA_E_INVALID
    assert find(out=None) == N.CSA_E_INVALID
    assert find(out=p) == N.CSA_E_INVALID                                        # the output aliases the table
    assert find(out=ctypes.c_void_p(0x100000 + 8)) == N.CSA_E_INVALID            # ... overlaps the queries
    assert find(cap=(1 << 32) - 1) == N.CSA_E_UNSUPPORTED
    assert "rows find" in N.last_error()
    assert find(n=0, queries=None, out=None) == N.CSA_OK                         # nothing to do, nothing launched
    assert L.csa_version() == 1


# --- PanelSet's algebra over host rows ----------------------------------------------------------------------

OPERATORS = [operator.and_, operator.or_, operator.sub, operator.xor]
COMPARISONS = [operator.le, operator.lt, operator.ge, operator.gt]
METHODS = ["intersection", "union", "difference", "symmetric_difference", "isdisjoint", "issubset", "issuperset"]


def _found(panels):
    A = pkg("analysis")
    return A.PanelSet(len(np.unique(panels, axis=0)), panels.copy(), len(IDS), IDS)


def check_algebra(make_a, make_b, sa, sb):
    """Every operator, comparison and method of two PanelSets (fresh ones per expression from ``make_*``) against
    Python's on the decoded sets ``sa`` and ``sb``; also with a plain set on either side."""
    A = pkg("analysis")
    for op in OPERATORS:
        want = op(sa, sb)
        for left, right in ((make_a(), make_b()), (make_a(), set(sb)), (set(sa), make_b()), (make_a(), frozenset(sb))):
            got = op(left, right)
            assert isinstance(got, A.PanelSet) and len(got) == len(want) and set(got) == want, op
            assert got == want and J.tuples(op(left, right).rows(), IDS) == want
    for op in COMPARISONS:
        for x, y, mx, my in ((sa, sb, make_a, make_b), (sa & sb, sa, lambda: make_a() & make_b(), make_a),
                             (sa, sa & sb, make_a, lambda: make_a() & make_b()), (sa, sa, make_a, make_a)):
            assert op(mx(), my()) is op(x, y) and op(mx(), set(y)) is op(x, y) and op(set(x), my()) is op(x, y), op
    for name in METHODS:
        for y, my in ((sb, make_b), (sa - sb, lambda: make_a() - make_b()), (sa & sb, lambda: make_a() & make_b())):
            want = getattr(sa, name)(y)
            for right in (my(), set(y), list(y)):
                got = getattr(make_a(), name)(right)
                assert (got == want and len(got) == len(want)) if isinstance(want, set) else got is want, name
    probe = sorted(sa)[:5] + sorted(sb - sa)[:3] + sorted(sa)[:2]
    assert make_a().contains_many(probe).tolist() == [p in sa for p in probe]
    assert make_a().contains_many([]).tolist() == []


@pytest.mark.parametrize("S,distinct,shared", [(300, (92, 95), 88), (40, (35, 33), 16)])
def test_panelset_algebra_on_host_rows(S, distinct, shared):
    A = pkg("analysis")
    pa, pb = oracle_panels(J.COUPLES, 2, 0, S), oracle_panels(J.COUPLES, 2, 1, S)
    sa, sb = J.tuples(np.unique(pa, axis=0), IDS), J.tuples(np.unique(pb, axis=0), IDS)
    assert (len(sa), len(sb)) == distinct and len(sa & sb) == shared
    assert sa - sb and sb - sa and sa & sb                       # all three classes occur: a condition on the input
    assert (len(sa - sb), len(sb - sa)) == (distinct[0] - shared, distinct[1] - shared)
    check_algebra(lambda: _found(pa), lambda: _found(pb), sa, sb)
    unpickled = lambda p: (lambda: pickle.loads(pickle.dumps(_found(p))))
    check_algebra(unpickled(pa), unpickled(pb), sa, sb)
    check_algebra(lambda: _found(pa), unpickled(pb), sa, sb)
    # a op a
    a = _found(pa)
    assert (a & a) == sa and (a | a) == sa and len(a - a) == 0 and len(a ^ a) == 0 and set(a - a) == set()
    assert a <= a and a >= a and not a < a and not a > a and not a.isdisjoint(a) and (a - a).isdisjoint(a)
    # what stays: membership, equality, iteration, the pickle
    assert sorted(a) == sorted(sa) and sorted(sa)[0] in a and a == _found(pa) and a != _found(pb)
    assert np.array_equal(pickle.loads(pickle.dumps(a & _found(pb))).rows(), (a & _found(pb)).rows())
    # errors
    with pytest.raises(KeyError):
        a & {("agent00", "nobody")}
    with pytest.raises(KeyError):
        a.contains_many([("nobody",)])
    other = A.PanelSet(len(sa), pa.copy(), len(IDS), ["x%d" % i for i in range(20)])
    with pytest.raises(ValueError, match="different instances"):
        a & other
    with pytest.raises(ValueError, match="different instances"):
        a <= A.PanelSet(len(sa), np.zeros((1, 1), np.uint64), 19, IDS[:19])
    empty = A.PanelSet(len(sa), None, len(IDS), IDS)             # a run with keep_panels=False
    for expr in (lambda: a & empty, lambda: empty | a, lambda: empty <= a, lambda: a.isdisjoint(empty),
                 lambda: empty & sa, lambda: sa - empty, lambda: empty.contains_many([])):
        with pytest.raises(RuntimeError, match="panels were not kept"):
            expr()


# --- two runs side by side ----------------------------------------------------------------------------------

def _distribution(panels, n, ids=None):
    S = pkg("stats")
    first, mult = S.panel_multiplicities_host(panels)
    return S.PanelDistribution(len(panels), first, mult, panels, n, list(range(n)) if ids is None else ids)


def test_distribution_table():
    S = pkg("stats")
    panels = oracle_panels(J.COUPLES, 2, 0, 300)
    d = _distribution(panels, 20)
    t = d.table()
    want = R.np_table(panels)
    assert np.array_equal(t.rows, want[0]) and np.array_equal(t.first, want[1]) and np.array_equal(t.mult, want[2])
    assert int(t.length[0]) == t.cap == d.distinct == 92 and d.table() is t
    back = pickle.loads(pickle.dumps(d)).table()
    assert np.array_equal(back.rows, want[0]) and np.array_equal(back.mult, want[2])
    first, mult = S.panel_multiplicities_host(panels)
    with pytest.raises(RuntimeError, match="panels were not kept"):
        S.PanelDistribution(300, first, mult, None, 20, list(range(20))).table()
    forged = S.PanelDistribution(300, first, mult, panels, 20, list(range(20)))
    forged.S = 299
    with pytest.raises(RuntimeError, match="sum to 300"):
        forged.table()


@pytest.mark.parametrize("name,k,S", [(J.COUPLES, 2, 300), (J.COUPLES, 2, 10 ** 4), ("sf_e_tight_110", 110, 2000)])
def test_compare_panel_distributions(name, k, S):
    St = pkg("stats")
    pa, pb = oracle_panels(name, k, 0, S), oracle_panels(name, k, 1, S)
    n = pa.shape[1] * 64
    a, b = _distribution(pa, n), _distribution(pb, n)
    c = St.compare_panel_distributions(a, b)
    want = J.check_comparison(c, pa, pb)
    if S == 10 ** 4:
        assert want[:4] == [100, 100, 0, 0]                   # every panel possible was drawn by both runs
    if name != J.COUPLES:
        assert want[1] == 0 and c.overlap() == 0.0 and c.total_variation() == 1.0 and c.jaccard() == 0.0
    # the mirror image, and through pickles
    J.check_comparison(St.compare_panel_distributions(b, a), pb, pa)
    assert St.compare_panel_distributions(pickle.loads(pickle.dumps(a)), b) == c
    # a run beside itself
    same = St.compare_panel_distributions(a, _distribution(pa, n))
    J.check_comparison(same, pa, pa)
    assert same.total_variation() == 0.0 and same.overlap() == 1.0 and same.jaccard() == 1.0
    assert same.cross_collision() == a.sum_squares / (S * S)
    assert same.only_a == same.only_b == 0 and same.mass_a_on_b() == 1.0


def test_compare_degenerate_and_refused():
    St = pkg("stats")
    pa = oracle_panels(J.COUPLES, 2, 0, 300)
    a, none = _distribution(pa, 20), _distribution(pa[:0], 20)
    for x, y, px, py in ((a, none, pa, pa[:0]), (none, a, pa[:0], pa), (none, none, pa[:0], pa[:0])):
        c = St.compare_panel_distributions(x, y)
        J.check_comparison(c, px, py)
        assert [c.jaccard(), c.mass_a_on_b(), c.mass_b_on_a(), c.overlap(), c.total_variation(),
                c.cross_collision()] == [0.0] * 6
    with pytest.raises(ValueError, match="different instances"):
        St.compare_panel_distributions(a, _distribution(pa, 20, ["x%d" % i for i in range(20)]))
    with pytest.raises(ValueError, match="different instances"):
        St.compare_panel_distributions(a, _distribution(pa, 19))
    first, mult = St.panel_multiplicities_host(pa)
    with pytest.raises(RuntimeError, match="panels were not kept"):
        St.compare_panel_distributions(a, St.PanelDistribution(300, first, mult, None, 20, list(range(20))))
    forged = _distribution(pa, 20)
    forged.table().mult[0] += 1                                  # the record's sum no longer is the run's S
    with pytest.raises(RuntimeError, match="sum to 300 and 301"):
        St.compare_panel_distributions(a, forged)


def test_portfolio_overlap_equals_the_loop():
    St = pkg("stats")
    panels = oracle_panels(J.COUPLES, 2, 0, 300)
    rows, weights = J.portfolio_case(panels, 20, 2)
    want = J.overlap_loop(panels, rows, weights)
    assert want["panels"] == 50 and want["panels_seen"] == 40 and 0 < want["overlap"] < 1
    d = _distribution(panels, 20)
    J.check_overlap(St.portfolio_overlap(d, rows, weights), want)
    J.check_overlap(St.portfolio_overlap(pickle.loads(pickle.dumps(d)), rows, weights), want)
    probe = J.tuples(rows[:1], list(range(20))).pop()
    assert d.count(probe) == want["counts"][0]
    nothing = St.portfolio_overlap(_distribution(panels[:0], 20), rows, weights)
    assert (nothing.legacy_mass, nothing.portfolio_mass_seen, nothing.overlap, nothing.panels_seen) == (0.0, 0.0, 0.0, 0)
    none = St.portfolio_overlap(d, rows[:0], weights[:0])
    assert (none.panels, none.legacy_mass, none.portfolio_mass_seen, none.overlap) == (0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        St.portfolio_overlap(d, rows, weights[:-1])
