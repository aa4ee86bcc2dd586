"""Two sorted distinct-row tables side by side on the device: csa_rows_join_async and csa_rows_find_async
through the C ABI (the merge's record and merge-path passes, then rj_flag_kernel, the scan, rj_summary_kernel,
rj_pos_kernel, rj_gather_kernel; rj_find_kernel), and the product paths that stand on them -- analysis.PanelSet's
set algebra over kept panels, legacy_panel_comparison, legacy_portfolio_overlap, contains_many.

Expected values come from np.unique and Counter arithmetic (join_cases), from Python's own set operators, and
from the C oracle's panels.  Every assertion is integer or bit-for-bit float equality; every buffer the calls
write carries guard words behind it."""
import operator

import numpy as np
import pytest

import join_cases as J
import rows_cases as R
from conftest import inst_paths, pkg
from multiplicity_cases import oracle_panels
from test_gpu_rows_sort import GUARD, GUARD32, GUARD64, _dev32, _dev64, _guards_ok, _u32

pytestmark = pytest.mark.gpu


def _join(a, b, W, select, scales=(1, 1), cap_a=None, cap_b=None, cap_out=None, outputs=(True, True, True),
          lengths=None, poison=False):
    """One csa_rows_join_async call over tables ``(rows, mult or None)``; capacities default to the lengths.  With
    ``poison`` the entries past the lengths hold rows (half copies of valid rows, half fresh) and mults.  Returns
    (rows, mult_a, mult_b, length, record, status), outputs not asked for as None."""
    import torch
    N = pkg("_native")
    L = N.lib()
    rng = np.random.default_rng(5)

    def side(t, cap, length):
        rows, mult = t
        n = len(rows)
        cap = n if cap is None else cap
        full = np.zeros((cap, W), np.uint64)
        full[:n] = rows
        m = np.zeros(cap, np.int64)
        if mult is not None:
            m[:n] = mult
        if poison and cap > n:
            extra = rng.integers(0, 1 << 64, size=(cap - n, W), dtype=np.uint64)
            if n:
                extra[::2] = rows[rng.integers(0, n, size=len(extra[::2]))]
            full[n:], m[n:] = extra, 0xFFFFFFF0
        return (_dev64(full, GUARD) if cap else None, None if mult is None else _dev32(m, GUARD),
                _dev64(np.array([n if length is None else length], np.uint64)), cap)

    lengths = (None, None) if lengths is None else lengths
    A, B = side(a, cap_a, lengths[0]), side(b, cap_b, lengths[1])
    selected = J.np_join(a, b, select)[3]
    cap_out = selected if cap_out is None else cap_out
    need = int(L.csa_rows_join_scratch_bytes(A[3], B[3], W))
    scratch = torch.full(((need + 7) // 8 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    out = torch.full((cap_out * W + GUARD,), GUARD64, dtype=torch.int64, device="cuda") if outputs[0] else None
    mult_a = torch.full((cap_out + GUARD,), GUARD32, dtype=torch.int32, device="cuda") if outputs[1] else None
    mult_b = torch.full((cap_out + GUARD,), GUARD32, dtype=torch.int32, device="cuda") if outputs[2] else None
    length = torch.full((1 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    record = torch.full((11 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    status = torch.zeros(4 + GUARD, dtype=torch.int32, device="cuda")
    N.check(L.csa_rows_join_async(*(N.ptr(x) for x in A[:3]), A[3], *(N.ptr(x) for x in B[:3]), B[3], W, select,
                                  scales[0], scales[1], N.ptr(scratch), need, N.ptr(out), N.ptr(mult_a), N.ptr(mult_b),
                                  cap_out, N.ptr(length), N.ptr(record), N.ptr(status), None))
    torch.cuda.synchronize()
    assert out is None or _guards_ok(out, cap_out * W, GUARD64)
    assert mult_a is None or _guards_ok(mult_a, cap_out, GUARD32)
    assert mult_b is None or _guards_ok(mult_b, cap_out, GUARD32)
    assert _guards_ok(length, 1, GUARD64) and _guards_ok(record, 11, GUARD64)
    assert _guards_ok(scratch, (need + 7) // 8, GUARD64) and _guards_ok(status, 4, 0)
    for s in (A, B):
        assert s[0] is None or _guards_ok(s[0], s[3] * W, GUARD64)
        assert s[1] is None or _guards_ok(s[1], s[3], GUARD32)
    ln = int(length[0].item())
    d = min(ln, cap_out)
    return (None if out is None else out[:d * W].cpu().numpy().view(np.uint64).reshape(d, W),
            None if mult_a is None else _u32(mult_a, d), None if mult_b is None else _u32(mult_b, d), ln,
            [int(x) for x in record[:11].cpu().numpy().view(np.uint64)], status[:4].cpu().numpy().astype(np.uint32))


def _check(got, want, what):
    assert got[5][0] == 0, what
    assert got[3] == want[3] and got[4] == want[4], what
    for g, w in zip(got[:3], want[:3]):
        assert g is None or np.array_equal(g, w), what


@pytest.mark.parametrize("W", R.WIDTHS)
@pytest.mark.parametrize("name", R.MERGE_NAMES)
def test_join_shapes(gpu_available, name, W):
    """Empty sides, equal lists, interleaved and disjoint ones, lengths straddling the 1024-record merge tile:
    rows, both multiplicity outputs, the length and all 11 record words are numpy's, for every select, with mults
    and with NULL mults; capacities beyond the lengths with poison behind them change nothing; NULL outputs are
    accepted."""
    assert pkg("_native").lib().csa_rows_sort_tile() == R.MERGE_TILE
    a, b = R.merge_pairs(W)[name]
    for mults in (True, False):
        ta, tb = ((t[0], t[2] if mults else None) for t in (a, b))
        scales = (int(a[2].sum()), int(b[2].sum())) if mults else (len(a[0]), len(b[0]))
        for select in J.SELECTS:
            want = J.np_join(ta, tb, select, scales)
            _check(_join(ta, tb, W, select, scales), want, (name, W, mults, select))
        want = J.np_join(ta, tb, 7, scales)
        caps = dict(cap_a=len(a[0]) + 37, cap_b=len(b[0]) + R.MERGE_TILE + 1, poison=True)
        _check(_join(ta, tb, W, 7, scales, **caps), want, (name, W, mults, "poison"))
    for outputs in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        _check(_join(ta, tb, W, 3, scales, outputs=outputs), J.np_join(ta, tb, 3, scales), (name, W, outputs))


def test_join_capacity(gpu_available):
    """cap_out equal to the selected count: a clean status; one below: CSA_E_UNSUPPORTED, the true count
    reported, nothing past cap_out rows written (the guards inside _join)."""
    N = pkg("_native")
    a, b = R.merge_pairs(2)["overlap"]
    ta, tb = (a[0], a[2]), (b[0], b[2])
    for select in (7, 4, 1):
        want = J.np_join(ta, tb, select)
        u = want[3]
        assert u > 1
        got = _join(ta, tb, 2, select, cap_out=u)
        _check(got, want, select)
        got = _join(ta, tb, 2, select, cap_out=u - 1)
        assert got[5][0] == N.CSA_E_UNSUPPORTED and got[3] == u and got[4] == want[4]
        assert np.array_equal(got[0], want[0][:u - 1]) and np.array_equal(got[1], want[1][:u - 1])
        assert np.array_equal(got[2], want[2][:u - 1])


def test_join_forged_lengths_are_clamped(gpu_available):
    a, b = R.merge_pairs(2)["overlap"]
    ta, tb = (a[0], a[2]), (b[0], b[2])
    want = J.np_join(ta, tb, 7)
    for lengths in ((1 << 63, len(b[0])), (len(a[0]), len(b[0]) + 1), ((1 << 64) - 1, 1 << 40)):
        _check(_join(ta, tb, 2, 7, lengths=lengths), want, lengths)


def test_join_record_overflow_word(gpu_available):
    """Mults of 2^32 - 1 on 5 shared rows with scales 2^32 - 1: word 9 is 5 (2^32 - 1)^2 >= 2^64 (it fits only
    below 2 shared rows), so word 10 is 1 and the status is raised.  With scales 1 word 9 is the exact
    5 (2^32 - 1), but word 8, the sum of mult_a * mult_b, is 5 (2^32 - 1)^2 whatever the scales, so for these very
    tables word 10 stays 1: integer arithmetic leaves no other answer.  Exact sums with word 10 = 0 are shown on
    tables whose products fit: mults 2^29 beside 2^32 - 1, and mults 2^30 on both sides, where word 8 fits at any
    scale and word 9 fits at scales 1 but not at scales 2^32 - 1."""
    N = pkg("_native")
    rows = R.ascending(5, 2)
    s = 2 ** 32 - 1
    big, eighth, quarter = (np.full(5, m, np.int64) for m in (s, 2 ** 29, 2 ** 30))
    t = (rows, big)
    assert 5 * s * s >= 2 ** 64 > s * s
    want = J.np_join(t, t, 4, (s, s))
    got = _join(t, t, 2, 4, (s, s))
    assert want[4][10] == 1 and got[4] == want[4] and got[5][0] == N.CSA_E_UNSUPPORTED
    assert np.array_equal(got[0], rows) and got[1].tolist() == got[2].tolist() == [s] * 5
    want = J.np_join(t, t, 4, (1, 1))
    got = _join(t, t, 2, 4, (1, 1))
    assert want[4][8:] == [5 * s * s % 2 ** 64, 5 * s, 1] and got[4] == want[4] and got[5][0] == N.CSA_E_UNSUPPORTED
    want = J.np_join((rows, eighth), t, 4, (1, 1))                 # 5 * 2^29 (2^32 - 1) < 2^64, beyond any 64-bit float's integers
    assert want[4][8:] == [5 * 2 ** 29 * s, 5 * 2 ** 29, 0] and 5 * 2 ** 29 * s < 2 ** 64
    _check(_join((rows, eighth), t, 2, 4, (1, 1)), want, "exact")
    q = (rows, quarter)
    want = J.np_join(q, q, 4, (1, 1))
    assert want[4][8:] == [5 * 2 ** 60, 5 * 2 ** 30, 0]
    _check(_join(q, q, 2, 4, (1, 1)), want, "exact at scales 1")
    want = J.np_join(q, q, 4, (s, s))
    got = _join(q, q, 2, 4, (s, s))
    assert want[4][8:] == [5 * 2 ** 60, 5 * 2 ** 30 * s % 2 ** 64, 1] and got[4] == want[4]
    assert got[5][0] == N.CSA_E_UNSUPPORTED


def _find(table, queries, cap=None, length=None):
    import torch
    N = pkg("_native")
    n, W = table.shape
    cap = n if cap is None else cap
    full = np.full((cap, W), 0xFFFFFFFFFFFFFFFF, np.uint64)      # rows past the table: above it, ascending
    full[:n] = table
    full[n:, W - 1] = 0xFFFFFFFFFFFFFF00 + np.arange(cap - n, dtype=np.uint64)
    d_t = _dev64(full, GUARD) if cap else None
    d_q = _dev64(queries, GUARD) if len(queries) else None
    d_len = _dev64(np.array([n if length is None else length], np.uint64))
    out = torch.full((len(queries) + GUARD,), GUARD32, dtype=torch.int32, device="cuda")
    N.check(N.lib().csa_rows_find_async(N.ptr(d_t), N.ptr(d_len), cap, W, N.ptr(d_q), len(queries),
                                        N.ptr(out) if len(queries) else None, None))
    torch.cuda.synchronize()
    assert _guards_ok(out, len(queries), GUARD32)
    return _u32(out, len(queries))


@pytest.mark.parametrize("W", [1, 27])
def test_find(gpu_available, W):
    table = J.find_table(W)
    assert len(table) == 2 * R.MERGE_TILE + 77
    batches, want = J.query_batches(table)
    for name, q in batches.items():
        assert np.array_equal(_find(table, q), want[name]), name
    q = batches["ends"]
    assert np.array_equal(_find(table, q, length=100), J.np_find(table[:100], q))          # the length bounds it
    assert np.array_equal(_find(table, q, cap=len(table) + 5, length=1 << 63), want["ends"])   # clamped to cap
    assert np.array_equal(_find(table, q, cap=len(table) + 5), want["ends"])                # rows past the length unread
    assert _find(table[:0], batches["present"]).tolist() == [J.MISSING] * 300               # an empty table


# --- the product paths --------------------------------------------------------------------------------------

class Spy:
    """Counts csa_rows_join_async / csa_rows_find_async calls and records what Tensor.cpu() copies."""

    def __init__(self, monkeypatch):
        import torch
        L = pkg("_native").lib()
        self.joins, self.finds, self.copied = [], [], []
        real_join, real_find, real_cpu = L.csa_rows_join_async, L.csa_rows_find_async, torch.Tensor.cpu

        def join(*a):
            self.joins.append(int(a[9]))         # select
            return real_join(*a)

        def find(*a):
            self.finds.append(int(a[5]))         # n_queries
            return real_find(*a)

        def cpu(t, *a, **kw):
            self.copied.append((t.data_ptr(), t.numel()))
            return real_cpu(t, *a, **kw)

        monkeypatch.setattr(L, "csa_rows_join_async", join)
        monkeypatch.setattr(L, "csa_rows_find_async", find)
        monkeypatch.setattr(torch.Tensor, "cpu", cpu)


OPERATORS = [(operator.and_, 4), (operator.or_, 7), (operator.sub, 1), (operator.xor, 3)]
COMPARISONS = [operator.le, operator.lt, operator.ge, operator.gt]


def _ids(inst):
    A = pkg("analysis")
    return list(A.encode_cached(inst.categories, inst.agents).agent_ids)


def test_panelset_algebra_on_the_device(gpu_available, monkeypatch):
    """found_panels of two seeds: every operator and comparison is Python's on the decoded sets, through one
    csa_rows_join_async each, the result's rows on the device; the S x W panel tensors never reach the host."""
    import torch
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    inst = pkg().read_instance(*inst_paths(J.COUPLES), 2)
    ids = _ids(inst)
    found = [A.legacy_probabilities(inst, 300, seed)[1] for seed in (0, 1)]
    kept = [f._packed for f in found]
    assert all(isinstance(p, torch.Tensor) and p.is_cuda for p in kept)
    sa, sb = (J.tuples(np.unique(oracle_panels(J.COUPLES, 2, seed, 300), axis=0), ids) for seed in (0, 1))
    assert sa - sb and sb - sa and sa & sb
    a, b = found
    spy = Spy(monkeypatch)
    for op, select in OPERATORS:
        n, n_copied = len(spy.joins), len(spy.copied)
        got = op(a, b)
        assert spy.joins[n:] == [select]
        assert isinstance(got, A.PanelSet) and got._are_distinct and got.device_rows() is got._dev_rows
        assert got._dev_rows.is_cuda and tuple(got._dev_rows.shape) == (len(op(sa, sb)), 1)
        assert [c for _, c in spy.copied[n_copied:]] == [14]     # status, length and record: no rows yet
        assert len(got) == len(op(sa, sb)) and J.tuples(got.rows(), ids) == op(sa, sb) and got == op(sa, sb)
        assert op(a, a) == op(sa, sa) and op(got, b) == op(op(sa, sb), sb)        # a result is an operand
    for op in COMPARISONS:
        n = len(spy.joins)
        assert op(a, b) is op(sa, sb) and op(a & b, a) is op(sa & sb, sa) and op(a, a) is op(sa, sa)
        assert op(a | b, b) is op(sa | sb, sb)
        assert spy.joins[n:] == [0, 4, 0, 0, 7, 0]               # the comparisons read the record only
    assert a.isdisjoint(b - a) and not a.isdisjoint(b) and (a & b).issubset(b) and (a | b).issuperset(a)
    for p in kept:
        assert p.data_ptr() not in [q for q, _ in spy.copied]
    # a plain set goes through the host mirror, reflected forms included
    n = len(spy.joins)
    assert (a & sb) == (sa & sb) and (sa - b) == (sa - sb) and (sb | a) == (sa | sb) and (a ^ sb) == (sa ^ sb)
    assert (sa <= a) and not (a < sa) and len(spy.joins) == n
    # contains_many
    probe = sorted(sa)[:7] + sorted(sb - sa)[:4] + sorted(sa)[:2]
    assert a.contains_many(probe).tolist() == [p in sa for p in probe] and spy.finds == [len(probe)]
    # CSA_ROWS_HOST=1: the host mirror, the same sets
    monkeypatch.setenv("CSA_ROWS_HOST", "1")
    n = len(spy.joins)
    assert (a & b) == (sa & sb) and (a - b) == (sa - sb) and len(spy.joins) == n


@pytest.mark.parametrize("name,k", [("sf_e_tight_110", 110), ("example_small_20", 20)])
def test_panelset_prefix_runs(gpu_available, monkeypatch, name, k):
    """One seed at S = 3001 against S = 2000: the shorter run is a prefix of the longer, so b <= a and a - b has
    the oracle's count; rows of W = 27 and W = 4 words through three sort tiles."""
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    inst = pkg().read_instance(*inst_paths(name), k)
    ids = _ids(inst)
    long_, short = oracle_panels(name, k, 5, 3001), oracle_panels(name, k, 5, 2000)
    assert np.array_equal(long_[:2000], short)
    ua, ub = np.unique(long_, axis=0), np.unique(short, axis=0)
    sa, sb = J.tuples(ua, ids), J.tuples(ub, ids)
    a, b = (A.legacy_probabilities(inst, S, 5)[1] for S in (3001, 2000))
    spy = Spy(monkeypatch)
    assert b <= a and a >= b and (len(sa) == len(sb) or (b < a and not a <= b))
    diff = a - b
    assert len(diff) == len(sa) - len(sb) == len(sa - sb) and diff.device_rows().shape[1] == ua.shape[1]
    assert np.array_equal(diff.rows(), J.np_join((ua, None), (ub, None), 1)[0]) and diff == (sa - sb)
    assert (a & b) == sb and np.array_equal((a | b).rows(), ua) and len(b - a) == 0 and (a ^ b) == (sa - sb)
    assert len(spy.joins) >= 8


@pytest.mark.parametrize("name,k,S", [(J.COUPLES, 2, 300), ("sf_e_tight_110", 110, 2000)])
def test_legacy_panel_comparison(gpu_available, monkeypatch, name, k, S):
    """Every integer of the comparison is the Counter result over the C oracle's panels of both seeds; each run is
    bit-equal to legacy_panel_distribution alone; the tables were joined on the device."""
    A, St = pkg("analysis"), pkg("stats")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    inst = pkg().read_instance(*inst_paths(name), k)
    spy = Spy(monkeypatch)
    run_a, run_b, c = A.legacy_panel_comparison(inst, S)
    assert spy.joins == [0]
    pa, pb = oracle_panels(name, k, 0, S), oracle_panels(name, k, 1, S)
    want = J.check_comparison(c, pa, pb)
    assert want[1] > 0 if name == J.COUPLES else want[1] == 0
    for run, seed, panels in ((run_a, 0, pa), (run_b, 1, pb)):
        alone = A.legacy_panel_distribution(inst, S, seed)
        assert run[0] == alone[0] and run[1] == alone[1] and np.array_equal(run[2].upper(), alone[2].upper())
        assert [x.tolist() for x in run[3].multiplicities()] == [x.tolist() for x in alone[3].multiplicities()]
        t, table = run[3].table(), R.np_table(panels)
        assert t.rows.is_cuda and np.array_equal(t.rows.cpu().numpy().view(np.uint64), table[0])
        assert np.array_equal(_u32(t.mult, len(table[0])), table[2])
        assert np.array_equal(_u32(t.first, len(table[0])), table[1])
    # the host mirror over the same runs gives the same object, and count() through the lookup the same counts
    monkeypatch.setenv("CSA_ROWS_HOST", "1")
    again = St.compare_panel_distributions(A.legacy_panel_distribution(inst, S, 0)[3],
                                           A.legacy_panel_distribution(inst, S, 1)[3])
    assert again == c and spy.joins == [0]
    monkeypatch.delenv("CSA_ROWS_HOST")
    top = run_a[3].top(3)
    n = len(spy.finds)
    assert [run_a[3].count(p) for p, _ in top] == [m for _, m in top] and len(spy.finds) == n + 3
    assert run_a[3].count(top[0][0]) == A.legacy_panel_distribution(inst, S, 0)[3].count(top[0][0])


def test_legacy_portfolio_overlap(gpu_available, monkeypatch):
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    inst = pkg().read_instance(*inst_paths(J.COUPLES), 2)
    ids = _ids(inst)
    panels = oracle_panels(J.COUPLES, 2, 0, 300)
    rows, weights = J.portfolio_case(panels, len(ids), 2)
    want = J.overlap_loop(panels, rows, weights)
    portfolio = [frozenset(ids[q] for q in np.flatnonzero(np.unpackbits(r.view(np.uint8), bitorder="little")))
                 for r in rows]
    dist = A.legacy_panel_distribution(inst, 300, 0)[3]
    spy = Spy(monkeypatch)
    po = A.legacy_portfolio_overlap(inst, dist, portfolio, weights.tolist())
    assert spy.finds == [len(rows)] and dist.table().rows.is_cuda
    J.check_overlap(po, want)
    assert max(c for _, c in spy.copied) <= len(rows)            # P counts come back, nothing else
    with pytest.raises(KeyError):
        A.legacy_portfolio_overlap(inst, dist, [("nobody",)], [1.0])
