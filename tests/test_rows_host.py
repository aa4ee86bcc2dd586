"""The sorted distinct-row table without a GPU: the numpy mirrors of csa_rows_sort_unique_async and
csa_rows_merge_unique_async (stats.rows_sort_unique_host / rows_merge_unique_host) against numpy's own
np.unique and the reference's panel counts, the entry points' argument validation (refused on the host before
any device call), and distributed.PanelRedraw's streaming form over a draw of numpy chunks behind the device
interface (stats.HostRowTables).  Every assertion is integer equality."""
import ctypes

import numpy as np
import pytest

import rows_cases as R
from conftest import pkg
from multiplicity_cases import CASES, mult_golden, oracle_panels, pack

T_HOST = 64      # the mirrors know no tile: the families at sizes around a small stand-in


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
@pytest.mark.parametrize("W", [1, 2, 27])
def test_sort_mirror_equals_numpy(family, W):
    S = pkg("stats")
    for n in R.sizes(T_HOST):
        rows = R.FAMILIES[family](n, W)
        for base in (0, (1 << 32) - n):
            got = S.rows_sort_unique_host(rows, base)
            want = R.np_table(rows, base)
            assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want)), (family, W, n, base)
            assert got[0].shape == (len(want[0]), W) and int(got[2].sum()) == n


@pytest.mark.parametrize("W", [1, 2, 27])
def test_merge_mirror_equals_sort_of_the_concatenation(W):
    S = pkg("stats")
    for name, (a, b) in R.merge_pairs(W, M=T_HOST).items():
        got = S.rows_merge_unique_host(a, b)
        want = R.np_merge(a, b)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
    # two chunks of one batch merge to the batch's own table
    rows = R.dup_pool(5 * T_HOST + 3, W)
    cut = 2 * T_HOST + 1
    got = S.rows_merge_unique_host(S.rows_sort_unique_host(rows[:cut]), S.rows_sort_unique_host(rows[cut:], cut))
    assert all(np.array_equal(g, w) for g, w in zip(got, R.np_table(rows)))


@pytest.mark.parametrize("case", CASES)
def test_mirrors_against_the_reference_counts(case):
    """tests/golden/multiplicity_<case>.json holds the reference's distinct panels with first index and count."""
    S = pkg("stats")
    g = mult_golden(case)
    panels = oracle_panels(g["instance"], g["k"], g["seed"], g["S"])
    rows, first, mult = S.rows_sort_unique_host(panels)
    order = np.argsort(first, kind="stable")
    assert first[order].tolist() == g["first"] and mult[order].tolist() == g["count"]
    assert np.array_equal(rows[order], pack(g["panels"], g["n"]))
    cut = g["S"] // 3
    merged = S.rows_merge_unique_host(S.rows_sort_unique_host(panels[:cut]), S.rows_sort_unique_host(panels[cut:], cut))
    assert all(np.array_equal(a, b) for a, b in zip(merged, (rows, first, mult)))


def test_argument_validation_without_a_device():
    N = pkg("_native")
    L = N.lib()
    T = L.csa_rows_sort_tile()
    assert T > 0
    for W in (1, 27):
        s = [L.csa_rows_sort_scratch_bytes(n, W) for n in (0, 1, 2, T - 1, T, T + 1, 8 * T + 3, 1 << 20)]
        m = [L.csa_rows_merge_scratch_bytes(n, 100, W) for n in (0, 1, T, T + 1, 1 << 20)]
        m2 = [L.csa_rows_merge_scratch_bytes(100, n, W) for n in (0, 1, T, T + 1, 1 << 20)]
        assert s == sorted(s) and m == sorted(m) and m2 == sorted(m2) and s[0] > 0
    p = ctypes.c_void_p(0x1000)      # never dereferenced: every call below is refused before any device call
    q, r = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000)
    big = 1 << 40

    def sort(rows=p, n=10, W=2, base=0, scratch=q, sb=big, out=r, first=None, mult=None, distinct=p):
        return L.csa_rows_sort_unique_async(rows, n, W, base, scratch, sb, out, first, mult, distinct, None, None)

    assert sort(W=0) == N.CSA_E_INVALID
    assert sort(distinct=None) == N.CSA_E_INVALID
    assert sort(rows=None) == N.CSA_E_INVALID
    assert sort(scratch=None) == N.CSA_E_INVALID
    assert sort(out=None) == N.CSA_E_INVALID
    assert sort(sb=L.csa_rows_sort_scratch_bytes(10, 2) - 1) == N.CSA_E_INVALID
    assert sort(out=p) == N.CSA_E_INVALID                                     # the output aliases the input
    assert sort(out=ctypes.c_void_p(0x1000 + 8)) == N.CSA_E_INVALID           # ... or overlaps it
    assert sort(base=(1 << 32) - 9) == N.CSA_E_UNSUPPORTED                    # base + n = 2^32 + 1
    assert sort(n=(1 << 32) + 1, base=0) == N.CSA_E_UNSUPPORTED
    assert "rows sort" in N.last_error()

    la, lb, lo = (ctypes.c_void_p(0x400000 + 8 * i) for i in range(3))      # the three length words

    def merge(a=(p, p, p, la, 10), b=(q, q, q, lb, 10), W=2, scratch=r, sb=big, out=(ctypes.c_void_p(0x300000), p, p),
              cap_out=20, out_len=lo, status=p):
        return L.csa_rows_merge_unique_async(*a, *b, W, scratch, sb, *out, cap_out, out_len, status, None)

    assert merge(sb=L.csa_rows_merge_scratch_bytes(10, 10, 2), a=(p, p, p, la, 1 << 31),
                 b=(q, q, q, lb, 1 << 31)) == N.CSA_E_UNSUPPORTED      # refused for the capacities alone

    assert merge(W=0) == N.CSA_E_INVALID
    assert merge(a=(p, p, p, None, 10)) == N.CSA_E_INVALID
    assert merge(b=(q, q, q, None, 10)) == N.CSA_E_INVALID
    assert merge(out_len=None) == N.CSA_E_INVALID
    assert merge(status=None) == N.CSA_E_INVALID
    assert merge(out_len=lb) == N.CSA_E_INVALID                               # B's length would be overwritten
    assert merge(a=(None, p, p, la, 10)) == N.CSA_E_INVALID
    assert merge(b=(q, None, q, lb, 10)) == N.CSA_E_INVALID
    assert merge(b=(q, q, None, lb, 10)) == N.CSA_E_INVALID
    assert merge(scratch=None) == N.CSA_E_INVALID
    assert merge(sb=L.csa_rows_merge_scratch_bytes(10, 10, 2) - 1) == N.CSA_E_INVALID
    assert merge(out=(None, p, p)) == N.CSA_E_INVALID
    assert merge(out=(p, p, p)) == N.CSA_E_INVALID                            # the output aliases A
    assert merge(out=(ctypes.c_void_p(0x100000 + 16), p, p)) == N.CSA_E_INVALID   # ... overlaps B
    assert merge(a=(p, p, p, la, 1 << 31), b=(q, q, q, lb, 1 << 31)) == N.CSA_E_UNSUPPORTED
    assert "rows merge" in N.last_error()
    assert L.csa_version() == 1


class FakeDeviceDraw:
    """A draw with device_redraw's interface whose 'device' chunks are numpy arrays and whose table operations
    are the host mirrors."""

    def __init__(self, panels, free_bytes=1 << 62):
        self.panels, self.free, self.chunks, self.status = panels, free_bytes, [], None

    def __call__(self, begin, count):
        raise AssertionError("the host form was called where device chunks are on offer")

    def device_chunk(self, begin, count):
        self.chunks.append((begin, count))
        return self.panels[begin:begin + count].copy()

    def tables(self):
        return pkg("stats").HostRowTables(self.free)


@pytest.fixture(scope="module")
def job():
    g = mult_golden("couples_s0")
    return g, oracle_panels(g["instance"], g["k"], 11, 5000)


def test_streaming_form_over_host_chunks(job, monkeypatch):
    D, A, S = pkg("distributed"), pkg("analysis"), pkg("stats")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    g, panels = job
    want_rows, want_first, want_mult = R.np_table(panels)
    draw = FakeDeviceDraw(panels)
    rd = D.PanelRedraw(draw, 5000, panels.shape[1], chunk=777)
    assert rd.streams()
    rows, first, mult = rd.table(len(want_rows), lists=True)
    assert draw.chunks == [(o, min(777, 5000 - o)) for o in range(0, 5000, 777)] and draw.chunks[-1][1] == 338
    assert np.array_equal(rows, want_rows) and np.array_equal(first, want_first) and np.array_equal(mult, want_mult)
    rows2, f2, m2 = rd.table(len(want_rows))
    assert np.array_equal(rows2, want_rows) and f2 is None and m2 is None
    # through PanelSet: the rows, the decoded set and the pickle
    found = A.PanelSet(len(want_rows), None, g["n"], list(range(g["n"])))
    found._redraw = D.PanelRedraw(FakeDeviceDraw(panels), 5000, panels.shape[1], chunk=777)
    assert np.array_equal(found.rows(), want_rows)
    assert found.device_rows() is None
    assert sorted(found) == sorted(tuple(int(q) for q in np.flatnonzero(
        np.unpackbits(r.view(np.uint8), bitorder="little"))) for r in want_rows)
    # through ShardedPanelDistribution: the list ordered by first index
    hf, hm = S.panel_multiplicities_host(panels)
    dist = S.ShardedPanelDistribution(5000, len(hf), np.bincount(hm), int((hm * hm).sum()), hf[:0], hm[:0],
                                      redraw=D.PanelRedraw(FakeDeviceDraw(panels), 5000, panels.shape[1], chunk=777),
                                      n=g["n"], agent_ids=list(range(g["n"])))
    f, m = dist.multiplicities()
    assert np.array_equal(f, hf) and np.array_equal(m, hm)
    # CSA_ROWS_HOST=1 forces the host form
    monkeypatch.setenv("CSA_ROWS_HOST", "1")
    assert not rd.streams()


def test_streaming_form_forged_count_and_size_guard(job, monkeypatch):
    D, A = pkg("distributed"), pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    g, panels = job
    d = len(R.np_table(panels)[0])
    for forged in (d + 1, d - 1, 1):     # a longer count: another length; a shorter one: the table overflows
        with pytest.raises(RuntimeError, match="re-drawn"):
            D.PanelRedraw(FakeDeviceDraw(panels), 5000, panels.shape[1], chunk=777).table(forged)
    bad = A.PanelSet(d + 1, None, g["n"], list(range(g["n"])))
    bad._redraw = D.PanelRedraw(FakeDeviceDraw(panels), 5000, panels.shape[1], chunk=777)
    with pytest.raises(RuntimeError, match="re-drawn"):
        bad.rows()
    need = pkg("stats").table_bytes(d, 777, panels.shape[1])
    draw = FakeDeviceDraw(panels, free_bytes=need - 1)
    with pytest.raises(RuntimeError, match="%d bytes.*%d are free" % (need, need - 1)):
        D.PanelRedraw(draw, 5000, panels.shape[1], chunk=777).table(d)
    assert draw.chunks == []             # refused before anything was drawn
    D.PanelRedraw(FakeDeviceDraw(panels, free_bytes=need), 5000, panels.shape[1], chunk=777).table(d)


def test_failed_read_keeps_the_redraw(job, monkeypatch):
    """A read that raises -- the size guard, a forged count -- leaves the set able to read again: the re-draw is
    dropped only once it has delivered.  After the guard, a retry with enough memory or with CSA_ROWS_HOST=1
    returns the rows, and a pickle holds them."""
    import pickle
    D, A = pkg("distributed"), pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    g, panels = job
    want = R.np_table(panels)[0]

    class HostAndDeviceDraw(FakeDeviceDraw):
        def __call__(self, begin, count):
            return self.panels[begin:begin + count]

    for retry in ("memory", "host"):
        draw = HostAndDeviceDraw(panels, free_bytes=10)
        found = A.PanelSet(len(want), None, g["n"], list(range(g["n"])))
        found._redraw = D.PanelRedraw(draw, 5000, panels.shape[1], chunk=777)
        for _ in range(2):
            with pytest.raises(RuntimeError, match="10 are free"):
                found.rows()
        with pytest.raises(RuntimeError, match="10 are free"):
            pickle.dumps(found)
        if retry == "memory":
            draw.free = 1 << 40
        else:
            monkeypatch.setenv("CSA_ROWS_HOST", "1")
        assert np.array_equal(found.rows(), want) and found._redraw is None
        back = pickle.loads(pickle.dumps(found))
        assert np.array_equal(back.rows(), want) and sorted(back) == sorted(found)
        monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    # a forged count raises on every read, never "panels were not kept"
    bad = A.PanelSet(len(want) + 1, None, g["n"], list(range(g["n"])))
    bad._redraw = D.PanelRedraw(FakeDeviceDraw(panels), 5000, panels.shape[1], chunk=777)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="re-drawn"):
            bad.rows()
