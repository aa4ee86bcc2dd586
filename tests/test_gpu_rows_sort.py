"""The sorted distinct-row table on the device: csa_rows_sort_unique_async and csa_rows_merge_unique_async
through the C ABI (rs_tile_sort_kernel, rs_merge_kernel, the flag / scan / position / gather passes), and the
product paths that read found_panels through them -- analysis.PanelSet over kept panels,
distributed.PanelRedraw's streaming form over device_redraw, stats.ShardedPanelDistribution.

Expected values come from numpy alone (rows_cases.np_table: np.unique(axis=0) with its index and counts) and,
for the product paths, from the C oracle's panels.  Every assertion is integer equality; every buffer the
calls write carries guard words behind it."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import rows_cases as R
from conftest import REPO, inst_paths, pkg
from multiplicity_cases import oracle_panels

pytestmark = pytest.mark.gpu

GUARD = 16
GUARD64 = -0x0123456789ABCDEF
GUARD32 = 0x5A5A5A5A
COUPLES = "couples_panel_from_twenty_people_no_constraints_2"


def _dev64(a, guard=0):
    """uint64 array -> int64 device tensor (flat), ``guard`` guard words behind it."""
    import torch
    flat = np.ascontiguousarray(a, np.uint64).view(np.int64).ravel()
    t = torch.full((len(flat) + guard,), GUARD64, dtype=torch.int64, device="cuda")
    t[:len(flat)] = torch.from_numpy(flat)
    return t


def _dev32(a, guard=0):
    import torch
    flat = np.asarray(a, np.int64).astype(np.uint32).view(np.int32)
    t = torch.full((len(flat) + guard,), GUARD32, dtype=torch.int32, device="cuda")
    t[:len(flat)] = torch.from_numpy(flat)
    return t


def _u32(t, n):
    return t[:n].cpu().numpy().view(np.uint32).astype(np.int64)


def _guards_ok(t, used, value):
    return bool((t[used:] == value).all().item())


def _sort(rows, index_base=0, lists=True):
    """One csa_rows_sort_unique_async call with fresh poisoned buffers; returns (rows, first, mult) of the
    list's own length, after checking the guards and the input."""
    import torch
    N = pkg("_native")
    L = N.lib()
    n, W = rows.shape
    d_in = _dev64(rows, GUARD)
    need = int(L.csa_rows_sort_scratch_bytes(n, W))
    scratch = torch.full(((need + 7) // 8 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    out = torch.full((n * W + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    first = torch.full((n + GUARD,), GUARD32, dtype=torch.int32, device="cuda") if lists else None
    mult = torch.full((n + GUARD,), GUARD32, dtype=torch.int32, device="cuda") if lists else None
    distinct = torch.full((1 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    N.check(L.csa_rows_sort_unique_async(N.ptr(d_in), n, W, index_base, N.ptr(scratch), need, N.ptr(out), N.ptr(first),
                                         N.ptr(mult), N.ptr(distinct), None, None))
    torch.cuda.synchronize()
    d = int(distinct[0].item())
    assert 0 <= d <= n
    assert _guards_ok(out, n * W, GUARD64) and _guards_ok(distinct, 1, GUARD64)
    assert _guards_ok(scratch, (need + 7) // 8, GUARD64)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint64)[:n * W].reshape(n, W), rows)      # input unchanged
    assert _guards_ok(d_in, n * W, GUARD64)
    got = out[:d * W].cpu().numpy().view(np.uint64).reshape(d, W)
    if not lists:
        return got, None, None
    assert _guards_ok(first, n, GUARD32) and _guards_ok(mult, n, GUARD32)
    return got, _u32(first, d), _u32(mult, d)


@pytest.mark.parametrize("W", R.WIDTHS)
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_sort_unique_families(gpu_available, family, W):
    """Every size of rows_cases.sizes(T) -- a partial tile, a run without partner, three merge levels -- of one
    content family at one row width: rows, first (index_base 0 and 2^32 - n) and mult bit-equal to numpy, the
    NULL-list form the same rows."""
    T = pkg("_native").lib().csa_rows_sort_tile()
    assert T == R.MERGE_TILE
    for n in R.sizes(T):
        rows = R.FAMILIES[family](n, W)
        n = len(rows)
        want = R.np_table(rows)
        for base in (0, (1 << 32) - n):
            got = _sort(rows, base)
            assert np.array_equal(got[0], want[0]), (family, W, n, base)
            assert np.array_equal(got[1], want[1] + base) and np.array_equal(got[2], want[2]), (family, W, n, base)
        assert np.array_equal(_sort(rows, 0, lists=False)[0], want[0]), (family, W, n)


def test_host_mirror_is_the_device_contract(gpu_available):
    S = pkg("stats")
    rows = R.dup_pool(3 * R.MERGE_TILE + 5, 2)
    got, want = _sort(rows, 1000), S.rows_sort_unique_host(rows, 1000)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def _merge(a, b, W, cap_a=None, cap_b=None, cap_out=None, poison=False):
    """One csa_rows_merge_unique_async call; capacities default to the lengths (>= 1).  With ``poison`` the
    entries past the lengths hold rows (half copies of valid rows, half fresh), firsts and mults."""
    import torch
    N = pkg("_native")
    L = N.lib()
    rng = np.random.default_rng(5)

    def side(t, cap):
        rows, first, mult = t
        n = len(rows)
        cap = max(n, 1) if cap is None else cap
        full = np.zeros((cap, W), np.uint64)
        full[:n] = rows
        f, m = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        f[:n], m[:n] = first, mult
        if poison and cap > n:
            extra = rng.integers(0, 1 << 64, size=(cap - n, W), dtype=np.uint64)
            if n:
                extra[::2] = rows[rng.integers(0, n, size=len(extra[::2]))]
            full[n:], f[n:], m[n:] = extra, 0, 0xFFFFFFF0
        return _dev64(full, GUARD), _dev32(f, GUARD), _dev32(m, GUARD), _dev64(np.array([n], np.uint64)), cap

    A, B = side(a, cap_a), side(b, cap_b)
    union = len(R.np_merge(a, b)[0])
    cap_out = max(union, 1) if cap_out is None else cap_out
    need = int(L.csa_rows_merge_scratch_bytes(A[4], B[4], W))
    scratch = torch.full(((need + 7) // 8 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    out = torch.full((cap_out * W + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    first = torch.full((cap_out + GUARD,), GUARD32, dtype=torch.int32, device="cuda")
    mult = torch.full((cap_out + GUARD,), GUARD32, dtype=torch.int32, device="cuda")
    length = torch.full((1 + GUARD,), GUARD64, dtype=torch.int64, device="cuda")
    status = torch.zeros(4 + GUARD, dtype=torch.int32, device="cuda")
    N.check(L.csa_rows_merge_unique_async(*(N.ptr(x) for x in A[:4]), A[4], *(N.ptr(x) for x in B[:4]), B[4], W,
                                          N.ptr(scratch), need, N.ptr(out), N.ptr(first), N.ptr(mult), cap_out,
                                          N.ptr(length), N.ptr(status), None))
    torch.cuda.synchronize()
    assert _guards_ok(out, cap_out * W, GUARD64) and _guards_ok(first, cap_out, GUARD32)
    assert _guards_ok(mult, cap_out, GUARD32) and _guards_ok(length, 1, GUARD64)
    assert _guards_ok(scratch, (need + 7) // 8, GUARD64) and _guards_ok(status, 4, 0)
    for side_ in (A, B):
        assert _guards_ok(side_[0], side_[4] * W, GUARD64) and _guards_ok(side_[1], side_[4], GUARD32)
    ln = int(length[0].item())
    d = min(ln, cap_out)
    return (out[:d * W].cpu().numpy().view(np.uint64).reshape(d, W), _u32(first, d), _u32(mult, d), ln,
            status[:4].cpu().numpy().astype(np.uint32))


@pytest.mark.parametrize("W", [1, 2, 27])
@pytest.mark.parametrize("name", R.MERGE_NAMES)
def test_merge_unique_shapes(gpu_available, name, W):
    """Empty sides, equal lists, interleaved and disjoint ones, A wholly below B: the union is numpy's, with the
    lower first and the summed mult; capacities beyond the lengths with poison behind them change nothing."""
    a, b = R.merge_pairs(W)[name]
    want = R.np_merge(a, b)
    for poison in (False, True):
        caps = dict(cap_a=len(a[0]) + 37, cap_b=len(b[0]) + R.MERGE_TILE + 1, poison=True) if poison else {}
        rows, first, mult, ln, st = _merge(a, b, W, **caps)
        assert st[0] == 0 and ln == len(want[0]), (name, W, poison)
        assert np.array_equal(rows, want[0]) and np.array_equal(first, want[1]) and np.array_equal(mult, want[2])


def test_merge_unique_capacity(gpu_available):
    """cap_out equal to the union: a clean status; one below: CSA_E_UNSUPPORTED, the union's size reported,
    nothing past cap_out rows written (the guards inside _merge)."""
    N = pkg("_native")
    a, b = R.merge_pairs(2)["overlap"]
    want = R.np_merge(a, b)
    u = len(want[0])
    rows, first, mult, ln, st = _merge(a, b, 2, cap_out=u)
    assert st[0] == 0 and ln == u and np.array_equal(rows, want[0])
    rows, first, mult, ln, st = _merge(a, b, 2, cap_out=u - 1)
    assert st[0] == N.CSA_E_UNSUPPORTED and ln == u
    assert np.array_equal(rows, want[0][:u - 1])


# --- the product paths --------------------------------------------------------------------------------------

class Spy:
    """Counts csa_rows_sort_unique_async calls, records what Tensor.cpu() copies, and forbids the host forms."""

    def __init__(self, monkeypatch):
        import torch
        L = pkg("_native").lib()
        D = pkg("distributed")
        self.sorts, self.copied = [], []
        real_sort, real_cpu = L.csa_rows_sort_unique_async, torch.Tensor.cpu

        def sort(*a):
            self.sorts.append((int(a[1]), int(a[2]), int(a[3])))      # n_rows, W, index_base
            return real_sort(*a)

        def cpu(t, *a, **kw):
            self.copied.append((t.data_ptr(), t.numel()))
            return real_cpu(t, *a, **kw)

        def host_form(self_):
            raise AssertionError("PanelRedraw.__call__: the S x W host array was asked for")

        monkeypatch.setattr(L, "csa_rows_sort_unique_async", sort)
        monkeypatch.setattr(torch.Tensor, "cpu", cpu)
        monkeypatch.setattr(D.PanelRedraw, "__call__", host_form)


def _tuples(rows, n):
    return sorted(tuple(int(q) for q in np.flatnonzero(np.unpackbits(r.view(np.uint8), bitorder="little")[:n]))
                  for r in rows)


def _load_found_in_cpu_child(path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = ("import pickle, sys; sys.path.insert(0, %r); f = pickle.load(open(%r, 'rb')); "
            "assert 'torch' not in sys.modules or not sys.modules['torch'].cuda.is_available(); "
            "print(repr(sorted(f))); print(len(f))" % (REPO, str(path)))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got, ln = out.stdout.strip().splitlines()
    return got, int(ln)


@pytest.mark.parametrize("name,k,S,seed", [(COUPLES, 2, 10 ** 4, 3), ("example_small_20", 20, 3000, 4),
                                           ("sf_e_110", 110, 20011, (1 << 40) + 12345),
                                           ("synthetic8192_200", 200, 3000, 6)])
def test_kept_panels_read_on_the_device(gpu_available, monkeypatch, tmp_path, name, k, S, seed):
    """found_panels of a one-GPU run: rows(), iteration, the pickle and device_rows() come from the sorted
    table -- the S x W panel tensor is never copied to the host."""
    import torch
    A = pkg("analysis")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    inst = pkg().read_instance(*inst_paths(name), k)
    alloc, found, hist = A.legacy_probabilities(inst, S, seed)
    kept = found._packed
    assert isinstance(kept, torch.Tensor) and kept.is_cuda
    W = (len(inst.agents) + 63) // 64
    spy = Spy(monkeypatch)
    want = np.unique(oracle_panels(name, k, seed & 0xFFFFFFFFFFFFFFFF, S), axis=0)
    again = pickle.loads(pickle.dumps(found))           # __getstate__ first: it must take the device path itself
    rows = found.rows()
    assert spy.sorts == [(S, W, 0)]                     # the device path ran, once
    assert np.array_equal(rows, want) and len(found) == len(want)
    assert kept.data_ptr() not in [p for p, _ in spy.copied] and max(c for _, c in spy.copied) <= len(want) * W
    dr = found.device_rows()
    assert dr.is_cuda and dr.dtype == torch.int64 and tuple(dr.shape) == (len(want), W)
    assert np.array_equal(dr.cpu().numpy().view(np.uint64), want)
    assert dr.untyped_storage().nbytes() == max(len(want), 1) * W * 8      # the D rows, not the sort's S-row output
    ids = list(A.encode_cached(inst.categories, inst.agents).agent_ids)
    tuples = sorted(tuple(ids[q] for q in t) for t in _tuples(want, len(ids)))
    assert sorted(found) == tuples and tuples[0] in found and found == again
    assert np.array_equal(again.rows(), want) and again.device_rows() is None
    with open(tmp_path / "found.pkl", "wb") as fh:
        pickle.dump(found, fh)
    got, ln = _load_found_in_cpu_child(tmp_path / "found.pkl")
    assert got == repr(tuples) and ln == len(want)
    # a forged count: the sorted length is a second exact count
    forged = A.PanelSet(len(want) + 1, kept, len(ids), ids)
    with pytest.raises(RuntimeError, match="%d distinct panels, the run counted %d" % (len(want), len(want) + 1)):
        forged.rows()
    # CSA_ROWS_HOST=1: the old path, the same rows
    monkeypatch.setenv("CSA_ROWS_HOST", "1")
    n_sorts = len(spy.sorts)
    assert np.array_equal(A.PanelSet(len(want), kept, len(ids), ids).rows(), want) and len(spy.sorts) == n_sorts


@pytest.mark.parametrize("name,k,S,seed", [(COUPLES, 2, 5000, 8), ("sf_e_tight_110", 110, 3001, 9)])
def test_streaming_redraw_on_the_device(gpu_available, monkeypatch, name, k, S, seed):
    """PanelRedraw(device_redraw(...), S, W, chunk=777).table: rows, first and mult of the whole job from
    per-chunk sort-uniques merged on the device; the draw statistics untouched; a forged count raises; a
    ShardedPanelDistribution bound to the re-draw answers as the host-list distribution does."""
    import torch
    A, D, ST = pkg("analysis"), pkg("distributed"), pkg("stats")
    monkeypatch.delenv("CSA_ROWS_HOST", raising=False)
    inst = pkg().read_instance(*inst_paths(name), k)
    enc = A.encode_cached(inst.categories, inst.agents)
    enc.check_quotas(k)
    opanels = oracle_panels(name, k, seed, S)
    want = R.np_table(opanels)
    hf, hm = ST.panel_multiplicities_host(opanels)
    W, d = enc.W, len(want[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    before = A.draw_stats(enc)
    spy = Spy(monkeypatch)
    rd = D.PanelRedraw(D.device_redraw(enc, k, seed, dev), S, W, chunk=777)
    assert rd.streams()
    rows, first, mult = rd.table(d, lists=True)
    assert spy.sorts == [(min(777, S - o), W, o) for o in range(0, S, 777)]
    assert max(c for _, c in spy.copied) <= max(d * W, 8)
    assert np.array_equal(rows, want[0]) and np.array_equal(first, want[1]) and np.array_equal(mult, want[2])
    order = np.argsort(first, kind="stable")
    assert np.array_equal(first[order], hf) and np.array_equal(mult[order], hm)
    assert A.draw_stats(enc) == before
    for forged in (d - 1, d + 1):
        with pytest.raises(RuntimeError, match="re-drawn"):
            rd.table(forged)
    found = A.PanelSet(d, None, enc.n, enc.agent_ids)
    found._redraw = rd
    assert np.array_equal(found.rows(), want[0]) and found.device_rows() is None
    # the sharded distribution: the same answers as the host-list one
    plain = ST.PanelDistribution(S, hf, hm, opanels, enc.n, enc.agent_ids)
    sharded = ST.ShardedPanelDistribution(S, d, plain.spectrum, plain.sum_squares, hf[:0], hm[:0], redraw=rd, n=enc.n,
                                          agent_ids=enc.agent_ids)
    n_sorts = len(spy.sorts)
    assert [a.tolist() for a in sharded.multiplicities()] == [a.tolist() for a in plain.multiplicities()]
    assert len(spy.sorts) > n_sorts
    assert sharded.top(5) == plain.top(5)
    probe = plain.top(1)[0][0]
    assert sharded.count(probe) == plain.count(probe) == plain.top(1)[0][1]
    # the size guard, before anything is drawn
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **kw: (1000, 1 << 30))
    n_sorts = len(spy.sorts)
    with pytest.raises(RuntimeError, match="%d bytes of device memory, 1000 are free" % ST.table_bytes(d, 777, W)):
        rd.table(d)
    assert len(spy.sorts) == n_sorts
