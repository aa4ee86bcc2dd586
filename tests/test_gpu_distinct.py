"""The distinct-panel kernels (unique_kernel, the five uq_* kernels, the exchange's rep list) against
counts known by construction, on forged hashes (tests/distinct_cases.py), through the C ABI.

What the draw oracles cannot reach: the multi-element scans of uq_scan_part_kernel / uq_scan_tot_kernel
(n > 1 048 576), the segmented filter of the partitioned pass (>= 65 536 entries), long and wrapping
probe chains, rows that differ only in their last word under one hash, a 100 %-full LDS table (with
honest slots, and with every entry starting at one slot: the 8192-probe insertion), and the overflow
status one distinct panel later.  Every assertion is integer equality with a constructed
value; tests/test_distinct_cases_host.py pins the constructions on the CPU.

Not reached here: the `!q.fits` branch of csa_exchange_pack_async / csa_exchange_keys_async
(unique_kernel with a rep list) needs more than 16.8 M entries, which no few-second test moves; and
csa_unique_keys_async re-draws its rows from an instance, so its hashes cannot be forged beyond what
test_gpu_parity.py::test_exchange_keys_exact_on_device does.
"""
import functools

import numpy as np
import pytest

import distinct_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

PANEL_BEGIN = 2 ** 40 + 7


@functools.lru_cache(maxsize=4)
def _case(name):
    return C.UNIQUE_CASES[name]()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel()).cuda()


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def _unique(h, p, seg=None):
    """csa_unique_async (seg=None) or csa_unique_segments_async (seg=(cap, counts)) over all of h / p
    with the table a caller brings (pow2 >= 2 n slots, as distributed.HashTable), d_unique and the
    status block zeroed.  Returns (count, status words)."""
    import torch
    N = pkg("_native")
    L = N.lib()
    n, W = p.shape
    slots = C.table_slots(n)
    dh, dp = _dev(h), _dev(p)
    table = torch.zeros(slots, dtype=torch.int64, device="cuda")
    uniq = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    if seg is None:
        N.check(L.csa_unique_async(N.ptr(dh), N.ptr(dp), n, W, N.ptr(table), slots, N.ptr(uniq), N.ptr(status), None))
    else:
        cap, counts = seg
        assert n == len(counts) * cap
        dc = _dev(counts)
        N.check(L.csa_unique_segments_async(N.ptr(dh), N.ptr(dp), len(counts), cap, N.ptr(dc), W, N.ptr(table),
                                            slots, N.ptr(uniq), N.ptr(status), None))
    torch.cuda.synchronize()
    return int(uniq.item()), status.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("name", list(C.UNIQUE_CASES))
def test_unique_count_is_the_constructed_one(gpu_available, monkeypatch, name):
    """csa_unique_async on every builder: the dispatcher's own choice (the partitioned pass from 65 536
    entries on) and the single global table (CSA_UNIQUE_PART=0) both give the constructed count with a
    clean status block.  8193 distinct panels in one partition are the exception: the partitioned pass
    must leave CSA_E_UNSUPPORTED in the status block (never a silently short count), the global table
    must count them."""
    N = pkg("_native")
    h, p, expected = _case(name)
    n = len(h)
    # the first call below really is the partitioned pass (and for 65 535 entries really is not)
    assert C.takes_partitioned(n, C.table_slots(n)) == (n >= C.PART_MIN)
    monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
    count, st = _unique(h, p)
    print("%s: n %d expected %d, dispatcher's path: count %d status %s" % (name, n, expected, count, st.tolist()))
    if name == "one_partition_over":
        assert st[0] == N.CSA_E_UNSUPPORTED
        with pytest.raises(N.CsaError, match="LDS table"):
            N.check(N.lib().csa_status_decode(N.ptr(st)))
    else:
        assert st[0] == 0
        assert count == expected
    monkeypatch.setenv("CSA_UNIQUE_PART", "0")
    count, st = _unique(h, p)
    print("%s: global table: count %d status %s" % (name, count, st.tolist()))
    assert st[0] == 0
    assert count == expected


@pytest.mark.parametrize("kind", ["honest", "collision_chains"])
def test_unique_segments_partitioned(gpu_available, monkeypatch, kind):
    """csa_unique_segments_async at 8 x 9973 = 79 784 entries (the partitioned pass, pbits 7) with
    ragged segment counts and every invalid slot poisoned: the distinct count of the valid entries only,
    on both paths."""
    h, p, counts, expected = C.segments(C.segment_source(kind))
    n = len(h)
    assert n >= C.PART_MIN and C.takes_partitioned(n, C.table_slots(n)) and C.plan(n)[0] == 7
    for mode in (None, "0"):
        if mode is None:
            monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
        else:
            monkeypatch.setenv("CSA_UNIQUE_PART", mode)
        count, st = _unique(h, p, seg=(C.SEG_CAP, counts))
        print("%s segments, CSA_UNIQUE_PART=%s: expected %d count %d status %s"
              % (kind, mode, expected, count, st.tolist()))
        assert st[0] == 0
        assert count == expected


def _owners(case, world):
    """The constructed triples by owner h1 % world: per owner a sorted uint64[m, 2 + W]."""
    key = np.concatenate([case.distinct_hashes, case.distinct_panels], axis=1)
    owner = case.distinct_hashes[:, 0] % np.uint64(world)
    return [_sorted_rows(key[owner == w]) for w in range(world)]


def _exchange(kind, h, p, world, cap, panel_begin=0):
    """csa_exchange_pack_async / csa_exchange_keys_async over all of h / p.  Returns (host segments
    uint64[world, cap, 2 + W] or keys uint64[world, cap, 3], send counts, status words)."""
    import torch
    N = pkg("_native")
    L = N.lib()
    n, W = p.shape
    dh, dp = _dev(h), _dev(p)
    sb = int(L.csa_exchange_scratch_bytes(n))
    scratch = torch.zeros((sb + 7) // 8, dtype=torch.int64, device="cuda")
    sc = torch.zeros(world, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    if kind == "pack":
        sh = torch.zeros(world * cap * 2, dtype=torch.int64, device="cuda")
        sp = torch.zeros(world * cap * W, dtype=torch.int64, device="cuda")
        N.check(L.csa_exchange_pack_async(N.ptr(dh), N.ptr(dp), n, W, world, cap, N.ptr(scratch), scratch.numel() * 8,
                                          N.ptr(sh), N.ptr(sp), N.ptr(sc), N.ptr(status), None))
        torch.cuda.synchronize()
        out = np.concatenate([sh.cpu().numpy().view(np.uint64).reshape(world, cap, 2),
                              sp.cpu().numpy().view(np.uint64).reshape(world, cap, W)], axis=2)
    else:
        sk = torch.zeros(world * cap * 3, dtype=torch.int64, device="cuda")
        N.check(L.csa_exchange_keys_async(N.ptr(dh), N.ptr(dp), n, W, panel_begin, world, cap, N.ptr(scratch),
                                          scratch.numel() * 8, N.ptr(sk), N.ptr(sc), N.ptr(status), None))
        torch.cuda.synchronize()
        out = sk.cpu().numpy().view(np.uint64).reshape(world, cap, 3)
    return out, sc.cpu().numpy(), status.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name", ["honest_large_1050001", "skewed_large"])
def test_exchange_pack_rep_list(gpu_available, name, world):
    """csa_exchange_pack_async over 2048 partitions (two elements per thread in both scans): every
    owner's segment holds exactly the constructed triples with h1 % world == owner, once each.  The
    capacity is the largest owner's constructed count, so every slot of that segment is used."""
    case = _case(name)
    h, p, expected = case
    want = _owners(case, world)
    cap = max(len(w) for w in want)
    seg, sc, st = _exchange("pack", h, p, world, cap)
    print("%s pack world %d: cap %d send_counts %s status %s" % (name, world, cap, sc.tolist(), st.tolist()))
    assert st[0] == 0
    assert sc.tolist() == [len(w) for w in want] and sum(sc.tolist()) == expected
    for w in range(world):
        assert np.array_equal(_sorted_rows(seg[w, : sc[w]]), want[w])


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name", ["honest_large_1050001", "skewed_large"])
def test_exchange_keys_rep_list(gpu_available, name, world):
    """csa_exchange_keys_async with a panel_begin beyond 2^40: every key carries the hash of the entry
    its global index names, and the indexed entries are exactly one per constructed triple of that
    owner."""
    case = _case(name)
    h, p, expected = case
    n = len(h)
    want = _owners(case, world)
    cap = max(len(w) for w in want)
    keys, sc, st = _exchange("keys", h, p, world, cap, PANEL_BEGIN)
    print("%s keys world %d: cap %d send_counts %s status %s" % (name, world, cap, sc.tolist(), st.tolist()))
    assert st[0] == 0
    assert sc.tolist() == [len(w) for w in want] and sum(sc.tolist()) == expected
    for w in range(world):
        k = keys[w, : sc[w]]
        assert (k[:, 2] >= np.uint64(PANEL_BEGIN)).all() and (k[:, 2] < np.uint64(PANEL_BEGIN + n)).all()
        idx = (k[:, 2] - np.uint64(PANEL_BEGIN)).astype(np.int64)
        assert np.array_equal(h[idx], k[:, :2])
        assert np.array_equal(_sorted_rows(np.concatenate([h[idx], p[idx]], axis=1)), want[w])


def test_exchange_pack_full_partition(gpu_available):
    """A 100 %-full LDS table lists all of its 8192 entries: one_partition_full through the pack with
    one owner."""
    case = _case("one_partition_full")
    h, p, expected = case
    assert expected == C.K_UQ_TABLE
    seg, sc, st = _exchange("pack", h, p, 1, expected)
    assert st[0] == 0
    assert sc.tolist() == [expected]
    assert np.array_equal(_sorted_rows(seg[0]), _owners(case, 1)[0])
