"""The forged inputs of tests/distinct_cases.py, pinned on the CPU: each builder's `expected` against
the host mirror of the exact rule (distributed.local_distinct), its partition occupancy, its slot
placement, and `plan(n)` against the figures the cases were sized for -- so the expectations of
tests/test_gpu_distinct.py do not rest on the device, and a later change to uq_plan that moves a case
off the path it targets fails here."""
import numpy as np
import pytest

import distinct_cases as C
from conftest import pkg

SMALL = ["one_partition_full", "one_partition_over", "collision_chains", "slot_pileup", "full_pileup",
         "threshold_65535", "threshold_65536", "threshold_65537"]


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def _check_case(case, n, W):
    D = pkg("distributed")
    h, p, expected = case
    assert h.dtype == np.uint64 and h.shape == (n, 2)
    assert p.dtype == np.uint64 and p.shape == (n, W)
    uh, up = D.local_distinct(h, p)
    assert len(uh) == expected
    # and they are exactly the constructed triples, each occurring at least once
    assert np.array_equal(np.concatenate([uh, up], axis=1),
                          _sorted_rows(np.concatenate([case.distinct_hashes, case.distinct_panels], axis=1)))
    return uh, up


def _occupancy(case, n):
    """Distinct triples per partition under plan(n)."""
    pbits, P, _, _ = C.plan(n)
    return np.bincount(C.part(case.distinct_hashes[:, 0], pbits).astype(np.int64), minlength=P)


@pytest.mark.parametrize("name", SMALL)
def test_expected_is_the_host_distinct_count(name):
    case = C.UNIQUE_CASES[name]()
    n = {"one_partition_full": 70000, "one_partition_over": 70001, "collision_chains": 66000,
         "slot_pileup": 66000, "full_pileup": 66000}.get(name) or int(name.split("_")[1])
    W = {"one_partition_full": 3, "one_partition_over": 3, "collision_chains": 3}.get(name, 2)
    _check_case(case, n, W)
    occ = _occupancy(case, n)
    if name == "one_partition_full":
        assert case[2] == 8192 and occ.max() == 8192 and np.count_nonzero(occ) == 1
    elif name == "one_partition_over":
        assert case[2] == 8193 and occ.max() == 8193 and np.count_nonzero(occ) == 1
    else:
        assert occ.max() <= C.K_UQ_TABLE and occ.sum() == case[2]


@pytest.mark.parametrize("builder", ["honest_large", "skewed_large"])
def test_large_generators_at_100000(builder):
    """The large builders' construction, checked on a 100 000-entry instance of the same generator."""
    case = getattr(C, builder)(100000)
    _check_case(case, 100000, 1)
    assert _occupancy(case, 100000).max() <= C.K_UQ_TABLE
    assert case[2] < 100000 // 3          # duplicate-heavy: about 3/4 of the entries are copies


def test_skewed_large_is_skewed():
    """skewed_large at its real size: five partitions of ~63 000 entries and <= ~4100 distinct triples,
    the first and the last partition among them, every partition within the LDS table."""
    n = 1050001
    h, p, expected = case = C.skewed_large(n)
    pbits, P, _, _ = C.plan(n)
    assert h.shape == (n, 2) and p.shape == (n, 1)
    entries = np.bincount(C.part(h[:, 0], pbits).astype(np.int64), minlength=P)
    occ = _occupancy(case, n)
    forced = [0, 1, P // 2 - 1, P // 2, P - 1]
    assert (entries[forced] >= 63000).all() and (entries[forced] < 64000).all()
    assert (occ[forced] >= 4000).all() and (occ[forced] <= 4200).all()
    rest = np.delete(entries, forced)
    assert rest.max() < 1000
    assert 0.29 * n < entries[forced].sum() < 0.31 * n
    assert occ.max() <= C.K_UQ_TABLE and occ.sum() == expected
    assert len(np.unique(p[:, 0])) == expected          # W = 1: a triple is its row


def test_one_partition_cases_share_their_first_8192_triples():
    full, over = C.one_partition_full(), C.one_partition_over()
    assert np.array_equal(full.distinct_hashes, over.distinct_hashes[:8192])
    assert np.array_equal(full.distinct_panels, over.distinct_panels[:8192])
    top = C.part(over.distinct_hashes[:, 0], 13)
    assert (top == C.ONE_PART_TOP13).all()
    # the low bits stay honest: the table fills from all over, not from one slot
    assert len(np.unique(C.lds_slot(full.distinct_hashes[:, 0], full.distinct_hashes[:, 1]))) > 4000


def test_collision_chains_shape():
    """2000 groups of 5 rows under one hash each, differing only in the last word, every triple at least
    twice."""
    h, p, expected = case = C.collision_chains()
    assert expected == 10000
    dh, dp = case.distinct_hashes, case.distinct_panels
    assert len(np.unique(dh, axis=0)) == 2000
    g = dp.reshape(2000, 5, 3)
    assert (g[:, :, :2] == g[:, :1, :2]).all()
    assert all(len(np.unique(g[:, :, 2][i])) == 5 for i in range(2000))
    assert np.array_equal(dh.reshape(2000, 5, 2)[:, 0], pkg("distributed").panel_hashes(g[:, 0]))
    _, counts = np.unique(np.concatenate([h, p], axis=1), axis=0, return_counts=True)
    assert counts.min() >= 2


def test_slot_pileup_lands_on_the_top_slots():
    n = 66000
    slots = C.table_slots(n)
    assert slots == 262144
    h, p, expected = case = C.slot_pileup()
    fh = case.distinct_hashes[:C.PILEUP]
    assert len(np.unique(fh, axis=0)) == C.PILEUP
    ls = C.lds_slot(fh[:, 0], fh[:, 1])
    gs = C.global_slot(fh[:, 0], fh[:, 1], slots)
    assert sorted(np.unique(ls).tolist()) == [8190, 8191]
    assert sorted(np.unique(gs).tolist()) == [slots - 2, slots - 1]
    pbits = C.plan(n)[0]
    assert len(np.unique(C.part(fh[:, 0], pbits))) == 1
    # each forged triple at least twice, so a duplicate has to walk the wrapped chain to its match
    key = np.concatenate([h, p], axis=1)
    forged = np.concatenate([fh, case.distinct_panels[:C.PILEUP]], axis=1)
    u, counts = np.unique(key, axis=0, return_counts=True)
    idx = {tuple(r): c for r, c in zip(u.tolist(), counts.tolist())}
    assert min(idx[tuple(r)] for r in forged.tolist()) >= 2


def test_full_pileup_fills_one_table_from_one_slot():
    """8192 triples of one partition, all starting at LDS slot 8191, each exactly twice, and nothing else
    in that partition: the last insertion needs all 8192 probes."""
    n = 66000
    h, p, expected = case = C.full_pileup()
    fh, fp = case.distinct_hashes[:C.K_UQ_TABLE], case.distinct_panels[:C.K_UQ_TABLE]
    assert len(np.unique(fh, axis=0)) == C.K_UQ_TABLE
    assert (C.lds_slot(fh[:, 0], fh[:, 1]) == 8191).all()
    occ = _occupancy(case, n)
    pbits = C.plan(n)[0]
    x = int(C.part(fh[0, 0], pbits))
    assert (C.part(fh[:, 0], pbits) == x).all() and occ[x] == C.K_UQ_TABLE
    assert np.delete(occ, x).max() < 1000
    in_x = C.part(h[:, 0], pbits) == x
    assert in_x.sum() == 2 * C.K_UQ_TABLE
    _, counts = np.unique(np.concatenate([h[in_x], p[in_x]], axis=1), axis=0, return_counts=True)
    assert (counts == 2).all() and len(counts) == C.K_UQ_TABLE
    # the global table sees them as chains too, but short ones
    gs = C.global_slot(fh[:, 0], fh[:, 1], C.table_slots(n))
    assert np.bincount((gs >> np.uint64(13)).astype(np.int64)).max() < 400


def test_copies_are_spread_over_chunks():
    """The fixed permutation: the copies of a triple land in different CH chunks (uq_count_kernel /
    uq_scatter_kernel workgroups), for nearly every duplicated triple."""
    h, p, expected = C.one_partition_full()
    CH = C.plan(len(h))[2]
    key = np.concatenate([h, p], axis=1)
    _, inv, counts = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.ravel()
    chunk = np.arange(len(h)) // CH
    first = np.full(expected, -1)
    first[inv[::-1]] = chunk[::-1]
    spread = np.zeros(expected, bool)
    np.logical_or.at(spread, inv, chunk != first[inv])
    assert spread[counts >= 4].mean() > 0.9


def test_plan_figures():
    """uq_plan's regimes at the sizes the cases use (and the README's 10^7 job)."""
    assert C.plan(400000) == (9, 512, 4096, 98) and C.scan_per(400000) == (1, 1)
    assert C.plan(1050001)[0] == 11 and C.plan(1050001)[3] == 257 and C.scan_per(1050001) == (2, 2)
    assert C.plan(4200001) == (13, 8192, 4352, 966) and C.scan_per(4200001) == (4, 8)
    assert C.plan(10 ** 7) == (13, C.K_UQ_MAX_PARTS, 9984, 1002) and C.scan_per(10 ** 7) == (4, 8)
    assert C.plan(65536)[0] == 6 and C.plan(65537)[0] == 7
    assert C.plan(sum(C.SEG_COUNTS))[0] == 6 and C.plan(8 * C.SEG_CAP)[0] == 7 and 8 * C.SEG_CAP == 79784
    for n in (1050001, 4200001):
        assert n % 2 == 1 and n % 256 and n % C.plan(n)[2]
    # which dispatcher branch each csa_unique_async case takes with the table a caller brings
    for n in (65536, 65537, 66000, 70000, 70001, 79784, 1050001, 4200001, 10 ** 7):
        assert C.takes_partitioned(n, C.table_slots(n)), n
    assert not C.takes_partitioned(65535, C.table_slots(65535))
    assert C.fits(16 * 1024 * 1024) and not C.fits(2049 * 8192)


@pytest.mark.parametrize("kind", ["honest", "collision_chains"])
def test_segments_layout(kind):
    """The segmented layout: the valid entries are the case's, their distinct count is `expected`, and
    the poison would change the count if it were read."""
    D = pkg("distributed")
    case = C.segment_source(kind)
    h, p, counts, expected = C.segments(case)
    S, cap = len(C.SEG_COUNTS), C.SEG_CAP
    W = p.shape[1]
    assert len(h) == S * cap == 79784 and counts.tolist() == list(C.SEG_COUNTS)
    assert C.takes_partitioned(S * cap, C.table_slots(S * cap))
    assert D.distinct_segments(h.reshape(S, cap, 2), p.reshape(S, cap, W), counts) == expected == case[2]
    slot = np.arange(S * cap)
    valid = (slot % cap) < counts.astype(np.int64)[slot // cap]
    assert np.array_equal(h[valid], case[0]) and np.array_equal(p[valid], case[1])
    n_bad = int((~valid).sum())
    # read in full, every fresh poison triple would count and every poison copy would not
    assert D.distinct_exact(h, p) == expected + n_bad // 2
