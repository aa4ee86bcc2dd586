"""Group composition on the device: group_hist_kernel alone on synthetic panels, and the product path
(analysis.legacy_composition) on panels the C oracle draws -- every table exact against the host
implementation (stats.group_hist_host, itself checked against brute force in test_composition_host)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLD, inst_paths, pkg
from oracle import coracle
from oracle.legacy_oracle import read_instance as oracle_read

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLD, "sf_e_110_intersections.csv")
GUARD = 2          # guard rows of `bins` entries before and after the table, in the same allocation
GUARD_VALUE = -0x0123456789ABCDEF


def _bits(members, W):
    x = np.zeros(W * 64, np.bool_)
    x[np.asarray(members, np.int64)] = True
    return np.packbits(x, bitorder="little").view("<u8")


def _synthetic(W, G, S, bins, seed):
    """n = 64 W - 5 agents (padding bits in the last word), panels of k = bins - 1 members.  Groups: the
    full mask first (every panel lies wholly inside it: the top bin), then the empty mask, bit 0,
    bit n - 1, a single agent, then random sets of mixed density.  Panels: up to 509 random k-subsets,
    drawn again and again past that (duplicates); panel 0 is repeated at two more places and one panel
    is empty."""
    rs = np.random.RandomState(seed)
    n = 64 * W - 5
    k = bins - 1
    assert k <= n
    special = [list(range(n)), [], [0], [n - 1], [n // 2]]
    masks = np.zeros((G, W), np.uint64)
    for g in range(G):
        if g < len(special):
            masks[g] = _bits(special[g], W)
        else:
            masks[g] = _bits(np.flatnonzero(rs.uniform(size=n) < rs.choice([0.02, 0.3, 0.9])), W)
    panels = np.zeros((S, W), np.uint64)
    if k and S:
        B = min(S, 509)
        idx = np.argpartition(rs.uniform(size=(B, n)), k - 1, axis=1)[:, :k]   # k smallest keys: a uniform k-subset
        x = np.zeros((B, W * 64), np.bool_)
        x[np.arange(B)[:, None], idx] = True
        base = np.packbits(x, axis=1, bitorder="little").view("<u8").reshape(B, W)
        panels[:B] = base
        panels[B:] = base[rs.randint(0, B, size=S - B)]
    if S > 3:
        panels[S // 2] = panels[0]
        panels[S - 1] = panels[0]
        panels[1] = 0
    return masks, panels


def _launch(panels, masks, bins, init=None, calls=1):
    """csa_group_hist_async over host arrays; returns (table int64[G, bins], status uint32[4], guards ok)."""
    import torch
    N = pkg("_native")
    S, W = panels.shape
    G = masks.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.full(((G + 2 * GUARD) * bins,), GUARD_VALUE, dtype=torch.int64, device=dev)
    body = buf[GUARD * bins:(G + GUARD) * bins]
    if init is None:
        body.zero_()
    else:
        body.copy_(torch.from_numpy(np.ascontiguousarray(init, np.int64).reshape(-1)))
    d_panels = torch.from_numpy(np.ascontiguousarray(panels).view(np.int64).reshape(-1)).to(dev) if S else \
        torch.zeros(1, dtype=torch.int64, device=dev)
    d_masks = torch.from_numpy(np.ascontiguousarray(masks).view(np.int64).reshape(-1)).to(dev) if G else \
        torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    for _ in range(calls):
        N.check(N.lib().csa_group_hist_async(N.ptr(d_panels), S, W, N.ptr(d_masks), G, bins,
                                             ctypes.c_void_p(body.data_ptr()), N.ptr(status),
                                             ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    h = buf.cpu().numpy()
    guards_ok = bool(np.all(h[:GUARD * bins] == GUARD_VALUE) and np.all(h[(G + GUARD) * bins:] == GUARD_VALUE))
    return h[GUARD * bins:(G + GUARD) * bins].reshape(G, bins).copy(), status.cpu().numpy().view(np.uint32), guards_ok


# (W, G, S, bins): every W in {1, 2, 27, 32, 33, 128}, G in {0, 1, 63, 64, 65, 130}, S in {0, 1, 63, 64, 65,
# 1000, 70001} and bins in {1, 3, 111, 201} at least once; then the paths the code takes beyond them:
# 32 and 16 groups per slab (W = 256, 300) and the table-less form (bins too many for LDS)
KERNEL_CASES = [
    (1, 1, 1, 3),
    (2, 63, 63, 111),
    (27, 64, 64, 111),
    (32, 65, 65, 201),
    (33, 130, 70001, 201),
    (128, 130, 1000, 201),
    (1, 64, 70001, 1),
    (27, 0, 1000, 3),
    (2, 65, 0, 3),
    (256, 40, 600, 201),
    (300, 20, 65, 3),
    (2, 6, 1000, 5000),
    (128, 65, 300, 400),
]


@pytest.mark.parametrize("W,G,S,bins", KERNEL_CASES)
def test_group_hist_kernel_exact(gpu_available, W, G, S, bins):
    St = pkg("stats")
    # k = bins - 1 members; 5000 bins (no LDS table at all) and 400 bins at W = 128 (masks + table past the
    # LDS with 64 groups) take panels of 100 and 200 members
    k = {5000: 100, 400: 200}.get(bins, bins - 1)
    masks, panels = _synthetic(W, G, S, k + 1, 1000 * W + G)
    want = St.group_hist_host(masks, panels, bins)
    got, status, guards_ok = _launch(panels, masks, bins)
    assert status.tolist() == [0, 0, 0, 0]
    assert guards_ok
    assert np.array_equal(got, want)
    if G and S:
        assert np.array_equal(got.sum(axis=1), np.full(G, S))
        # the full mask: every panel lies wholly inside it (bin k), but for the empty one
        assert got[0, k] == S - (1 if S > 3 and k else 0)


def test_group_hist_accumulates(gpu_available):
    """Two calls into one table add up, on top of what the table held; entries no panel lands in keep
    their pattern."""
    St = pkg("stats")
    W, G, S, bins = 27, 70, 3000, 111
    masks, panels = _synthetic(W, G, S, bins, 5)
    once = St.group_hist_host(masks, panels, bins)
    pattern = (np.arange(G * bins, dtype=np.int64).reshape(G, bins) * 7919) % 1000003 + (1 << 40)
    got, status, guards_ok = _launch(panels, masks, bins, init=pattern, calls=2)
    assert status[0] == 0 and guards_ok
    assert np.array_equal(got, pattern + 2 * once)
    assert np.array_equal(got[once == 0], pattern[once == 0]) and (once == 0).sum() > G * bins // 2
    # two different batches
    a, sa, _ = _launch(panels[:1234], masks, bins)
    b, sb, _ = _launch(panels[1234:], masks, bins, init=a)
    assert sa[0] == 0 and sb[0] == 0 and np.array_equal(b, once)


@pytest.mark.parametrize("W,bins,S", [(2, 4, 500), (27, 111, 70001)])
def test_group_hist_count_past_bins(gpu_available, W, bins, S):
    """One panel holds `bins` members of one group: that entry is not counted, the status block decodes
    to CSA_E_INVALID with the panel's index, every other entry is exact and nothing outside the table
    is written."""
    St, N = pkg("stats"), pkg("_native")
    G = 66
    masks, panels = _synthetic(W, G, S, bins, 77)
    n = 64 * W - 5
    bad_panel, bad_group = S - 7, 65
    # the last group: agents 0 .. bins - 1 and no more; the bad panel: exactly those agents
    masks[bad_group] = _bits(list(range(bins)), W)
    panels[bad_panel] = masks[bad_group]
    masks[0] = _bits(list(range(bins, n)), W)     # (the full mask would also see `bins` members,
    masks[5:bad_group] &= ~_bits([0], W)          # and so might a dense random group)
    keep = np.ones(S, bool)
    keep[bad_panel] = False
    want = St.group_hist_host(masks, panels[keep], bins)
    others = np.arange(G) != bad_group
    want[others] += St.group_hist_host(masks[others], panels[bad_panel:bad_panel + 1], bins)
    with pytest.raises(N.CsaError):
        St.group_hist_host(masks, panels, bins)             # the host implementation refuses it too
    got, status, guards_ok = _launch(panels, masks, bins)
    assert guards_ok
    assert status[0] == N.CSA_E_INVALID
    assert int(status[1]) | (int(status[2]) << 32) == bad_panel
    assert N.lib().csa_status_decode(N.ptr(np.ascontiguousarray(status))) == N.CSA_E_INVALID
    assert np.array_equal(got, want)
    assert got[bad_group].sum() == S - 1


# ---- the product path ------------------------------------------------------------------------------

def _instance(name, k):
    cat, resp = inst_paths(name)
    return pkg().read_instance(cat, resp, k), oracle_read(cat, resp, k)


def _oracle_table(oinst, k, seed, S, groups):
    rc, panels, _, _ = coracle.draw(oinst, k, seed & 0xFFFFFFFFFFFFFFFF, 0, S)
    assert rc == 0
    return panels, pkg("stats").group_hist_host(groups.masks, panels, k + 1)


def _check_composition(comp, want, groups, S, k, panels, n):
    assert comp.labels == groups.labels and comp.S == S and comp.k == k
    assert comp.counts.dtype == np.int64 and np.array_equal(comp.counts, want)
    assert np.array_equal(comp.counts.sum(axis=1), np.full(len(groups), S))
    # sum_c c * hist[g][c] = the per-person counts summed over the group's members, as integers
    person = coracle.counts(panels, n)
    member = np.unpackbits(groups.masks.view(np.uint8).reshape(len(groups), -1), axis=1, bitorder="little")[:, :n]
    assert np.array_equal((comp.counts * np.arange(k + 1, dtype=np.int64)).sum(axis=1),
                          member.astype(np.int64) @ person)


def test_legacy_composition_sf_e(gpu_available):
    A, St = pkg("analysis"), pkg("stats")
    inst, oinst = _instance("sf_e_110", 110)
    S, seed, k = 20011, 2 ** 40 + 12345, 110
    features = St.feature_groups(inst)
    groups = features + St.intersection_groups(inst, FIXTURE)
    assert len(groups) == 377
    panels, want = _oracle_table(oinst, k, seed, S, groups)
    alloc, found, hist, comp = A.legacy_composition(inst, S, seed, groups)
    _check_composition(comp, want, groups, S, k, panels, oinst.n)
    # every feature's support lies inside its quota
    lo, hi = comp.support()
    for g, (cat, feat) in enumerate(features.labels):
        q = inst.categories[cat][feat]
        assert q["min"] <= lo[g] <= hi[g] <= q["max"], (cat, feat)
    # the other three results are legacy_probabilities' own
    alloc2, found2, hist2 = A.legacy_probabilities(inst, S, seed)
    assert alloc == alloc2 and len(found) == len(found2) == coracle.unique(panels, oinst.n)
    assert np.array_equal(hist.upper(), hist2.upper())
    assert list(alloc.values()) == (coracle.counts(panels, oinst.n) / S).tolist()
    # and the standalone call over the panels the run kept gives the same table
    again = St.group_composition(groups, found._packed, k)
    assert np.array_equal(again.counts, want) and again.S == S


def test_legacy_composition_three_chunks(gpu_available):
    A, St = pkg("analysis"), pkg("stats")
    inst, oinst = _instance("sf_e_110", 110)
    S, seed, k = 5000, 77, 110
    groups = St.feature_groups(inst) + St.intersection_groups(inst, FIXTURE)
    _, want = _oracle_table(oinst, k, seed, S, groups)
    enc = A.encode_cached(inst.categories, inst.agents)
    one = A.legacy_sample_device(enc, k, S, seed, chunk=S, groups=groups)
    many = A.legacy_sample_device(enc, k, S, seed, chunk=2048, groups=groups)
    assert np.array_equal(one.composition, want) and np.array_equal(many.composition, want)
    assert np.array_equal(one.counts, many.counts) and one.unique == many.unique
    assert A.legacy_sample_device(enc, k, S, seed, chunk=2048).composition is None


@pytest.mark.parametrize("name,k,S", [("sf_e_tight_110", 110, 7001), ("example_large_200", 200, 3001),
                                      ("synthetic8192_200", 200, 600),
                                      ("couples_panel_from_twenty_people_no_constraints_2", 2, 10000)])
def test_legacy_composition_instances(gpu_available, name, k, S):
    """Restarts (sf_e_tight), the solo kernel at W = 32 and 201 bins, the wide kernel at W = 128, and
    W = 1 with 3 bins."""
    A, St = pkg("analysis"), pkg("stats")
    inst, oinst = _instance(name, k)
    ids = list(inst.agents)
    groups = St.feature_groups(inst) + St.agent_groups(inst, {"first": ids[:1], "last": ids[-1:], "all": ids,
                                                              "none": [], "odd": ids[1::2]})
    seed = 3
    panels, want = _oracle_table(oinst, k, seed, S, groups)
    alloc, found, hist, comp = A.legacy_composition(inst, S, seed, groups)
    _check_composition(comp, want, groups, S, k, panels, oinst.n)
    assert comp.counts[len(groups) - 3, k] == S                   # "all": every panel wholly inside
    alloc2, found2, hist2 = A.legacy_probabilities(inst, S, seed)
    assert alloc == alloc2 and len(found) == len(found2) and np.array_equal(hist.upper(), hist2.upper())


def test_legacy_composition_mt(gpu_available):
    import random
    A, St = pkg("analysis"), pkg("stats")
    inst, _ = _instance("example_small_20", 20)
    S, k = 10000, 20
    groups = St.feature_groups(inst)
    enc = A.encode_cached(inst.categories, inst.agents)
    random.seed(0)
    _, panels, _ = A.mt_draw(enc, k, S)
    want = St.group_hist_host(groups.masks, panels, k + 1)
    alloc, found, hist, comp = A.legacy_composition(inst, S, 0, groups, rng="mt")
    assert np.array_equal(comp.counts, want) and comp.S == S
    assert np.array_equal(comp.counts.sum(axis=1), np.full(len(groups), S))
    alloc2, found2, hist2 = A.legacy_probabilities(inst, S, 0, rng="mt")
    assert alloc == alloc2 and len(found) == len(found2) and np.array_equal(hist.upper(), hist2.upper())


def _rccl_world1():
    import socket
    import torch.distributed as dist
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)


def test_legacy_composition_sharded_rccl_world1(gpu_available, monkeypatch):
    """The sharded form over a one-rank RCCL group with the exchange forced on (its collectives run,
    the table's all_reduce among them): the table and the other three results equal the one-GPU
    call, also on a second call on the cached pipeline; the caller's device is unchanged."""
    import torch
    import torch.distributed as dist
    A, St, Dd = pkg("analysis"), pkg("stats"), pkg("distributed")
    inst, oinst = _instance("sf_e_110", 110)
    S, seed, k = 9001, 21, 110
    groups = St.feature_groups(inst) + St.intersection_groups(inst, FIXTURE)
    _, want = _oracle_table(oinst, k, seed, S, groups)
    alloc, found, hist, comp = A.legacy_composition(inst, S, seed, groups)
    assert np.array_equal(comp.counts, want)
    monkeypatch.setenv("CSA_FORCE_EXCHANGE", "1")
    monkeypatch.setenv("CSA_SHARD_CHUNK", "4000")
    dev0 = torch.cuda.current_device()
    _rccl_world1()
    try:
        for call in range(2):
            a2, f2, h2, c2 = Dd.legacy_probabilities_distributed(inst, S, seed, groups=groups)
            assert torch.cuda.current_device() == dev0
            assert np.array_equal(c2.counts, want) and c2.S == S and c2.k == k and c2.labels == groups.labels
            assert a2 == alloc and len(f2) == len(found) and np.array_equal(h2.upper(), hist.upper())
        assert len(Dd.legacy_probabilities_distributed(inst, S, seed)) == 3
    finally:
        dist.destroy_process_group()
