"""The exchange in which the panel multiplicities travel, host side: the numpy mirrors
``distributed.mult_key_buckets`` / ``merge_mult_keys`` over simulated worlds on the C oracle's panels
(against ``stats.panel_multiplicities_host`` of the whole run and the reference's own panel counts,
tests/golden/multiplicity_<case>.json), forged 128-bit collisions, an empty rank, a full segment,
``PanelExchange.run_multiplicity`` over gloo on host tensors, ``stats.ShardedPanelDistribution`` built from
host pieces with a draw function that records what it is asked for, and the argument checks of the two C
entry points that return before any device call.  No GPU."""
import ctypes
import os
import pickle
import socket

import numpy as np
import pytest

from conftest import REPO, pkg
from multiplicity_cases import CASES, expected_top, mult_golden, oracle_panels

COUPLES = ("couples_panel_from_twenty_people_no_constraints_2", 2, 5, 20000)      # 100 distinct panels
WORLDS = [1, 2, 3, 8]


def _run(name):
    """(panels, honest hashes) of a named run: "couples", or a golden of CASES."""
    if name == "couples":
        inst, k, seed, S = COUPLES
    else:
        g = mult_golden(name)
        inst, k, seed, S = g["instance"], g["k"], g["seed"], g["S"]
    panels = oracle_panels(inst, k, seed, S)
    return panels, pkg("distributed").panel_hashes(panels)


def _expected_pairs(h, p):
    """(first, mult) ascending in first under the project's rule, equal hash AND equal bitmask: np.unique
    over the (h1, h2, row) triples."""
    _, first, mult = np.unique(np.concatenate([h, p], axis=1), axis=0, return_index=True, return_counts=True)
    order = np.argsort(first)
    return first[order].astype(np.int64), mult[order].astype(np.int64)


def simulate(panels, hashes, world, cap=None):
    """Both mirrors over ``world`` contiguous shards: every sender's (keys, counts), every owner's list."""
    D = pkg("distributed")
    shards = [D.shard_range(len(panels), world, r) for r in range(world)]
    cap = cap or D.exchange_capacity(max(e - b for b, e in shards), world)
    sends = [D.mult_key_buckets(hashes[b:e], panels[b:e], b, world, cap) for b, e in shards]
    owners = []
    for r in range(world):
        keys = np.stack([k[r] for k, _ in sends])
        owners.append(D.merge_mult_keys(keys, [c[r] for _, c in sends], lambda idx: panels[idx]))
    return shards, sends, owners


def check_owners(owners, hashes, world, want_first, want_mult):
    firsts = np.concatenate([f for f, _ in owners])
    mults = np.concatenate([m for _, m in owners])
    assert len(set(firsts.tolist())) == len(firsts)                      # the owners' lists are disjoint
    order = np.argsort(firsts)
    assert np.array_equal(firsts[order], want_first) and np.array_equal(mults[order], want_mult)
    for r, (f, _) in enumerate(owners):                                  # every entry sits on h1 % world
        assert np.all(hashes[f, 0] % np.uint64(world) == np.uint64(r))
        assert f.dtype == np.int64 and np.all(np.diff(f) > 0)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["couples"] + CASES)
def test_mirrors_over_simulated_worlds(name, world):
    panels, hashes = _run(name)
    want_first, want_mult = pkg("stats").panel_multiplicities_host(panels)
    shards, sends, owners = simulate(panels, hashes, world)
    check_owners(owners, hashes, world, want_first, want_mult)
    if name == "couples":
        assert len(want_first) == 100
        for (b, e), (keys, sc) in zip(shards, sends):
            assert int(sc.sum()) == 100                                  # each of them on every rank
    else:
        g = mult_golden(name)
        assert want_first.tolist() == g["first"] and want_mult.tolist() == g["count"]
    for (b, e), (keys, sc) in zip(shards, sends):
        for w in range(world):
            seg = keys[w, : sc[w]]
            assert np.all(seg[:, 0] % np.uint64(world) == np.uint64(w))
            idx = seg[:, 2].astype(np.int64)
            assert np.all((idx >= b) & (idx < e)) and np.array_equal(hashes[idx], seg[:, :2])
            assert not keys[w, sc[w]:].any()
        assert int(sum(keys[w, : sc[w], 3].sum() for w in range(world))) == e - b


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("case", ["forged", "forged_dups"])
def test_forged_collisions(case, world):
    """A forged hash shared by two different panels gives two entries; every copy of panel x hashing like
    panel y gives separate, correctly summed entries for x and y."""
    if case == "forged":
        panels = oracle_panels("example_small_20", 20, 3, 5000)
        hashes = pkg("distributed").panel_hashes(panels)
        assert len(np.unique(panels, axis=0)) == 5000 and not np.array_equal(panels[0], panels[1000])
        hashes[1000] = hashes[0]
    else:
        panels, hashes = _run("couples")
        x = panels[0]
        y = next(r for r in panels if not np.array_equal(r, x))
        same_x = (panels == x).all(axis=1)
        hashes[same_x] = pkg("distributed").panel_hashes(y[None])[0]
        assert same_x.sum() > world
    want_first, want_mult = _expected_pairs(hashes, panels)
    host_first, host_mult = pkg("stats").panel_multiplicities_host(panels)
    assert np.array_equal(want_first, host_first) and np.array_equal(want_mult, host_mult)
    _, _, owners = simulate(panels, hashes, world)
    check_owners(owners, hashes, world, want_first, want_mult)
    if case == "forged":
        f, m = owners[int(hashes[0, 0] % np.uint64(world))]
        assert {0, 1000} <= set(f.tolist()) and m[f == 0].tolist() == [1] and m[f == 1000].tolist() == [1]


def test_a_world_with_an_empty_rank():
    panels, hashes = _run("couples")
    panels, hashes = panels[:2], hashes[:2]
    shards, sends, owners = simulate(panels, hashes, 3)
    assert shards[2] == (2, 2) and sends[2][1].tolist() == [0, 0, 0]
    check_owners(owners, hashes, 3, *pkg("stats").panel_multiplicities_host(panels))
    assert sum(len(f) for f, _ in owners) == len(np.unique(panels, axis=0))


def test_a_segment_past_its_capacity_raises():
    D = pkg("distributed")
    panels = oracle_panels("sf_e_110", 110, 0, 1000)
    hashes = D.panel_hashes(panels)
    with pytest.raises(RuntimeError, match="capacity"):
        D.mult_key_buckets(hashes, panels, 0, 2, 100)
    keys, sc = D.mult_key_buckets(hashes, panels, 0, 2, D.exchange_capacity(1000, 2))
    assert int(sc.sum()) == 1000


def test_mult_record_and_order_keys():
    D = pkg("distributed")
    rec = D.mult_record([1, 1, 2, 9, 3], 4)
    assert rec.tolist() == [5, 0, 2, 1, 1, 1, 9, 1 + 1 + 4 + 81 + 9, 16]
    assert D.mult_record([], 3).tolist() == [0, 0, 0, 0, 0, 0, 0, 0]


# ---- gloo on host tensors -------------------------------------------------------------------------
GLOO_RUN = ("couples_panel_from_twenty_people_no_constraints_2", 2, 7, 3000)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D = pkg("distributed")
        inst, k, seed, S = GLOO_RUN
        panels = oracle_panels(inst, k, seed, S)
        b, e = D.shard_range(S, world, rank)
        W = panels.shape[1]
        mine = np.ascontiguousarray(panels[b:e])
        h = torch.from_numpy(D.panel_hashes(mine).ravel().view(np.int64).copy()) if e > b else \
            torch.zeros(0, dtype=torch.int64)
        p = torch.from_numpy(mine.view(np.int64).ravel().copy())
        ex = D.PanelExchange(D.shard_range(S, world, 0)[1], W, world, "cpu")
        first, mult, rec = ex.run_multiplicity(h, p, e - b, panel_begin=b, n_bins=16,
                                               panels_of=lambda idx: panels[idx])
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), first=first.numpy(), mult=mult.numpy(), rec=rec.numpy())
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_run_multiplicity_equals_the_mirror(tmp_path, world):
    import torch.multiprocessing as mp
    D = pkg("distributed")
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    inst, k, seed, S = GLOO_RUN
    panels = oracle_panels(inst, k, seed, S)
    hashes = D.panel_hashes(panels)
    _, _, owners = simulate(panels, hashes, world)
    got = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    for r in range(world):
        assert np.array_equal(got[r]["first"], owners[r][0]) and np.array_equal(got[r]["mult"], owners[r][1])
        assert np.array_equal(got[r]["rec"], D.mult_record(owners[r][1], 16))
    check_owners([(g["first"], g["mult"]) for g in got], hashes, world, *pkg("stats").panel_multiplicities_host(panels))


# ---- the sharded PanelDistribution from host pieces -------------------------------------------------
TOP_KEEP = 8


def _sharded(case, world=3, forge=None, keep=True):
    """A ShardedPanelDistribution of rank 1 of ``world`` over a golden's run, the draw function recording
    every (begin, count) it serves."""
    D, ST = pkg("distributed"), pkg("stats")
    g = mult_golden(case)
    panels = oracle_panels(g["instance"], g["k"], g["seed"], g["S"])
    hashes = D.panel_hashes(panels)
    _, _, owners = simulate(panels, hashes, world)
    cf, cm = [], []
    for f, m in owners:                                # each owner's TOP_KEEP best entries
        best = np.lexsort((f, -m))[:TOP_KEEP]
        cf.append(f[best])
        cm.append(m[best])
    calls = []

    def draw(begin, count):
        calls.append((int(begin), int(count)))
        return panels[begin:begin + count]

    mult = np.array(g["count"])
    spectrum = np.bincount(mult) if forge is None else forge(np.bincount(mult))
    redraw = D.PanelRedraw(draw, g["S"], panels.shape[1], chunk=4096) if keep else None
    d = ST.ShardedPanelDistribution(g["S"], g["unique"], spectrum, int((mult * mult).sum()), owners[1][0],
                                    owners[1][1], (np.concatenate(cf), np.concatenate(cm)), TOP_KEEP, redraw,
                                    g["n"], list(range(g["n"])))
    return g, d, calls, owners


@pytest.mark.parametrize("case", CASES)
def test_sharded_distribution_top_from_the_candidates(case):
    g, d, calls, owners = _sharded(case)
    mult = np.array(g["count"])
    assert d.S == g["S"] and d.distinct == len(d) == g["unique"]
    assert d.spectrum.tolist() == np.bincount(mult).tolist() and d.max_multiplicity == int(mult.max())
    assert d.coverage() == 1 - int((mult == 1).sum()) / g["S"] and d.max_probability() == int(mult.max()) / g["S"]
    f, m = d.owned()
    assert np.array_equal(f, owners[1][0]) and np.array_equal(m, owners[1][1]) and calls == []
    assert d.top(5) == expected_top(g, 5)
    assert all(c == 1 for _, c in calls) and len(calls) <= TOP_KEEP      # single indices, never the range
    assert d.top(min(TOP_KEEP, g["unique"])) == expected_top(g, min(TOP_KEEP, g["unique"]))
    assert all(c == 1 for _, c in calls) and len(calls) <= TOP_KEEP
    assert d.top(0) == []


@pytest.mark.parametrize("case", CASES)
def test_sharded_distribution_materialises_once(case):
    g, d, calls, _ = _sharded(case)
    whole = [(off, min(4096, g["S"] - off)) for off in range(0, g["S"], 4096)]
    more = min(TOP_KEEP + 1, g["unique"])
    got = d.top(TOP_KEEP + 1)
    assert got == expected_top(g, more)
    ranges = lambda: [c for c in calls if c[1] != 1]                     # noqa: E731  (not top's single indices)
    if g["unique"] > TOP_KEEP:
        assert calls == whole                                            # the job [0, S), once
    else:
        assert ranges() == []                                            # a short list is all candidates
    assert d.count(g["panels"][0]) == g["count"][0] and d.count(g["panels"][-1]) == g["count"][-1]
    back = pickle.loads(pickle.dumps(d))
    assert ranges() == whole
    assert type(back) is pkg("stats").PanelDistribution
    assert [a.tolist() for a in d.multiplicities()] == [g["first"], g["count"]]
    assert [a.tolist() for a in back.multiplicities()] == [g["first"], g["count"]]
    assert back.top(5) == d.top(5) == expected_top(g, 5) and back.count(g["panels"][0]) == g["count"][0]
    assert back.spectrum.tolist() == d.spectrum.tolist() and back.sum_squares == d.sum_squares
    assert ranges() == whole


def test_sharded_distribution_forged_spectrum_raises():
    """A spectrum that passes the constructor's sums but is not the re-drawn panels'."""
    def forge(f):
        f = f.copy()
        occupied = np.flatnonzero(f)
        a, b = next((a, b) for a in occupied for b in occupied if b - a >= 2)
        f[a] -= 1
        f[b] -= 1
        f[a + 1] += 1
        f[b - 1] += 1
        return f

    g, d, calls, _ = _sharded("rejecty_6_s3", forge=forge)
    assert d.top(3) == expected_top(g, 3)                                # the candidates do not read it
    for call in (d.multiplicities, lambda: d.count(g["panels"][0]), lambda: pickle.dumps(d)):
        with pytest.raises(RuntimeError, match="spectrum"):
            call()
    with pytest.raises(ValueError):
        pkg("stats").ShardedPanelDistribution(g["S"], g["unique"] + 1, d.spectrum, d.sum_squares, [], [])


def test_sharded_distribution_without_panels():
    g, d, calls, _ = _sharded("couples_s0", keep=False)
    assert d.chao1() == g["unique"] + 0.0 and d.coverage() == 1.0 and len(d.owned()[0]) > 0
    for call in (lambda: d.top(1), lambda: d.count(g["panels"][0]), d.multiplicities, lambda: pickle.dumps(d)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == pkg("analysis").PanelSet._where


# ---- C ABI: what returns before any device call ---------------------------------------------------
def test_invalid_arguments_return_before_any_device_call():
    N = pkg("_native")
    L = N.lib()
    word = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(word, ctypes.c_void_p)
    bad = N.CSA_E_INVALID
    send = L.csa_exchange_mult_keys_async
    assert send(p, 5, p, p, p, 0, 0, 8, p, p, p, None) == bad                   # world == 0
    assert send(p, 5, p, p, p, 0, 1025, 8, p, p, p, None) == bad                # world > 1024
    assert send(p, 5, p, p, p, 0, 2, 0, p, p, p, None) == bad                   # capacity == 0
    assert send(None, 5, p, p, p, 0, 2, 8, p, p, p, None) == bad
    assert send(p, 5, None, p, p, 0, 2, 8, p, p, p, None) == bad
    assert send(p, 5, p, None, p, 0, 2, 8, p, p, p, None) == bad
    assert send(p, 5, p, p, None, 0, 2, 8, p, p, p, None) == bad
    assert send(p, 5, p, p, p, 0, 2, 8, None, p, p, None) == bad
    assert send(p, 5, p, p, p, 0, 2, 8, p, None, p, None) == bad
    assert send(p, 5, p, p, p, 0, 2, 8, p, p, None, None) == bad
    assert send(None, 0, None, None, None, 0, 2, 8, p, p, p, None) == bad       # d_distinct, even when empty
    assert send(p, 1 << 32, p, p, p, 0, 2, 8, p, p, p, None) == N.CSA_E_UNSUPPORTED
    assert send(p, 5, p, p, p, (1 << 32) - 4, 2, 8, p, p, p, None) == N.CSA_E_UNSUPPORTED
    merge = L.csa_merge_mult_keys_async
    big = int(L.csa_merge_mult_keys_scratch_bytes(16, 1))
    assert big >= 8 * (6 * 64 + 1 + 2 * 16 + 2 * 16 + 2 * 16)
    sizes = [int(L.csa_merge_mult_keys_scratch_bytes(n, 3)) for n in (0, 1, 31, 32, 33, 1000, 1 << 20, (1 << 20) + 1)]
    assert sizes == sorted(sizes)
    assert merge(None, 2, 0, 0, p, 2, 8, p, p, big, p, p, p, p, None) == bad    # no instance
    # (p stands for an instance: these return before it is read; the scratch check reads its W and so
    # needs a real one, which needs a device -- tests/test_gpu_multiplicity_exchange.py)
    assert merge(p, 2, 0, 0, None, 2, 8, p, p, big, p, p, p, p, None) == bad
    assert merge(p, 2, 0, 0, p, 2, 8, None, p, big, p, p, p, p, None) == bad
    assert merge(p, 2, 0, 0, p, 2, 8, p, None, big, p, p, p, p, None) == bad
    assert merge(p, 2, 0, 0, p, 2, 8, p, p, big, None, p, p, p, None) == bad
    assert merge(p, 2, 0, 0, p, 2, 8, p, p, big, p, None, p, p, None) == bad
    assert merge(p, 2, 0, 0, p, 2, 8, p, p, big, p, p, None, p, None) == bad
    assert merge(p, 2, 0, 0, p, 2, 8, p, p, big, p, p, p, None, None) == bad
    assert merge(p, 2, 0, 0, p, 0, 8, p, p, big, p, p, p, p, None) == bad       # n_segments == 0
    assert merge(p, 2, 0, 0, p, 2, 0, p, p, big, p, p, p, p, None) == bad       # capacity == 0
    assert merge(p, 2, 0, 0, p, 1 << 20, 1 << 20, p, p, big, p, p, p, p, None) == N.CSA_E_UNSUPPORTED
