"""The exchange in which the panel multiplicities travel, on the device: csa_exchange_mult_keys_async
(mult_keys_kernel), csa_merge_mult_keys_async (mkey_insert / mkey_merge / mkey_emit around an index-list
re-draw) and distributed.legacy_panel_distribution_distributed.

Simulated ranks share one device, the all_to_all done by slicing; the send segments are held to
distributed.mult_key_buckets, the owners' lists to np.unique over the (h1, h2, row) triples of the whole
run -- the project's equality rule, which knows nothing of the code under test -- and the product call to the
reference's own panel counts (tests/golden/multiplicity_<case>.json) and the C oracle's panels.  Every
assertion is integer equality."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, inst_paths, pkg
from multiplicity_cases import CASES, expected_top, mult_golden, oracle_panels

pytestmark = pytest.mark.gpu

COUPLES = "couples_panel_from_twenty_people_no_constraints_2"
UNSET = 123456789


def _enc(name, k):
    P = pkg()
    inst = P.read_instance(*inst_paths(name), k)
    return inst, P.encode(inst.categories, inst.agents)


def _expected_pairs(h, p):
    _, first, mult = np.unique(np.concatenate([h, p], axis=1), axis=0, return_index=True, return_counts=True)
    order = np.argsort(first)
    return first[order].astype(np.int64), mult[order].astype(np.int64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).ravel().copy()).cuda()


def _u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n].astype(np.int64)


def _send(h, p, W, b, e, world, cap, status, guard=64):
    """One simulated rank: csa_unique_mult_async over its share, then csa_exchange_mult_keys_async.  Returns
    the device keys (poisoned beforehand, ``guard`` more keys behind them), the counts and the local list's
    length."""
    import torch
    N = pkg("_native")
    L = N.lib()
    n = e - b
    need = int(L.csa_unique_mult_scratch_bytes(n))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device="cuda")
    first = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    mult = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    distinct = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    N.check(L.csa_unique_mult_async(N.ptr(h[2 * b:]), N.ptr(p[b * W:]), n, W, N.ptr(scratch), need, N.ptr(first),
                                    N.ptr(mult), N.ptr(distinct), N.ptr(status), None))
    sk = torch.full(((world * cap + guard) * 4,), -1, dtype=torch.int64, device="cuda")
    sc = torch.full((world,), UNSET, dtype=torch.int64, device="cuda")
    N.check(L.csa_exchange_mult_keys_async(N.ptr(h[2 * b:]), n, N.ptr(first), N.ptr(mult), N.ptr(distinct), b, world,
                                           cap, N.ptr(sk), N.ptr(sc), N.ptr(status), None))
    return sk, sc, distinct


def _merge(enc, k, seed, rk, rc, world, cap, status):
    """One simulated owner: csa_merge_mult_keys_async over its received segments, outputs poisoned
    beforehand.  Returns (first, mult) ascending in first, after checking the zero tail."""
    import torch
    N = pkg("_native")
    L = N.lib()
    seg = world * cap
    ob = int(L.csa_merge_mult_keys_scratch_bytes(seg, enc.W))
    scr = torch.full(((ob + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    of = torch.full((seg,), -1, dtype=torch.int32, device="cuda")
    om = torch.full((seg,), -1, dtype=torch.int32, device="cuda")
    od = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    N.check(L.csa_merge_mult_keys_async(enc.handle, k, seed, 0, N.ptr(rk), world, cap, N.ptr(rc), N.ptr(scr), ob,
                                        N.ptr(of), N.ptr(om), N.ptr(od), N.ptr(status), None))
    torch.cuda.synchronize()
    ln = int(od.item())
    assert 0 <= ln <= seg
    assert not of.cpu().numpy()[ln:].any() and not om.cpu().numpy()[ln:].any()      # zero past the list
    f, m = _u32(of, ln), _u32(om, ln)
    order = np.argsort(f, kind="stable")
    return f[order], m[order]


def exchange_on_device(enc, k, seed, hashes, panels, world, cap=None):
    """The 32-byte exchange with ``world`` simulated ranks on one device.  Returns (shards, cap, host sends
    [(keys uint64[world, cap, 4], counts)], owners [(first, mult)], status words)."""
    import torch
    D = pkg("distributed")
    W = panels.shape[1]
    h, p = _dev(hashes), _dev(panels)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    shards = [D.shard_range(len(panels), world, r) for r in range(world)]
    cap = cap or D.exchange_capacity(max(e - b for b, e in shards), world)
    sends = [_send(h, p, W, b, e, world, cap, status) for b, e in shards]
    torch.cuda.synchronize()
    owners = []
    for r in range(world):
        rk = torch.cat([sk[r * cap * 4:(r + 1) * cap * 4] for sk, _, _ in sends])
        rc = torch.stack([sc[r] for _, sc, _ in sends])
        owners.append(_merge(enc, k, seed, rk, rc, world, cap, status))
    host = []
    for sk, sc, _ in sends:
        raw = sk.cpu().numpy().view(np.uint64)
        assert (raw[world * cap * 4:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()       # nothing behind the segments
        host.append((raw[: world * cap * 4].reshape(world, cap, 4), sc.cpu().numpy()))
    return shards, cap, host, owners, status.cpu().numpy().astype(np.uint32)


def check_sends(shards, cap, host, hashes, panels, world):
    """Every sender's segments equal distributed.mult_key_buckets of its share, as sets."""
    D = pkg("distributed")
    for (b, e), (keys, sc) in zip(shards, host):
        mk, mc = D.mult_key_buckets(hashes[b:e], panels[b:e], b, world, cap)
        assert sc.tolist() == mc.tolist()
        for w in range(world):
            assert sorted(map(tuple, keys[w, : sc[w]].tolist())) == sorted(map(tuple, mk[w, : mc[w]].tolist()))
            assert (keys[w, sc[w]:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()         # unused keys left unwritten


def check_owners(owners, hashes, world, want_first, want_mult):
    firsts = np.concatenate([f for f, _ in owners])
    mults = np.concatenate([m for _, m in owners])
    assert len(set(firsts.tolist())) == len(firsts)
    order = np.argsort(firsts)
    assert np.array_equal(firsts[order], want_first) and np.array_equal(mults[order], want_mult)
    for r, (f, _) in enumerate(owners):
        assert np.all(hashes[f, 0] % np.uint64(world) == np.uint64(r))


_RUNS = {}


def _drawn(name, k, S, seed):
    """(enc, panels, honest hashes) of a run drawn on the device once per session."""
    key = (name, k, S, seed)
    if key not in _RUNS:
        A, D = pkg("analysis"), pkg("distributed")
        _, enc = _enc(name, k)
        panels = A.legacy_sample_raw(enc, k, S, seed, want_pairs=False, want_panels=True).panels
        _RUNS[key] = (enc, panels, D.panel_hashes(panels))
    enc, panels, hashes = _RUNS[key]
    return enc, panels, hashes.copy()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("case", ["couples", "forged", "forged_dups"])
def test_simulated_ranks_on_one_device(gpu_available, world, case):
    name, k, S, seed = ("example_small_20", 20, 5000, 3) if case == "forged" else (COUPLES, 2, 20000, 5)
    enc, panels, hashes = _drawn(name, k, S, seed)
    if case == "forged":
        assert not np.array_equal(panels[0], panels[1000])
        hashes[1000] = hashes[0]
    elif case == "forged_dups":
        x = panels[0]
        y = next(r for r in panels if not np.array_equal(r, x))
        same_x = (panels == x).all(axis=1)
        hashes[same_x] = pkg("distributed").panel_hashes(y[None])[0]      # every copy of x hashes like y
        assert same_x.sum() > world
    want_first, want_mult = _expected_pairs(hashes, panels)
    host_first, host_mult = pkg("stats").panel_multiplicities_host(panels)
    assert np.array_equal(want_first, host_first) and np.array_equal(want_mult, host_mult)
    shards, cap, host, owners, st = exchange_on_device(enc, k, seed, hashes, panels, world)
    print("%s world %d: cap %d, owners %s, status %s" % (case, world, cap, [len(f) for f, _ in owners], st.tolist()))
    assert st[0] == 0
    check_sends(shards, cap, host, hashes, panels, world)
    check_owners(owners, hashes, world, want_first, want_mult)
    assert len(want_first) == (5000 if case == "forged" else 100)


@pytest.mark.parametrize("world", [1, 3])
def test_mixed_shape(gpu_available, monkeypatch, tmp_path, world):
    """30 agents (12 + 18 over one category, quotas 1..4 each), k = 5, S = 70 001, seed 5: 39 209 distinct
    panels with multiplicities 1..8.  World 1: the local list comes from the partitioned pass (70 001 >=
    65 536 entries); world 3: from the global table (shares of 23 334)."""
    import distinct_cases as C
    monkeypatch.delenv("CSA_UNIQUE_PART", raising=False)
    A, D = pkg("analysis"), pkg("distributed")
    cat, resp = tmp_path / "categories.csv", tmp_path / "respondents.csv"
    cat.write_text("category,feature,min,max\ngender,female,1,4\ngender,male,1,4\n")
    resp.write_text("gender\n" + "female\n" * 12 + "male\n" * 18)
    k, S, seed = 5, 70001, 5
    share = D.shard_range(S, world, 0)[1]
    assert C.takes_partitioned(share, C.table_slots(share)) == (world == 1)
    inst = pkg().read_instance(str(cat), str(resp), k)
    enc = pkg().encode(inst.categories, inst.agents)
    panels = A.legacy_sample_raw(enc, k, S, seed, want_pairs=False, want_panels=True).panels
    hashes = D.panel_hashes(panels)
    want_first, want_mult = pkg("stats").panel_multiplicities_host(panels)
    shards, cap, host, owners, st = exchange_on_device(enc, k, seed, hashes, panels, world)
    assert st[0] == 0
    check_sends(shards, cap, host, hashes, panels, world)
    check_owners(owners, hashes, world, want_first, want_mult)
    assert len(want_first) == 39209 and sorted(set(want_mult.tolist())) == list(range(1, 9))


def test_segment_capacity_below_a_ranks_load(gpu_available):
    """1000 distinct panels for two owners of 100 keys each: CSA_E_UNSUPPORTED in the status block, the
    counts say how many asked, nothing is written past a segment."""
    import torch
    D, N = pkg("distributed"), pkg("_native")
    rng = np.random.default_rng(5)
    panels = rng.integers(0, 2 ** 63, size=(1000, 3), dtype=np.int64).astype(np.uint64)
    hashes = D.panel_hashes(panels)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    sk, sc, distinct = _send(_dev(hashes), _dev(panels), 3, 0, 1000, 2, 100, status)
    torch.cuda.synchronize()
    st = status.cpu().numpy().astype(np.uint32)
    assert st[0] == N.CSA_E_UNSUPPORTED and int(distinct.item()) == 1000
    with pytest.raises(N.CsaError, match="capacity"):
        N.check(N.lib().csa_status_decode(N.ptr(st)))
    counts = sc.cpu().numpy()
    assert counts.sum() == 1000 and (counts > 100).all()
    raw = sk.cpu().numpy().view(np.uint64)
    keys = raw[: 2 * 100 * 4].reshape(2, 100, 4)
    assert (raw[2 * 100 * 4:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    for w in range(2):                                   # full segments of the owner's own keys
        assert np.all(keys[w, :, 0] % np.uint64(2) == np.uint64(w)) and np.all(keys[w, :, 3] == 1)
        assert np.array_equal(hashes[keys[w, :, 2].astype(np.int64)], keys[w, :, :2])


def test_a_rank_with_no_panels(gpu_available):
    enc, panels, hashes = _drawn(COUPLES, 2, 20000, 5)
    panels, hashes = panels[:2], hashes[:2]
    shards, cap, host, owners, st = exchange_on_device(enc, 2, 5, hashes, panels, 3)
    assert shards[2] == (2, 2) and host[2][1].tolist() == [0, 0, 0] and st[0] == 0
    check_owners(owners, hashes, 3, *pkg("stats").panel_multiplicities_host(panels))


def test_merge_scratch_below_the_stated_size(gpu_available):
    import torch
    N = pkg("_native")
    L = N.lib()
    _, enc = _enc(COUPLES, 2)
    ob = int(L.csa_merge_mult_keys_scratch_bytes(16, enc.W))
    t = torch.zeros(max(ob // 8, 64) + 8, dtype=torch.int64, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = lambda nbytes: (enc.handle, 2, 0, 0, N.ptr(t), 2, 8, N.ptr(t), N.ptr(t), nbytes, N.ptr(t), N.ptr(t),   # noqa: E731
                           N.ptr(t), N.ptr(st), None)
    assert L.csa_merge_mult_keys_async(*args(ob - 1)) == N.CSA_E_INVALID
    assert "scratch" in N.last_error()


# ---- the product call -----------------------------------------------------------------------------
def _rccl_world1():
    import torch.distributed as dist
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)


def _product_case(case):
    """(instance name, k, S, seed, golden-shaped dict) of a product-call case: a golden of CASES, or
    pathological_5 at S = 20 000 (maximum 6 788 > 4 096 bins: the second spectrum pass)."""
    if case != "pathological_5_20000":
        g = mult_golden(case)
        return g["instance"], g["k"], g["S"], g["seed"], g
    name, k, S, seed = "pathological_5", 5, 20000, 0
    panels = oracle_panels(name, k, seed, S)
    first, mult = pkg("stats").panel_multiplicities_host(panels)
    rows = [sorted(int(q) for q in np.flatnonzero(np.unpackbits(r.view(np.uint8), bitorder="little"))) for r in
            panels[first]]
    assert int(mult.max()) == 6788 > pkg("analysis").MULT_BINS
    return name, k, S, seed, {"first": first.tolist(), "count": mult.tolist(), "panels": rows, "unique": len(first),
                              "S": S}


@pytest.mark.parametrize("case", CASES + ["pathological_5_20000"])
@pytest.mark.parametrize("force_exchange", ["0", "1"])
def test_product_call_rccl_world1(gpu_available, monkeypatch, case, force_exchange):
    import torch
    import torch.distributed as dist
    A, Dd, ST = pkg("analysis"), pkg("distributed"), pkg("stats")
    monkeypatch.setenv("CSA_FORCE_EXCHANGE", force_exchange)
    name, k, S, seed, g = _product_case(case)
    inst = pkg().read_instance(*inst_paths(name), k)
    one = A.legacy_panel_distribution(inst, S, seed)
    stats = dict(A.LAST_RUN_STATS)
    want_up, want_found = np.array(one[2].upper()), sorted(one[1])
    mult = np.array(g["count"])
    dev0 = torch.cuda.current_device()
    _rccl_world1()
    try:
        plain = Dd.legacy_probabilities_distributed(inst, S, seed)
        assert len(plain) == 3
        for call in range(2):                       # the second call reuses the cached exchange
            tm = {}
            out = Dd.legacy_panel_distribution_distributed(inst, S, seed, timings=tm)
            assert len(out) == 4 and torch.cuda.current_device() == dev0 and tm["total_ms"] > 0
            assert out[0] == plain[0] == one[0] and len(out[1]) == len(plain[1]) == len(one[1]) == g["unique"]
            assert np.array_equal(out[2].upper(), want_up) and np.array_equal(plain[2].upper(), want_up)
            assert A.LAST_RUN_STATS == stats        # the owner's re-draws are not draws of the run
            dist_ = out[3]
            assert isinstance(dist_, ST.ShardedPanelDistribution) == (force_exchange == "1")
            assert dist_.S == S and dist_.distinct == g["unique"]
            assert dist_.spectrum.tolist() == np.bincount(mult).tolist() == one[3].spectrum.tolist()
            assert dist_.sum_squares == int((mult * mult).sum()) and dist_.max_multiplicity == int(mult.max())
            enc = A.encode_cached(inst.categories, inst.agents)
            before = A.draw_stats(enc)
            assert dist_.top(5) == expected_top(g, 5) == one[3].top(5)
            if force_exchange == "1":
                assert not dist_._whole                  # answered from the gathered candidates
                f, m = dist_.owned()                     # one rank owns every panel
                assert f.tolist() == g["first"] and m.tolist() == g["count"]
            for e in (0, len(g["panels"]) - 1):
                assert dist_.count(g["panels"][e]) == g["count"][e]
            assert [a.tolist() for a in dist_.multiplicities()] == [g["first"], g["count"]]
            assert A.draw_stats(enc) == before and A.LAST_RUN_STATS == stats
            assert sorted(out[1]) == want_found
        if case == "couples_s0":
            # top_keep = 0 gathers nothing: top materialises; keep_panels=False: the estimators work, the rest raises
            d0 = Dd.legacy_panel_distribution_distributed(inst, S, seed, top_keep=0)[3]
            assert d0.top(3) == expected_top(g, 3)
            d1 = Dd.legacy_panel_distribution_distributed(inst, S, seed, keep_panels=False)[3]
            assert d1.spectrum.tolist() == np.bincount(mult).tolist() and d1.chao1() == one[3].chao1()
            assert d1.coverage() == one[3].coverage() and d1.collision_probability() == one[3].collision_probability()
            for fn in (lambda: d1.top(1), lambda: d1.count(g["panels"][0])):
                with pytest.raises(RuntimeError) as e:
                    fn()
                assert str(e.value) == A.PanelSet._where
    finally:
        dist.destroy_process_group()


def _gloo_worker(rank, world, port, out_dir, case):
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        Dd = pkg("distributed")
        g = mult_golden(case)
        inst = pkg().read_instance(*inst_paths(g["instance"]), g["k"])
        out = Dd.legacy_panel_distribution_distributed(inst, g["S"], g["seed"])
        d = out[3]
        f, m = d.owned()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), first=f, mult=m, spectrum=d.spectrum,
                 sums=np.array([d.S, d.distinct, d.sum_squares, d.max_multiplicity, len(out[1])]))
        dist.barrier()
        entered = []
        names = ("send", "recv", "isend", "irecv", "all_reduce", "all_gather", "all_gather_into_tensor",
                 "all_to_all_single", "broadcast", "barrier")
        real = {nm: getattr(dist, nm) for nm in names}
        for nm in names:
            setattr(dist, nm, (lambda nm_: lambda *a, **kw: (entered.append(nm_), real[nm_](*a, **kw))[1])(nm))
        try:
            if rank == world - 1:                  # the LAST rank alone: top from the candidates, then the pickle
                top = d.top(5)
                assert not d._whole
                with open(os.path.join(out_dir, "top.pkl"), "wb") as fh:
                    pickle.dump(top, fh)
                with open(os.path.join(out_dir, "dist.pkl"), "wb") as fh:
                    pickle.dump(d, fh)
            assert entered == []
        finally:
            for nm in names:
                setattr(dist, nm, real[nm])
        dist.barrier()
    finally:
        dist.destroy_process_group()


_LOAD_CHILD = r"""
import json, pickle, sys
sys.path.insert(0, %(repo)r)
with open(%(path)r, "rb") as fh:
    d = pickle.load(fh)
assert "torch" not in sys.modules, "unpickling needed torch"
print(json.dumps({"top": [[list(p), c] for p, c in d.top(5)], "count": d.count(%(panel)r), "distinct": d.distinct}))
"""


@pytest.mark.parametrize("case", ["couples_s0", "rejecty_6_s3"])
def test_product_call_gloo_two_ranks(gpu_available, tmp_path, case):
    """Two ranks on this GPU over gloo (RCCL refuses two ranks on one device)."""
    import json
    import torch.multiprocessing as mp
    g = mult_golden(case)
    mult = np.array(g["count"])
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path), case), nprocs=2, join=True)
    got = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    for r in range(2):                             # both ranks report the whole job
        assert got[r]["spectrum"].tolist() == np.bincount(mult).tolist()
        assert got[r]["sums"].tolist() == [g["S"], g["unique"], int((mult * mult).sum()), int(mult.max()), g["unique"]]
    firsts = np.concatenate([got[0]["first"], got[1]["first"]])
    mults = np.concatenate([got[0]["mult"], got[1]["mult"]])
    assert len(set(firsts.tolist())) == len(firsts)
    order = np.argsort(firsts)
    assert firsts[order].tolist() == g["first"] and mults[order].tolist() == g["count"]
    panels = oracle_panels(g["instance"], g["k"], g["seed"], g["S"])
    hashes = pkg("distributed").panel_hashes(panels)
    for r in range(2):
        assert np.all(hashes[got[r]["first"], 0] % np.uint64(2) == np.uint64(r))
    with open(tmp_path / "top.pkl", "rb") as fh:
        assert pickle.load(fh) == expected_top(g, 5)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = _LOAD_CHILD % dict(repo=REPO, path=str(tmp_path / "dist.pkl"), panel=g["panels"][3])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    back = json.loads(out.stdout)
    assert [(tuple(p), c) for p, c in back["top"]] == expected_top(g, 5)
    assert back["count"] == g["count"][3] and back["distinct"] == g["unique"]
