"""GPU parity of the register draw kernels outside their step loop: the fused tail (pick lists ->
bitmasks, hashes and XT) and the prologue (the attempt-start tables copied from the instance's image).

Every case draws the same panels twice -- through the fused tail with XT (csa_draw_xt_async) and
through the split path (csa_draw_picks_async + picks_pack_kernel + the transpose pass) -- and compares

  * panels, hashes, attempts and per-person counts of the two paths,
  * the fused XT with the transpose pass over the same panels (every word the draw owns written),
  * panels and attempts with the C oracle (the Python oracle for a changed start state),
  * the draw statistics (attempts, SelectionError restarts, min-quota rejections) of both paths with the
    oracle's.

The shapes sit where the tail and the prologue can go wrong: k = 0, 1, 6, 7 mod 8 and k < 8 (padding
picks of the last pick-list chunk), panel counts around the 64-panel XT block and the 128-panel tile,
pools with one / no padding XT word, the widest pool (32 words), a pool of at most 4 words, both
register kernels and both key widths; and for the image: two instances drawn alternately, a start state
changed between draws, a dead feature, and restart-heavy instances whose attempts re-read the tables.
Bar: bit-exact.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import inst_paths, pkg
from oracle import coracle
from oracle.legacy_oracle import FAIL, OracleInstance, PhiloxRng, draw_attempt, read_instance as oracle_read

pytestmark = pytest.mark.gpu


def _pool(F_per_cat, n, k, seed, lo=0.8, hi=1.25, dead=False):
    """Random pool: one category per entry of F_per_cat (a feature count: shares ~ Dirichlet(2); or the
    list of shares), quotas floor(lo k p) / ceil(hi k p).  ``dead``: the last category gets one more
    feature, held by 4 % of the pool, with min = max = 0.  Returns (categories, agents, OracleInstance)."""
    rng = np.random.default_rng(seed)
    cats, fmin, fmax, fcat, cols, base = {}, [], [], [], [], 0
    for c, spec in enumerate(F_per_cat):
        p = rng.dirichlet(np.full(spec, 2.0)) if isinstance(spec, int) else np.asarray(spec, float)
        zero = -1
        if dead and c == len(F_per_cat) - 1:
            p, zero = np.append(0.96 * p, 0.04), len(p)
        nf = len(p)
        cats["c%d" % c] = {}
        for j in range(nf):
            a, b = (0, 0) if j == zero else (int(np.floor(lo * k * p[j])), int(np.ceil(hi * k * p[j])))
            cats["c%d" % c]["f%d" % j] = {"min": a, "max": b}
            fmin.append(a)
            fmax.append(b)
            fcat.append(c)
        assert sum(fmax[base:]) >= k >= sum(fmin[base:])
        cols.append(base + rng.choice(nf, size=n, p=p))
        base += nf
    pf = np.stack(cols, axis=1).tolist()
    names = [(c, f) for c in cats for f in cats[c]]
    agents = {i: {names[g][0]: names[g][1] for g in row} for i, row in enumerate(pf)}
    o = OracleInstance(k=k, cat_names=list(cats), feat_names=names, fmin=fmin, fmax=fmax, fcat=fcat, person_feat=pf)
    return cats, agents, o


LANE_CATS = [6, 5, 4, 3]     # 18 features: draw_lane_kernel (16 < F <= 32)
SOLO16_CATS = [4, 3, 2]      # 9 features: draw_solo_kernel, FN = 16 (slack planes)
SOLO8_CATS = [3, 2]          # 5 features: draw_solo_kernel, FN = 8


@functools.lru_cache(maxsize=None)
def _synthetic(cats_key, n, k, seed, dead=False):
    cats, agents, o = _pool([list(c) if isinstance(c, tuple) else c for c in cats_key], n, k, seed, dead=dead)
    return pkg().encode(cats, agents), o


@functools.lru_cache(maxsize=None)
def _golden(name, k):
    P = pkg()
    inst = P.read_instance(*inst_paths(name), k)
    return P.encode(inst.categories, inst.agents), oracle_read(*inst_paths(name), k)


@functools.lru_cache(maxsize=None)
def _oracle(o_key, k, seed, begin, S):
    """(panels, attempts, statistics) of the C oracle, computed once per draw and shared (read-only)."""
    o = _ORACLES[o_key]
    rejects = np.zeros(S, np.uint32)
    rc, panels, att, _ = coracle.draw(o, k, seed, begin, S, max_attempts=100000, rejects=rejects)
    assert rc == 0
    for a in (panels, att, rejects):
        a.setflags(write=False)
    return panels, att, rejects


_ORACLES = {}


def _oracle_prefix(o, k, seed, begin, S, S_ref=None):
    """The oracle's first S of S_ref panels from `begin` (a panel depends on its own index only)."""
    _ORACLES[id(o)] = o
    panels, att, rejects = _oracle(id(o), k, seed, begin, S_ref or S)
    return panels[:S], att[:S], rejects[:S]


def _stats_of(att, rejects):
    S = len(att)
    return {"attempts": int(att.sum()), "rejections": int(rejects.sum()),
            "selection_errors": int(att.sum()) - S - int(rejects.sum())}


def _kernel_name(enc, k):
    N = pkg("_native")
    buf = ctypes.create_string_buffer(128)
    N.check(N.lib().csa_draw_kernel_name(enc.handle, k, buf, 128))
    return buf.value.decode()


def _draw_both_paths(enc, k, S, seed, begin):
    """The draw through the fused tail with XT and through the split path; asserts that the two agree in
    panels, hashes, attempts, counts, XT and statistics.  Returns (panels, attempts, statistics)."""
    import torch
    A, Dv = pkg("analysis"), pkg("device")
    W = enc.W
    nblk = (S + 63) // 64
    split = Dv.DevicePipeline(enc, k, S, want_attempts=True)
    A.draw_stats(enc, reset=True)
    split.reset()
    split.draw_picks(seed, begin, S)
    split.pack(S)
    split.transpose_count(S)
    torch.cuda.synchronize()
    assert int(split.status[0].item()) == 0
    stats_split = A.draw_stats(enc, reset=True)

    fused = Dv.DevicePipeline(enc, k, S, want_attempts=True)
    fused.reset()
    fused.xt.fill_(-1)                          # every word the draw owns must be written
    fused.panels.fill_(-1)
    fused.hashes.fill_(-1)
    assert fused.draw_xt(seed, begin, S)
    fused.pair_counts(S, overwrite=True, alone=True)
    fused.counts_from_pairs()
    torch.cuda.synchronize()
    assert int(fused.status[0].item()) == 0
    stats_fused = A.draw_stats(enc)

    assert torch.equal(fused.panels[: S * W], split.panels[: S * W])
    assert torch.equal(fused.hashes[: 2 * S], split.hashes[: 2 * S])
    assert torch.equal(fused.attempts[:S], split.attempts[:S])
    assert torch.equal(fused.xt[: nblk * fused.npad], split.xt[: nblk * split.npad])
    assert torch.equal(fused.counts, split.counts)
    assert int(fused.counts.sum()) == S * k
    assert stats_fused == stats_split
    return (fused.panels[: S * W].cpu().numpy().view(np.uint64).reshape(S, W),
            fused.attempts[:S].cpu().numpy().astype(np.uint32), stats_fused)


def _check(enc, o, k, S, seed, begin=0, S_ref=None):
    panels, att, stats = _draw_both_paths(enc, k, S, seed, begin)
    opanels, oatt, orej = _oracle_prefix(o, k, seed, begin, S, S_ref)
    assert np.array_equal(att, oatt)
    assert np.array_equal(panels, opanels)
    assert stats == _stats_of(oatt, orej)


def _expect_kernel(enc, k, kind, fn, wn, k8=True):
    name = _kernel_name(enc, k)
    assert name.startswith("draw_%s_kernel<%d, %d," % (kind, fn, wn)), name
    assert name.endswith("true>" if k8 else "false>"), name


# ---- the last pick-list chunk: k = 0, 1, 6, 7 mod 8 and a single partial chunk ---------------------

@pytest.mark.parametrize("k", [5, 16, 17, 22, 23])
@pytest.mark.parametrize("kind,cats,fn", [("lane", LANE_CATS, 32), ("solo", SOLO16_CATS, 16), ("solo", SOLO8_CATS, 8)])
def test_last_chunk_padding(gpu_available, kind, cats, fn, k):
    enc, o = _synthetic(tuple(cats), 300, k, 1000 + k)
    _expect_kernel(enc, k, kind, fn, 8)
    _check(enc, o, k, 333, seed=3, begin=7)


# ---- panel counts around the XT block (64) and the tile (128; the solo workgroup: two tiles) -------

@pytest.mark.parametrize("S", [1, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257])
@pytest.mark.parametrize("kind,cats,fn", [("lane", LANE_CATS, 32), ("solo", SOLO16_CATS, 16)])
def test_ragged_panel_counts(gpu_available, kind, cats, fn, S):
    k = 22
    enc, o = _synthetic(tuple(cats), 300, k, 2000)
    _expect_kernel(enc, k, kind, fn, 8)
    _check(enc, o, k, S, seed=9, begin=0, S_ref=257)


# ---- pool sizes: one padding XT word (n = 1727), none (1792), the widest pool (2048), W <= 4 --------

@pytest.mark.parametrize("n,wn", [(1727, 28), (1792, 28), (2048, 32), (200, 4)])
@pytest.mark.parametrize("kind,cats,fn", [("lane", LANE_CATS, 32), ("solo", SOLO16_CATS, 16), ("solo", SOLO8_CATS, 8)])
def test_pool_sizes(gpu_available, kind, cats, fn, n, wn):
    k = 40
    enc, o = _synthetic(tuple(cats), n, k, 3000 + n)
    _expect_kernel(enc, k, kind, fn, wn)
    _check(enc, o, k, 333, seed=n, begin=64)


def test_sf_e_shape(gpu_available):
    """The flagship shape (n = 1727: W = 27, one padding word; F = 31; k = 110 = 6 mod 8)."""
    enc, o = _golden("sf_e_110", 110)
    _expect_kernel(enc, 110, "lane", 32, 28)
    _check(enc, o, 110, 333, seed=2, begin=0)


# ---- both key widths: a minimum above 127 takes the 16-bit keys -----------------------------------

@pytest.mark.parametrize("kind,cats,fn", [("lane", [(0.6, 0.4)] + LANE_CATS[:3] + [(0.5, 0.5)], 32),
                                          ("solo", [(0.6, 0.4), 4, 3], 16), ("solo", [(0.6, 0.4), (0.4, 0.35, 0.25)], 8)])
def test_sixteen_bit_keys(gpu_available, kind, cats, fn):
    k = 300
    enc, o = _synthetic(tuple(cats), 1000, k, 4000)
    assert max(o.fmin) > 127 and max(o.fmax) <= 255
    _expect_kernel(enc, k, kind, fn, 16, k8=False)
    _check(enc, o, k, 200, seed=4, begin=0)


# ---- the instance's image ---------------------------------------------------------------------------

def test_two_instances_alternate(gpu_available):
    """Each instance keeps its own tables: two lane instances and a solo instance drawn in turn."""
    k = 22
    a = _synthetic(tuple(LANE_CATS), 300, k, 5000)
    b = _synthetic(tuple(LANE_CATS), 300, k, 5001)
    c = _synthetic(tuple(SOLO16_CATS), 300, k, 5002)
    for rnd in range(2):
        for enc, o in (a, b, c):
            _check(enc, o, k, 150, seed=6, begin=150 * rnd)


def _python_oracle(o, k, seed, begin, S, sel0):
    """Panels and attempts of legacy_find from the start state sel0 (the Python oracle's attempt loop)."""
    src = PhiloxRng(seed)
    W = (o.n + 63) // 64
    panels, att = np.zeros((S, W), np.uint64), np.zeros(S, np.uint32)
    for i in range(S):
        a = 0
        while True:
            st, picks, sel, _, _ = draw_attempt(o, k, src.for_attempt(begin + i, a), sel=sel0)
            a += 1
            if st != FAIL and all(sel[f] >= o.fmin[f] for f in range(o.F)):
                break
        for p in picks:
            panels[i, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
        att[i] = a
    return panels, att


@pytest.mark.parametrize("kind,cats,fn", [("lane", LANE_CATS, 32), ("solo", SOLO16_CATS, 16), ("solo", SOLO8_CATS, 8)])
def test_start_state_changed_between_draws(gpu_available, kind, cats, fn):
    """Drawn, the start state changed (some features partly used, none at its max: still a register
    kernel), drawn again from the rebuilt tables, and once more after the state is put back."""
    N = pkg("_native")
    k, S = 22, 70
    # an instance of its own: its start state is changed below
    ccats, agents, o = _pool(cats, 300, k, 6000)
    enc = pkg().encode(ccats, agents)
    _check(enc, o, k, S, seed=8)
    sel0 = np.array([1 if (f % 2 == 0 and o.fmax[f] >= 3) else 0 for f in range(o.F)], np.int32)
    assert sel0.any()
    N.check(N.lib().csa_instance_set_state(enc.handle, N.ptr(sel0), None, None))
    try:
        _expect_kernel(enc, k, kind, fn, 8)
        panels, att, stats = _draw_both_paths(enc, k, S, 8, 0)
        opanels, oatt = _python_oracle(o, k, 8, 0, S, sel0.tolist())
        assert np.array_equal(att, oatt)
        assert np.array_equal(panels, opanels)
        assert stats["attempts"] == int(oatt.sum())
    finally:
        N.check(N.lib().csa_instance_set_state(enc.handle, None, None, None))
    _check(enc, o, k, S, seed=8)


@pytest.mark.parametrize("kind,cats,fn", [("lane", LANE_CATS, 32), ("solo", SOLO16_CATS, 16), ("solo", SOLO8_CATS, 8)])
def test_dead_feature(gpu_available, kind, cats, fn):
    """A feature with min = max = 0 that has holders: its row and its person-mask bit are removed."""
    k = 22
    enc, o = _synthetic(tuple(cats), 300, k, 7000, dead=True)
    dead = [f for f in range(o.F) if o.fmax[f] == 0]
    assert len(dead) == 1 and o.pool_counts()[dead[0]] > 0
    _expect_kernel(enc, k, kind, fn, 8)
    _check(enc, o, k, 333, seed=5)


@pytest.mark.parametrize("name,k,S,kind", [("rejecty_6", 6, 2000, "solo"), ("sf_e_tight_110", 110, 1500, "lane")])
def test_restart_heavy(gpu_available, name, k, S, kind):
    """Many restarted attempts (the goldens: 9.9 attempts per panel at rejecty_6, 1.5 at sf_e_tight_110):
    every attempt start re-reads the tables."""
    enc, o = _golden(name, k)
    assert _kernel_name(enc, k).startswith("draw_%s_kernel" % kind)
    _check(enc, o, k, S, seed=3)
    _, oatt, _ = _oracle_prefix(o, k, 3, 0, S)
    assert int(oatt.sum()) - S > S // 4      # the instance restarts as often as its golden says
