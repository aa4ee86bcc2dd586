"""The register draw kernels' holder-scan keep and pool drop, where the pick sits and where the scan stops.

draw_lane_kernel and draw_solo_kernel keep the scanned word pair under a lane predicate (the one-lane
kernel: narrowing pair by pair, a lane leaving the scan at the first pair it does not take; the two-lane
kernel: every pair's own) and drop the pick from the register pool with a predicated 64-bit add per pair.
What can go wrong is tied to the
position of the pick (word, bit, lane) and to the pair at which a lane leaves the scan, so the instances
here draw EVERYONE: k = n from a pool of n = 64 W agents, one category whose features' maxima are their
holder counts.  No feature fills before its last holder is picked, no attempt restarts, and every
(word, bit) position of every lane -- bit 0, 31, 32 and 63, the first and the last word of each lane, the
second lane's mirrored pool -- is picked and dropped in every panel.  Everything is compared bit for bit
with the C oracle: the pick lists in pick order, the panels, their hashes, the attempts and the draw
statistics.  96 panels per batch (one and a half waves of the two-lane kernel, part of a wave of the
one-lane kernel), from panel 2^32 - 40, so every batch carries the Philox panel counter into its high word.

Where the instances differ from "minimum 0, maximum = holders, one category, n = 64 W" (each on the CPU
oracle alone: the plain recipe returns CSA_E_NO_CANDIDATE or leaves the register kernels):

  * a feature with more than 100 holders gets the minimum holders - 99 instead of 0.  The reference's
    argmax starts from the ratio -100 (legacy.py:125), so with minimum 0 a feature whose selected count
    reaches 100 x remaining is never chosen again and its last holders can never be picked; with the
    minimum holders - 99 the need never falls below -98.  The maxima, and with them the cascades, are
    unchanged.
  * the 16-bit-key cases (a minimum of -200) use two categories: a feature with need <= -200 stops being a
    candidate while it still has holders, so they must stay reachable through a second category.  The
    register kernels take maxima up to 255 only, so the two categories have 8 + 9 features (F = 17) up to
    W = 28 and 9 + 9 (F = 18, still the two-lane kernel) at W = 32.
  * F = 8 at W = 32 has n = 2040 = 8 x 255 agents (the last word ends at bit 55): 2048 agents in 8 features
    put 256 holders, one more than the register kernels' largest maximum, into every feature.
"""
import collections
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLD, inst_paths, pkg
from oracle import coracle
from oracle.legacy_oracle import OracleInstance
from oracle.legacy_oracle import read_instance as oracle_read

S = 96
BEGIN = 2 ** 32 - 40
SEED = 20250117
MAX_ATTEMPTS = 1000

# kernel: the family the instance must route to; W: pool words; cats: features per category; neg: the first
# feature's minimum is -200 (16-bit keys); single: words whose 64 agents alone hold one feature each
Case = collections.namedtuple("Case", "kernel W cats neg single n")


def _case(kernel, W, cats, neg=False, single=(), n=None):
    return Case(kernel, W, tuple(cats), neg, tuple(single), n or 64 * W)


CASES = (
    # the two-lane kernel: one pair per lane (no predicated keep), two pairs (the smallest keep), seven
    # pairs (an odd count), eight; 8-bit keys, and once each with a minimum of -200 (16-bit keys)
    [_case("lane", W, (17,)) for W in (4, 8, 28, 32)]
    + [_case("lane", W, (8, 9), neg=True) for W in (4, 8, 28)] + [_case("lane", 32, (9, 9), neg=True)]
    # the one-lane kernel
    + [_case("solo", W, (F,), n=2040 if (F, W) == (8, 32) else None) for F in (8, 16) for W in (4, 8, 32)]
    # a feature held by the agents of one word only: its rank falls exactly on a pair boundary (the holder
    # count before the next pair equals the rank sought) -- word 1 (the end of the first lane's first pair),
    # word 3 (the end of its second pair, and of the one-lane kernel's first row batch) and word 6 (the
    # end of the second lane's first pair in its mirrored order)
    + [_case("lane", 8, (17,), single=(1, 3, 6)), _case("solo", 8, (16,), single=(1, 3, 6))]
)


def _id(c):
    return "%s-W%d-F%d%s%s" % (c.kernel, c.W, sum(c.cats), "-min200" if c.neg else "", "-oneword" if c.single else "")


@functools.lru_cache(maxsize=None)
def instance(case):
    """(categories, agents, OracleInstance) of a case: every category deals its features round-robin over a
    random permutation of the agents (holder counts differ by at most one), after the single-word features
    of the first category took their words."""
    n = case.n
    rng = np.random.default_rng(1000 * case.W + sum(case.cats) + case.neg)
    cols, cats, fmin, fmax, fcat, base = [], {}, [], [], [], 0
    for c, nf in enumerate(case.cats):
        col = np.full(n, -1, np.int64)
        first = 0
        if c == 0:
            for w in case.single:
                col[64 * w: 64 * w + 64] = first
                first += 1
        rest = np.flatnonzero(col < 0)
        col[rng.permutation(rest)] = first + np.arange(len(rest)) % (nf - first)
        holders = np.bincount(col, minlength=nf)
        cats["c%d" % c] = {}
        for j in range(nf):
            h = int(holders[j])
            lo = -200 if (case.neg and c == 0 and j == 0) else max(0, h - 99)
            cats["c%d" % c]["f%d" % j] = {"min": lo, "max": h}
            fmin.append(lo)
            fmax.append(h)
            fcat.append(c)
        cols.append(base + col)
        base += nf
    pf = np.stack(cols, axis=1).tolist()
    names = [(c, f) for c in cats for f in cats[c]]
    agents = {i: {names[g][0]: names[g][1] for g in row} for i, row in enumerate(pf)}
    o = OracleInstance(k=n, cat_names=list(cats), feat_names=names, fmin=fmin, fmax=fmax, fcat=fcat, person_feat=pf)
    return cats, agents, o


Reference = collections.namedtuple("Reference", "panels attempts picks stats")


@functools.lru_cache(maxsize=None)
def reference(case):
    """The C oracle's draw of a case's batch, computed once and shared read-only."""
    _, _, o = instance(case)
    rejects = np.zeros(S, np.uint32)
    rc, panels, att, picks = coracle.draw(o, o.k, SEED, BEGIN, S, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                          rejects=rejects, threads=min(16, os.cpu_count() or 1))
    assert rc == 0
    for a in (panels, att, picks):
        a.setflags(write=False)
    stats = {"attempts": int(att.sum()), "rejections": int(rejects.sum()),
             "selection_errors": int(att.sum()) - S - int(rejects.sum())}
    return Reference(panels, att, picks, stats)


def _kernel_name(enc, k):
    N = pkg("_native")
    buf = ctypes.create_string_buffer(128)
    N.check(N.lib().csa_draw_kernel_name(enc.handle, k, buf, 128))
    return buf.value.decode()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
        raise AssertionError("%s differ from the oracle in %d of %d rows, first at row %d"
                             % (what, len(bad), len(want), bad[0]))


def _check_picks(enc, ref, k, n_panels, seed, begin):
    """csa_draw_picks_async (the row pick-list layout): picks in pick order, attempts, statistics."""
    import torch
    N, A = pkg("_native"), pkg("analysis")
    assert N.lib().csa_draw_picks_supported(enc.handle, k) == 1
    kp = int(N.lib().csa_picks_stride(k))
    picks = torch.full((n_panels * kp,), -1, dtype=torch.int16, device="cuda")
    att = torch.zeros(n_panels, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    A.draw_stats(enc, reset=True)
    N.check(N.lib().csa_draw_picks_async(enc.handle, k, seed, begin, n_panels, MAX_ATTEMPTS, N.ptr(picks), N.ptr(att),
                                         N.ptr(status), None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    _same(att.cpu().numpy().view(np.uint32), ref.attempts, "csa_draw_picks_async attempts")
    got = picks.cpu().numpy().view(np.uint16).astype(np.int32).reshape(n_panels, kp)[:, :k]
    _same(got, ref.picks, "csa_draw_picks_async picks")
    assert A.draw_stats(enc) == ref.stats


def _check_fused(enc, ref, k, n_panels, seed, begin):
    """DevicePipeline.draw_xt (the fused pack, chunked pick lists): panels, hashes, attempts, statistics."""
    import torch
    A, D, Dv = pkg("analysis"), pkg("distributed"), pkg("device")
    W = enc.W
    pipe = Dv.DevicePipeline(enc, k, n_panels, want_attempts=True)
    pipe.reset()
    for t in (pipe.panels, pipe.hashes, pipe.attempts):
        t.fill_(-1)
    A.draw_stats(enc, reset=True)
    assert pipe.draw_xt(seed, begin, n_panels, max_attempts=MAX_ATTEMPTS)
    torch.cuda.synchronize()
    assert pipe.status.tolist() == [0, 0, 0, 0]
    _same(pipe.attempts[:n_panels].cpu().numpy().view(np.uint32), ref.attempts, "draw_xt attempts")
    _same(pipe.panels[: n_panels * W].cpu().numpy().view(np.uint64).reshape(n_panels, W), ref.panels, "draw_xt panels")
    _same(pipe.hashes[: 2 * n_panels].cpu().numpy().view(np.uint64).reshape(n_panels, 2), D.panel_hashes(ref.panels),
          "draw_xt hashes")
    assert A.draw_stats(enc) == ref.stats


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_draw_everyone_matches_oracle(gpu_available, case):
    cats, agents, o = instance(case)
    ref = reference(case)
    # the oracle's own output: every agent is picked exactly once, at the first attempt
    assert np.all(ref.attempts == 1) and np.all(np.sort(ref.picks, axis=1) == np.arange(o.n))
    enc = pkg().encode(cats, agents)
    try:
        assert enc.W == case.W and o.F == sum(case.cats)
        name = _kernel_name(enc, o.k)
        if case.kernel == "lane":
            assert name.startswith("draw_lane_kernel<32, %d," % case.W), name
            assert name.endswith("false>") == case.neg, name
        else:
            assert name.startswith("draw_solo_kernel<%d, %d," % (8 if o.F <= 8 else 16, case.W)), name
        _check_picks(enc, ref, o.k, S, SEED, BEGIN)
        _check_fused(enc, ref, o.k, S, SEED, BEGIN)
    finally:
        enc.close()


def test_single_word_features_stop_on_a_pair_boundary():
    """The single-word cases do what they are for (on the oracle alone, no GPU).  Every pick inside such a
    word is made through its feature, among the word's remaining agents: the pick is the LAST of them when
    the rank equals the remaining count (the first lane's holder count after the word's pair equals the
    rank sought) and the FIRST when the rank is 1 (the same on the second lane, which counts from the
    end).  Both happen at least 20 times per word with two or more agents left."""
    for case in CASES:
        if not case.single:
            continue
        ref = reference(case)
        for w in case.single:
            last = first = 0
            for row in ref.picks:
                left = set(range(64 * w, 64 * w + 64))
                for p in row[(row >= 64 * w) & (row < 64 * w + 64)].tolist():
                    if len(left) >= 2:
                        last += p == max(left)
                        first += p == min(left)
                    left.remove(p)
            assert last >= 20 and first >= 20, (case, w, last, first)


@pytest.mark.gpu
def test_restart_heavy_golden(gpu_available):
    """pathological_5, 200 panels: 15.6 attempts per panel in the golden (3119 in all), most ending in a
    SelectionError raised at the start of the step after a pick (between a keep and the next drop) -- picks,
    panels, attempts against the C oracle, attempts and both restart counts per panel against the reference's
    golden.  n = 30 (one pool word): it runs the WN = 4 form of draw_solo_kernel, whose scan has two pairs, so the restarts
    cross the one keep boundary of that form (the larger forms' boundaries are the other tests')."""
    with open(os.path.join(GOLD, "philox_pathological_5_s0.json")) as fh:
        g = json.load(fh)
    n_panels, k, seed = 200, g["k"], g["seed"]
    inst = pkg().read_instance(*inst_paths(g["instance"]), k)
    o = oracle_read(*inst_paths(g["instance"]), k)
    rejects = np.zeros(n_panels, np.uint32)
    rc, panels, att, picks = coracle.draw(o, k, seed, 0, n_panels, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                          rejects=rejects)
    assert rc == 0
    # the oracle against the golden (the unmodified reference's own split)
    assert att.tolist() == g["attempts"][:n_panels]
    assert rejects.tolist() == g["rejections"][:n_panels]
    assert (att - 1 - rejects).tolist() == g["selection_errors"][:n_panels]
    assert picks[:64].tolist() == g["first_picks"]
    stats = {"attempts": sum(g["attempts"][:n_panels]), "rejections": sum(g["rejections"][:n_panels]),
             "selection_errors": sum(g["selection_errors"][:n_panels])}
    assert stats["selection_errors"] >= 500 and stats["rejections"] >= 100
    ref = Reference(panels, att, picks, stats)
    enc = pkg().encode(inst.categories, inst.agents)
    try:
        assert _kernel_name(enc, k).startswith("draw_solo_kernel<"), _kernel_name(enc, k)
        _check_picks(enc, ref, k, n_panels, seed, 0)
        _check_fused(enc, ref, k, n_panels, seed, 0)
    finally:
        enc.close()
