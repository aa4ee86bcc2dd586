"""Same-address deletion (check_same_address; legacy.py:78-113) in every launchable draw_kernel<64, FPL, WPL,
true>, bit for bit against the oracles with the same rings.

csa_instance_set_address routes every draw of an instance to draw_kernel<64, FPL, WPL, true>, where each
pick walks its address ring and deletes the household before the full-category cascades.  The reference's
own address runs (tests/test_gpu_address.py) reach draw_kernel<64, 1, 1, true> alone, with households of
at most four; here the GENERAL cells of tests/test_gpu_draw_matrix.py draw with the households of
tests/address_cases.py (one of 70 members over many words and lanes), so that a ring member sits in
another word and lane than its pick (WPL = 2 and 4), the feature rows are read in their high halves and
for FPL = 2 and 4, and the failure test the kernel defers to the end of the step is compared with an
oracle that raises inside the deletion (tests/test_oracle_address.py pins that oracle to the reference).

Per cell (test_cell_with_households_matches_oracle), after the conditions of tests/address_cases.py hold
on the oracle's output: csa_legacy_find, csa_legacy_sample (panels, counts, distinct panels),
csa_draw_async (hashes, picks; buffers pre-filled with -1), csa_draw_xt_async (no XT written),
csa_redraw_async (statistics untouched), and csa_legacy_find once more after the ring is taken away.
The three cells launch_draw refuses stay refused with a ring.

Single attempts and start states (test_single_attempts_and_start_states) on draw_kernel<64, 1, 2, true>,
<64, 2, 2, true> and <64, 4, 1, true>, against the Python oracle's draw_attempt: csa_legacy_attempt at
positions of the oracle's run, then from a start state (csa_instance_set_state) that is the oracle's
accepted attempt of the batch's first panel after its first PREFIX picks, rebuilt here by hand -- picks,
their households and the cascades of the features they filled are absent, members of the 70-member
household among them -- and csa_legacy_find over 64 panels from that state.
draw_kernel<64, 1, 2, true>'s instance raises no SelectionError with these households (none in 400 000
panels of the C oracle, from either side of panel 2^32), so its start state is made scarce: of the
feature furthest below its minimum only one holder more than it still needs stays present, and an
attempt fails as soon as two of them are deleted unpicked.

Small edges (a second or less each): one household of all n agents at k = 1 and k = 2, and households
across a word boundary (bits 63 | 64; bits 31, 32 and the last bit of a ragged last word).
"""
import ctypes

import numpy as np
import pytest

import address_cases as AC
from conftest import pkg
from oracle import coracle
from oracle.legacy_oracle import FAIL, OK, OracleInstance, PhiloxRng, draw_attempt, legacy_find
from test_gpu_draw_matrix import (BEGIN, BY_NAME, MAX_ATTEMPTS, SEED, _encode, _same, cell_S, oracle_reference,
                                  recipe_of)

pytestmark = pytest.mark.gpu

PREFIX = 14                 # picks of the oracle's attempt that the start state has behind it (of k = 20)
STATE_CELLS = ("draw_kernel<64, 1, 2, true>", "draw_kernel<64, 2, 2, true>", "draw_kernel<64, 4, 1, true>")
SCARCE = ("draw_kernel<64, 1, 2, true>",)       # (named in the docstring)


def _ids(cells):
    return [c.name for c in cells]


def _words(present, W):
    """bool[n] -> uint64[W] (agent p = bit p & 63 of word p >> 6)."""
    bits = np.zeros(W * 64, np.uint8)
    bits[:len(present)] = np.asarray(present, bool)
    return np.packbits(bits, bitorder="little").view(np.uint64)


# ---- the batch entries of a cell --------------------------------------------------------------------

def _check_find(enc, ref, k, S):
    N, A = pkg("_native"), pkg("analysis")
    picks = np.full((S, k), -1, np.int32)
    attempts = np.zeros(S, np.uint32)
    A.draw_stats(enc, reset=True)
    N.check(N.lib().csa_legacy_find(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(picks), N.ptr(attempts)))
    stats = A.draw_stats(enc)
    _same(attempts, ref.attempts, "csa_legacy_find attempts")
    _same(picks, ref.picks, "csa_legacy_find picks")
    assert stats == ref.stats


def _check_sample(enc, ref, k, S):
    N, A = pkg("_native"), pkg("analysis")
    panels = np.zeros((S, enc.W), np.uint64)
    attempts = np.zeros(S, np.uint32)
    counts = np.full(enc.n, -1, np.int64)
    uniq = np.zeros(1, np.uint64)
    A.draw_stats(enc, reset=True)
    N.check(N.lib().csa_legacy_sample(enc.handle, k, SEED, ref.begin, S,
                                      N.CSA_WANT_PANELS | N.CSA_WANT_COUNTS | N.CSA_WANT_UNIQUE, MAX_ATTEMPTS,
                                      N.ptr(panels), N.ptr(counts), None, N.ptr(uniq), N.ptr(attempts)))
    stats = A.draw_stats(enc)
    _same(attempts, ref.attempts, "csa_legacy_sample attempts")
    _same(panels, ref.panels, "csa_legacy_sample panels")
    assert np.array_equal(counts, coracle.counts(ref.panels, enc.n))
    assert int(uniq[0]) == coracle.unique(ref.panels, enc.n)
    assert stats == ref.stats


def _check_async(enc, ref, k, S):
    """csa_draw_async with hashes and picks, csa_draw_xt_async and csa_redraw_async on device buffers."""
    import torch
    N, A, D = pkg("_native"), pkg("analysis"), pkg("distributed")
    L, W = N.lib(), enc.W

    def buffers():
        return (torch.full((S * W,), -1, dtype=torch.int64, device="cuda"),
                torch.full((2 * S,), -1, dtype=torch.int64, device="cuda"),
                torch.full((S,), -1, dtype=torch.int32, device="cuda"),
                torch.zeros(4, dtype=torch.int32, device="cuda"))

    def same_panels(t, what):
        _same(t.cpu().numpy().view(np.uint64).reshape(S, W), ref.panels, what + " panels")

    def same_hashes(t, what):
        _same(t.cpu().numpy().view(np.uint64).reshape(S, 2), D.panel_hashes(ref.panels), what + " hashes")

    panels, hashes, attempts, status = buffers()
    picks = torch.full((S * k,), -1, dtype=torch.int32, device="cuda")
    A.draw_stats(enc, reset=True)
    N.check(L.csa_draw_async(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(panels), N.ptr(hashes),
                             N.ptr(attempts), N.ptr(picks), N.ptr(status), None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    same_hashes(hashes, "csa_draw_async")
    same_panels(panels, "csa_draw_async")
    _same(attempts.cpu().numpy().view(np.uint32), ref.attempts, "csa_draw_async attempts")
    _same(picks.cpu().numpy().reshape(S, k), ref.picks, "csa_draw_async picks")
    assert A.draw_stats(enc) == ref.stats

    # the fused XT belongs to the register kernels: with rings the call says so and leaves XT alone
    panels, hashes, attempts, status = buffers()
    npad, nblk = int(L.csa_xt_pad(enc.n)), (S + 63) // 64
    xt = torch.full((nblk * 2 * npad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    written = ctypes.c_int32(-1)
    N.check(L.csa_draw_xt_async(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(panels), N.ptr(hashes),
                                N.ptr(attempts), N.ptr(status), N.ptr(xt), ctypes.byref(written),
                                N.CSA_DRAW_RESET_STATUS | N.CSA_DRAW_RESET_STATS, None))
    torch.cuda.synchronize()
    assert written.value == 0 and bool((xt == 0x5A5A5A5A).all())
    assert status.tolist() == [0, 0, 0, 0]
    same_panels(panels, "csa_draw_xt_async")
    same_hashes(hashes, "csa_draw_xt_async")
    _same(attempts.cpu().numpy().view(np.uint32), ref.attempts, "csa_draw_xt_async attempts")
    assert A.draw_stats(enc) == ref.stats

    panels, _, _, status = buffers()
    N.check(L.csa_redraw_async(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(panels), N.ptr(status), None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    same_panels(panels, "csa_redraw_async")
    assert A.draw_stats(enc) == ref.stats           # a re-draw adds nothing to the statistics


@pytest.mark.parametrize("cell", AC.LAUNCHABLE, ids=_ids(AC.LAUNCHABLE))
def test_cell_with_households_matches_oracle(gpu_available, cell):
    N = pkg("_native")
    ref = AC.check_conditions(cell)
    AC.check_ring_failures()
    S = cell_S(cell)
    enc, o = _encode(cell)
    ring = AC.ring_of(o.n)[0]
    try:
        N.check(N.lib().csa_instance_set_address(enc.handle, N.ptr(ring)))
        _check_find(enc, ref, cell.k, S)
        _check_sample(enc, ref, cell.k, S)
        _check_async(enc, ref, cell.k, S)
        # without the ring the same handle draws the ring-free panels again
        N.check(N.lib().csa_instance_set_address(enc.handle, None))
        base = oracle_reference(recipe_of(cell), S)
        assert not np.array_equal(base.picks, ref.picks)
        _check_find(enc, base, cell.k, S)
    finally:
        enc.close()


@pytest.mark.parametrize("cell", AC.REFUSED, ids=_ids(AC.REFUSED))
def test_refused_cell_stays_refused_with_households(gpu_available, cell):
    """launch_draw refuses the cell (its feature rows exceed the LDS) with a ring as without one:
    CSA_E_UNSUPPORTED from every entry, nothing launched, the status block as the caller left it."""
    import torch
    N = pkg("_native")
    L = N.lib()
    S, k = 64, cell.k
    enc, o = _encode(cell)
    try:
        N.check(L.csa_instance_set_address(enc.handle, N.ptr(AC.ring_of(o.n)[0])))
        picks = np.full((S, k), -1, np.int32)
        assert L.csa_legacy_find(enc.handle, k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(picks), None) == N.CSA_E_UNSUPPORTED
        assert "LDS" in N.last_error()
        assert np.all(picks == -1)
        host = np.zeros((S, enc.W), np.uint64)
        assert L.csa_legacy_sample(enc.handle, k, SEED, BEGIN, S, N.CSA_WANT_PANELS, MAX_ATTEMPTS, N.ptr(host), None,
                                   None, None, None) == N.CSA_E_UNSUPPORTED
        assert "LDS" in N.last_error()
        assert not host.any()
        status = torch.tensor([0x5A5A5A5A, 1, 2, 3], dtype=torch.int32, device="cuda")
        panels = torch.full((S * enc.W,), -1, dtype=torch.int64, device="cuda")
        dpicks = torch.full((S * k,), -1, dtype=torch.int32, device="cuda")
        for d_picks in (None, dpicks):      # the batch route (the ring makes it GENERAL) and the pick-order route
            rc = L.csa_draw_async(enc.handle, k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(panels), None, None,
                                  N.ptr(d_picks), N.ptr(status), None)
            assert rc == N.CSA_E_UNSUPPORTED and "LDS" in N.last_error()
        torch.cuda.synchronize()
        assert status.tolist() == [0x5A5A5A5A, 1, 2, 3]
        assert bool((panels == -1).all()) and bool((dpicks == -1).all())
    finally:
        enc.close()


# ---- single attempts and start states ---------------------------------------------------------------

def _attempt(enc, k, panel, attempt):
    """csa_legacy_attempt -> (rc, picks, sel, rem, present words); every output pre-filled."""
    N = pkg("_native")
    pk = np.full(max(k, 1), -7, np.int32)
    npk = ctypes.c_int32(-7)
    sel = np.full(enc.F, -7, np.int32)
    rem = np.full(enc.F, -7, np.int32)
    present = np.full(enc.W, 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = N.lib().csa_legacy_attempt(enc.handle, k, SEED, panel, attempt, N.ptr(pk), ctypes.byref(npk), N.ptr(sel),
                                    N.ptr(rem), N.ptr(present))
    return rc, pk[:max(npk.value, 0)].tolist(), npk.value, sel, rem, present


def _oracle_attempt(o, k, panel, attempt, ring, state=(None, None, None)):
    return draw_attempt(o, k, PhiloxRng(SEED).for_attempt(panel, attempt), *state, addr_next=ring)


def _check_attempt(enc, o, k, panel, attempt, ring, state=(None, None, None), want=None):
    """One csa_legacy_attempt against draw_attempt from the same state; returns the oracle's status.
    (After a SelectionError the state outputs are unspecified, include/csa_legacy.h: the return code is
    all there is to compare.)"""
    N = pkg("_native")
    want = want or _oracle_attempt(o, k, panel, attempt, ring, state)
    rc, picks, n_picks, sel, rem, present = _attempt(enc, k, panel, attempt)
    where = "panel %d attempt %d" % (panel, attempt)
    if want[0] == FAIL:
        assert rc == N.CSA_E_SELECTION, where
        return FAIL
    assert want[0] == OK and rc == N.CSA_OK, where
    assert n_picks == len(want[1]) and picks == want[1], where
    assert sel.tolist() == want[2] and rem.tolist() == want[3], where
    assert np.array_equal(present, _words(want[4], enc.W)), where
    return OK


def _state_after(o, ring, picks):
    """(sel, rem, present) after ``picks`` were drawn in this order, by hand: each pick selected, its
    household absent, then everyone in a feature the pick filled (legacy.py:107-119 in bulk)."""
    pf, fmax = np.asarray(o.person_feat), np.asarray(o.fmax)
    present = np.ones(o.n, bool)
    sel = np.zeros(o.F, np.int64)
    for p in picks:
        assert present[p]
        sel[pf[p]] += 1
        present[p] = False
        q = ring[p]
        while q != p:
            present[q] = False
            q = ring[q]
        for c, g in enumerate(pf[p]):
            if sel[g] == fmax[g]:
                present &= pf[:, c] != g
    return sel, np.bincount(pf[present].ravel(), minlength=o.F), present


def _make_scarce(o, sel, present):
    """Of the feature furthest below its minimum, keep need + 1 holders (the lowest agents) present."""
    pf = np.asarray(o.person_feat)
    need = np.asarray(o.fmin) - sel
    f = int(np.argmax(need))
    assert need[f] >= 2
    holders = np.flatnonzero(present & (pf[:, o.fcat[f]] == f))
    present = present.copy()
    present[holders[need[f] + 1:]] = False
    return np.bincount(pf[present].ravel(), minlength=o.F), present


@pytest.mark.parametrize("name", STATE_CELLS)
def test_single_attempts_and_start_states(gpu_available, name):
    N = pkg("_native")
    L = N.lib()
    cell = BY_NAME[name]
    ref = AC.check_conditions(cell)
    enc, o = _encode(cell)
    k = cell.k
    ring_np, label = AC.ring_of(o.n)
    ring = ring_np.tolist()
    try:
        N.check(L.csa_instance_set_address(enc.handle, N.ptr(ring_np)))
        # from the default state: of the batch's first panels, the attempt that was accepted and the one
        # before it (a SelectionError or a min-quota rejection, which a single attempt returns as OK)
        if name in SCARCE:
            assert ref.stats["selection_errors"] == 0        # the oracle's run has none to take
        quota = {OK: 5, FAIL: 0} if name in SCARCE else {OK: 3, FAIL: 2}
        seen = {OK: 0, FAIL: 0}
        for i in range(16):
            for attempt in range(max(0, int(ref.attempts[i]) - 2), int(ref.attempts[i])):
                want = _oracle_attempt(o, k, ref.begin + i, attempt, ring)
                if seen[want[0]] < quota[want[0]]:
                    seen[_check_attempt(enc, o, k, ref.begin + i, attempt, ring, want=want)] += 1
        assert seen == quota, seen

        # the start state: the accepted attempt of the batch's first panel after PREFIX picks
        prefix = ref.picks[0, :PREFIX].tolist()
        sel, rem, present = _state_after(o, ring, prefix)
        upto = draw_attempt(o, PREFIX, PhiloxRng(SEED).for_attempt(ref.begin, int(ref.attempts[0]) - 1), addr_next=ring)
        assert (upto[0], upto[1]) == (OK, prefix)
        assert (upto[2], upto[3], upto[4]) == (sel.tolist(), rem.tolist(), present.tolist())   # by hand == oracle
        if name in SCARCE:
            rem, present = _make_scarce(o, sel, present)
        gone = ~present
        gone[prefix] = False
        assert (gone & (label == 0)).any() and (~gone & (label == 0)).any()    # the 70-member household, in part
        assert (gone & (label != 0) & (ring_np != np.arange(o.n))).any()
        state = (sel.tolist(), rem.tolist(), present.tolist())
        sel32, rem32, words = sel.astype(np.int32), rem.astype(np.int32), _words(present, enc.W)
        N.check(L.csa_instance_set_state(enc.handle, N.ptr(sel32), N.ptr(rem32), N.ptr(words)))
        try:
            k2 = k - PREFIX
            # the oracle's own continuation of that attempt is not a fresh one (its stream goes on at step
            # PREFIX); k2 fresh steps from the state are what csa_legacy_attempt draws
            seen = {OK: 0, FAIL: 0}
            for j in range(12):
                seen[_check_attempt(enc, o, k2, ref.begin + ref.carry - 6 + j, j % 3, ring, state)] += 1
            assert seen[OK] >= 2 and seen[FAIL] >= 2, seen
            # legacy_find from that state, 64 panels across panel 2^32
            S2, begin2 = 64, ref.begin + ref.carry - 30
            want = [legacy_find(o, k2, PhiloxRng(SEED), begin2 + i, MAX_ATTEMPTS, *state, addr_next=ring)
                    for i in range(S2)]
            picks = np.full((S2, k2), -1, np.int32)
            attempts = np.zeros(S2, np.uint32)
            N.check(L.csa_legacy_find(enc.handle, k2, SEED, begin2, S2, MAX_ATTEMPTS, N.ptr(picks), N.ptr(attempts)))
            _same(attempts, np.array([a for _, a in want], np.uint32), "csa_legacy_find attempts from the state")
            _same(picks, np.array([p for p, _ in want], np.int32), "csa_legacy_find picks from the state")
            assert sum(a for _, a in want) > S2                 # some panel restarted from the state too
        finally:
            N.check(L.csa_instance_set_state(enc.handle, None, None, None))
        # the default state is back
        assert _check_attempt(enc, o, k, ref.begin, int(ref.attempts[0]) - 1, ring) == OK
    finally:
        enc.close()


# ---- small edges ------------------------------------------------------------------------------------

def _tiny(n, k):
    """n agents, one category of two features without minimum quotas; the maxima are never reached, so
    nothing but a household is ever deleted unpicked."""
    cats = {"c": {"f0": {"min": 0, "max": k + 1}, "f1": {"min": 0, "max": k + 1}}}
    agents = {i: {"c": "f%d" % (i % 3 == 0)} for i in range(n)}
    o = OracleInstance(k=k, cat_names=["c"], feat_names=[("c", "f0"), ("c", "f1")], fmin=[0, 0], fmax=[k + 1, k + 1],
                       fcat=[0, 0], person_feat=[[int(i % 3 == 0)] for i in range(n)])
    return pkg().encode(cats, agents), o


def test_one_household_of_everyone(gpu_available):
    """All n agents at one address.  k = 1: a panel is its single pick, and the attempt leaves nobody (the
    ring walk runs its n - 1 steps).  k = 2: every attempt ends at "run out of people" (legacy.py:198-199)
    and the attempt limit is what comes back -- a status, not a fault."""
    N = pkg("_native")
    L = N.lib()
    n, S, begin = 64 * 2 + 37, 64, 2 ** 32 - 30
    ring = np.roll(np.arange(n, dtype=np.int32), -1)            # p -> p + 1 -> ... -> 0
    enc, o = _tiny(n, 1)
    try:
        N.check(L.csa_instance_set_address(enc.handle, N.ptr(ring)))
        rc, _, want_att, want = coracle.draw(o, 1, SEED, begin, S, want_picks=True, addr_next=ring)
        assert rc == 0 and (want_att == 1).all() and len(set(want[:, 0].tolist())) > 8
        picks = np.full((S, 1), -1, np.int32)
        attempts = np.zeros(S, np.uint32)
        N.check(L.csa_legacy_find(enc.handle, 1, SEED, begin, S, 3, N.ptr(picks), N.ptr(attempts)))
        _same(picks, want, "picks")
        _same(attempts, want_att, "attempts")
        for i in (0, 29, 30, 63):
            rc, pk, n_picks, sel, rem, present = _attempt(enc, 1, begin + i, 0)
            assert rc == N.CSA_OK and n_picks == 1 and pk == want[i].tolist()
            assert not present.any() and not rem.any() and sel.sum() == 1
            assert _check_attempt(enc, o, 1, begin + i, 0, ring.tolist()) == OK
    finally:
        enc.close()
    enc, o = _tiny(n, 2)
    try:
        N.check(L.csa_instance_set_address(enc.handle, N.ptr(ring)))
        panel = 2 ** 32 + 5
        assert coracle.draw(o, 2, SEED, panel, 1, max_attempts=3, addr_next=ring)[0] == 4     # OR_E_ATTEMPT_LIMIT
        for attempt in range(3):
            assert _check_attempt(enc, o, 2, panel, attempt, ring.tolist()) == FAIL
        picks = np.full((1, 2), -1, np.int32)
        assert L.csa_legacy_find(enc.handle, 2, SEED, panel, 1, 3, N.ptr(picks), None) == N.CSA_E_ATTEMPT_LIMIT
        assert N.last_error().startswith("panel %d:" % panel), N.last_error()
        # without the household the same call draws two people
        N.check(L.csa_instance_set_address(enc.handle, None))
        N.check(L.csa_legacy_find(enc.handle, 2, SEED, panel, 1, 3, N.ptr(picks), None))
        assert picks.tolist() == coracle.draw(o, 2, SEED, panel, 1, want_picks=True)[3].tolist()
    finally:
        enc.close()


def test_households_across_a_word_boundary(gpu_available):
    """draw_kernel<64, 1, 1, true>'s pool (n = 64 * 2 + 37) with two households only: bits 63 | 64 of
    adjacent words, and bits 31, 32 and the last bit of the ragged last word."""
    N = pkg("_native")
    L = N.lib()
    cell = AC.LAUNCHABLE[0]
    enc, o = _encode(cell)
    n, k, S = o.n, cell.k, 256
    assert n == 64 * 2 + 37
    houses = [(63, 64), (31, 32, n - 1)]
    ring = AC.close_rings(n, houses)
    try:
        N.check(L.csa_instance_set_address(enc.handle, N.ptr(ring)))
        rc, _, want_att, want = coracle.draw(o, k, SEED, BEGIN, S, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                             addr_next=ring)
        assert rc == 0
        picks = np.full((S, k), -1, np.int32)
        attempts = np.zeros(S, np.uint32)
        N.check(L.csa_legacy_find(enc.handle, k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(picks), N.ptr(attempts)))
        _same(attempts, want_att, "attempts")
        _same(picks, want, "picks")
        # every member is picked somewhere, never two of a household; then the state after one attempt
        for members in houses:
            hit = np.isin(want, members)
            assert hit.sum(axis=1).max() == 1
            for p in members:
                rows = np.flatnonzero((want == p).any(axis=1))
                assert len(rows), p
                i = int(rows[0])
                assert _check_attempt(enc, o, k, BEGIN + i, int(want_att[i]) - 1, ring.tolist()) == OK
    finally:
        enc.close()
