"""The household forms of the register kernels (draw_solo_hh_kernel, draw_lane_hh_kernel), every one of the
30 built, bit for bit against the C oracle with the same rings.

Under CSA_ADDRESS_BATCH (csa_instance_set_address_route) a batch draw of an instance with address rings that a
register kernel takes runs that kernel's household form: after a pick, every member of the pick's ring still
in the pool is deleted unpicked, before the full-feature cascades; the failure the reference raises inside that
deletion is deferred to the next step's start test (tests/test_oracle_address.py pins the oracle that raises
inside it).  The cells are the 70 register recipes of tests/test_gpu_draw_matrix.py with the rings of
tests/household_cases.py.  Per cell (test_cell_matches_oracle), after the cell's conditions hold on the oracle's
own output:

  * csa_draw_kernel_name names the cell's household form (over the cells all 30 are hit:
    test_every_household_kernel_ran);
  * csa_legacy_sample: panels, attempts, counts, distinct count, attempts / rejections / selection_errors;
  * csa_draw_async: panels and hashes (buffers pre-filled with -1);
  * csa_draw_picks_async: the pick order;
  * csa_draw_xt_async (DevicePipeline.draw_xt): written == 1, panels, hashes, XT (pre-filled with -1) and
    the counts against the oracle's panels transposed;
  * csa_redraw_async: panels, statistics untouched;
  * a ring of self-loops only: the ring-free panels, still on the household kernel;
  * back on CSA_ADDRESS_GENERAL: the same handle draws the same panels on draw_kernel<64, ..., true>, and
    csa_draw_xt_async reports written == 0 again.

Small edges (a second or less each): one household of all n agents at k = 1 and k = 2; mates at bits
63 | 64, 31 | 32 and the last bit of a ragged last word, and a mate in the other lane's half of a lane-kernel
pool, on a solo and on a lane cell; a household of 70 spread over 29 words; and a mate that a cascade removed
earlier in the same attempt: row 1 of draw_solo_kernel<8, 4, 8, true>'s batch (panel 2^32 - 299: the pick
of step 16, agent 142, finds its mate 29 gone since an earlier step's cascade) and row 2 of
draw_lane_kernel<32, 4, 2, 5, true>'s (panel 2^32 - 298: step 10, agent 136 in the second lane's half, mate
79 in the first's), found in the oracle's run and asserted here by replaying its picks.
"""
import ctypes

import numpy as np
import pytest

import address_cases as AC
import household_cases as HC
from conftest import pkg
from oracle import coracle
from oracle.legacy_oracle import OracleInstance
from test_gpu_address_matrix import _check_sample
from test_gpu_draw_matrix import (BEGIN, MAX_ATTEMPTS, SEED, _check_fused_xt, _check_picks, _encode, _kernel_name,
                                  _same)

pytestmark = pytest.mark.gpu

SEEN = {}   # cell name -> the csa_draw_kernel_name observed under CSA_ADDRESS_BATCH


def _households(enc, ring, route):
    N = pkg("_native")
    N.check(N.lib().csa_instance_set_address(enc.handle, N.ptr(ring)))
    N.check(N.lib().csa_instance_set_address_route(enc.handle, route))


def _sample(enc, k, begin, S, max_attempts=MAX_ATTEMPTS):
    """csa_legacy_sample -> (rc, panels, attempts)."""
    N = pkg("_native")
    panels = np.zeros((S, enc.W), np.uint64)
    attempts = np.zeros(S, np.uint32)
    rc = N.lib().csa_legacy_sample(enc.handle, k, SEED, begin, S, N.CSA_WANT_PANELS, max_attempts, N.ptr(panels),
                                   None, None, None, N.ptr(attempts))
    return rc, panels, attempts


def _check_async(enc, ref, k, S):
    """csa_draw_async (panels, hashes) and csa_redraw_async on device buffers pre-filled with -1."""
    import torch
    N, A, D = pkg("_native"), pkg("analysis"), pkg("distributed")
    L, W = N.lib(), enc.W
    panels = torch.full((S * W,), -1, dtype=torch.int64, device="cuda")
    hashes = torch.full((2 * S,), -1, dtype=torch.int64, device="cuda")
    attempts = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    A.draw_stats(enc, reset=True)
    N.check(L.csa_draw_async(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(panels), N.ptr(hashes),
                             N.ptr(attempts), None, N.ptr(status), None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    _same(hashes.cpu().numpy().view(np.uint64).reshape(S, 2), D.panel_hashes(ref.panels), "csa_draw_async hashes")
    _same(panels.cpu().numpy().view(np.uint64).reshape(S, W), ref.panels, "csa_draw_async panels")
    _same(attempts.cpu().numpy().view(np.uint32), ref.attempts, "csa_draw_async attempts")
    assert A.draw_stats(enc) == ref.stats
    panels.fill_(-1)
    N.check(L.csa_redraw_async(enc.handle, k, SEED, ref.begin, S, MAX_ATTEMPTS, N.ptr(panels), N.ptr(status), None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    _same(panels.cpu().numpy().view(np.uint64).reshape(S, W), ref.panels, "csa_redraw_async panels")
    assert A.draw_stats(enc) == ref.stats           # a re-draw adds nothing to the statistics


def _xt_written(enc, k, S):
    """written of one csa_draw_xt_async call (its buffers thrown away)."""
    import torch
    N = pkg("_native")
    L = N.lib()
    npad, nblk = int(L.csa_xt_pad(enc.n)), (S + 63) // 64
    panels = torch.zeros(S * enc.W, dtype=torch.int64, device="cuda")
    hashes = torch.zeros(2 * S, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    xt = torch.zeros(nblk * 2 * npad, dtype=torch.int32, device="cuda")
    written = ctypes.c_int32(-1)
    N.check(L.csa_draw_xt_async(enc.handle, k, SEED, BEGIN, S, MAX_ATTEMPTS, N.ptr(panels), N.ptr(hashes), None,
                                N.ptr(status), N.ptr(xt), ctypes.byref(written), 0, None))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    return written.value


@pytest.mark.parametrize("cell", HC.REGISTER, ids=[c.name for c in HC.REGISTER])
def test_cell_matches_oracle(gpu_available, cell):
    N = pkg("_native")
    ref = HC.check_conditions(cell)
    base = HC.base_of(cell)
    S, k = len(ref.attempts), cell.k
    enc, o = _encode(cell)
    ring = HC.ring_for(cell)[0]
    try:
        plain = _kernel_name(enc, k)
        assert plain == cell.name
        _households(enc, ring, N.CSA_ADDRESS_BATCH)
        SEEN[cell.name] = _kernel_name(enc, k)
        assert SEEN[cell.name] == HC.household_name(cell)
        _check_sample(enc, ref, k, S)
        _check_async(enc, ref, k, S)
        _check_picks(enc, ref, k, S)
        _check_fused_xt(enc, ref, k, S)               # (asserts written == 1)
        # self-loops only: nobody has a mate, the household kernel draws the ring-free panels
        _households(enc, np.arange(o.n, dtype=np.int32), N.CSA_ADDRESS_BATCH)
        assert _kernel_name(enc, k) == HC.household_name(cell)
        rc, panels, attempts = _sample(enc, k, BEGIN, S)
        assert rc == N.CSA_OK
        _same(attempts, base.attempts, "self-loop attempts")
        _same(panels, base.panels, "self-loop panels")
        # the default route: the same handle, the same panels, on GENERAL
        _households(enc, ring, N.CSA_ADDRESS_GENERAL)
        assert _kernel_name(enc, k).startswith("draw_kernel<64, ")
        rc, panels, attempts = _sample(enc, k, BEGIN, S)
        assert rc == N.CSA_OK
        _same(attempts, ref.attempts, "GENERAL attempts")
        _same(panels, ref.panels, "GENERAL panels")
        assert _xt_written(enc, k, 64) == 0
        # and without rings the route changes nothing
        N.check(N.lib().csa_instance_set_address(enc.handle, None))
        N.check(N.lib().csa_instance_set_address_route(enc.handle, N.CSA_ADDRESS_BATCH))
        assert _kernel_name(enc, k) == cell.name
    finally:
        enc.close()


def test_every_household_kernel_ran(gpu_available, request):
    """Every cell this session selected ran its household form; with all of them selected, all 30 built
    household kernels were hit."""
    selected = {item.callspec.params["cell"].name for item in request.session.items
                if getattr(item, "originalname", "") == "test_cell_matches_oracle" and item.module is request.module}
    assert selected, "run together with the cells"
    assert set(SEEN) == selected
    if len(selected) == len(HC.REGISTER):
        assert sorted(set(SEEN.values())) == sorted(pkg("_native").household_kernel_list())
        assert len(set(SEEN.values())) == 30


# ---- small edges ------------------------------------------------------------------------------------

def _tiny(n, k):
    """n agents, one category of two features without minimum quotas; the maxima are never reached, so
    nothing but a household is ever deleted unpicked (F = 2: draw_solo_hh_kernel<8, WN, true>)."""
    cats = {"c": {"f0": {"min": 0, "max": k + 1}, "f1": {"min": 0, "max": k + 1}}}
    agents = {i: {"c": "f%d" % (i % 3 == 0)} for i in range(n)}
    o = OracleInstance(k=k, cat_names=["c"], feat_names=[("c", "f0"), ("c", "f1")], fmin=[0, 0], fmax=[k + 1, k + 1],
                       fcat=[0, 0], person_feat=[[int(i % 3 == 0)] for i in range(n)])
    return pkg().encode(cats, agents), o


def test_one_household_of_everyone(gpu_available):
    """All n agents at one address.  k = 1: a panel is its single pick (the ring walk runs its n - 1 steps
    and empties the pool).  k = 2: every attempt runs out of people and the attempt limit is what comes
    back -- a status, not a fault."""
    N = pkg("_native")
    n, S, begin = 64 * 2 + 37, 64, 2 ** 32 - 30
    ring = np.roll(np.arange(n, dtype=np.int32), -1)            # p -> p + 1 -> ... -> 0
    enc, o = _tiny(n, 1)
    try:
        _households(enc, ring, N.CSA_ADDRESS_BATCH)
        assert _kernel_name(enc, 1) == "draw_solo_hh_kernel<8, 4, true>"
        rc, want, want_att, picks = coracle.draw(o, 1, SEED, begin, S, want_picks=True, addr_next=ring)
        assert rc == 0 and (want_att == 1).all() and len(set(picks[:, 0].tolist())) > 8
        rc, panels, attempts = _sample(enc, 1, begin, S, 3)
        assert rc == N.CSA_OK
        _same(attempts, want_att, "attempts")
        _same(panels, want, "panels")
    finally:
        enc.close()
    enc, o = _tiny(n, 2)
    try:
        _households(enc, ring, N.CSA_ADDRESS_BATCH)
        assert _kernel_name(enc, 2) == "draw_solo_hh_kernel<8, 4, true>"
        panel = 2 ** 32 + 5
        assert coracle.draw(o, 2, SEED, panel, 1, max_attempts=3, addr_next=ring)[0] == 4     # OR_E_ATTEMPT_LIMIT
        assert _sample(enc, 2, panel, 1, 3)[0] == N.CSA_E_ATTEMPT_LIMIT
        assert N.last_error().startswith("panel %d:" % panel), N.last_error()
        # without the household the same call draws two people
        N.check(N.lib().csa_instance_set_address(enc.handle, None))
        rc, panels, _ = _sample(enc, 2, panel, 1, 3)
        assert rc == N.CSA_OK
        _same(panels, coracle.draw(o, 2, SEED, panel, 1)[1], "ring-free panels")
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["draw_solo_kernel<8, 4, 8, true>", "draw_lane_kernel<32, 4, 2, 5, true>"])
def test_households_across_words_and_lane_halves(gpu_available, name):
    """n = 64 * 2 + 37 with three households only: bits 63 | 64 of adjacent words; bits 31, 32 and the last
    bit of the ragged last word; agents 5 and 150 -- words 0 and 2, which the lane kernel's two lanes hold
    (the first lane words 0 and 1, the second words 3 and 2 mirrored)."""
    N = pkg("_native")
    cell = HC.BY_NAME[name]
    enc, o = _encode(cell)
    n, k, S = o.n, cell.k, 256
    assert n == 64 * 2 + 37
    houses = [(63, 64), (31, 32, n - 1), (5, 150)]
    ring = AC.close_rings(n, houses)
    try:
        _households(enc, ring, N.CSA_ADDRESS_BATCH)
        assert _kernel_name(enc, k) == HC.household_name(cell)
        rejects = np.zeros(S, np.uint32)
        rc, want, want_att, picks = coracle.draw(o, k, SEED, BEGIN, S, max_attempts=MAX_ATTEMPTS, want_picks=True,
                                                 rejects=rejects, addr_next=ring)
        assert rc == 0
        for members in houses:          # every member is picked somewhere, never two of a household
            assert np.isin(picks, members).sum(axis=1).max() == 1
            assert all((picks == p).any() for p in members)
        rc, panels, attempts = _sample(enc, k, BEGIN, S)
        assert rc == N.CSA_OK
        _same(attempts, want_att, "attempts")
        _same(panels, want, "panels")
        stats = {"attempts": int(want_att.sum()), "rejections": int(rejects.sum()),
                 "selection_errors": int(want_att.sum()) - S - int(rejects.sum())}
        _check_picks(enc, AC.AddressReference(0, want, want_att, picks, rejects, stats, BEGIN, 300, 0, 0), k, S)
    finally:
        enc.close()


def test_household_of_seventy_over_many_words(gpu_available):
    """One household of 70, every 26th agent of n = 64 * 28 + 37: 29 words, at most three members a word."""
    N = pkg("_native")
    n, k, S = 64 * 28 + 37, 5, 128
    members = list(range(3, n, 26))[:70]
    assert len(members) == 70 and len({p >> 6 for p in members}) == 29
    ring = AC.close_rings(n, [members])
    enc, o = _tiny(n, k)
    try:
        _households(enc, ring, N.CSA_ADDRESS_BATCH)
        assert _kernel_name(enc, k) == "draw_solo_hh_kernel<8, 32, true>"
        rc, want, want_att, picks = coracle.draw(o, k, SEED, BEGIN, S, want_picks=True, addr_next=ring)
        base = coracle.draw(o, k, SEED, BEGIN, S)[1]
        assert rc == 0 and np.isin(picks, members).sum(axis=1).max() == 1 and np.isin(picks, members).any()
        assert (want != base).any()
        rc, panels, attempts = _sample(enc, k, BEGIN, S)
        assert rc == N.CSA_OK
        _same(attempts, want_att, "attempts")
        _same(panels, want, "panels")
    finally:
        enc.close()


def _cascaded_mates(o, ring, picks):
    """(step, pick, mate) of every ring mate that an earlier step's cascade had already removed when its
    pick was drawn, from a replay of an accepted attempt's picks."""
    pf, fmax = np.asarray(o.person_feat), np.asarray(o.fmax)
    present, how = np.ones(o.n, bool), {}
    sel, out = np.zeros(o.F, np.int64), []
    for t, p in enumerate(picks):
        assert present[p]
        sel[pf[p]] += 1
        present[p] = False
        q = int(ring[p])
        while q != p:
            if present[q]:
                present[q] = False
                how[q] = "mate"
            elif how.get(q) == "cascade":
                out.append((t, int(p), q))
            q = int(ring[q])
        for c, g in enumerate(pf[p]):
            if sel[g] == fmax[g]:
                gone = present & (pf[:, c] == g)
                how.update((int(x), "cascade") for x in np.flatnonzero(gone))
                present &= ~gone
    return out


@pytest.mark.parametrize("name,row,event", [("draw_solo_kernel<8, 4, 8, true>", 1, (16, 142, 29)),
                                            ("draw_lane_kernel<32, 4, 2, 5, true>", 2, (10, 136, 79))])
def test_mate_that_a_cascade_removed_earlier(gpu_available, name, row, event):
    """The panel named in the module docstring, alone: its pick's mate is no longer in the pool and must not
    be counted twice (remaining would fall one short and the later steps would pick differently)."""
    N = pkg("_native")
    cell = HC.BY_NAME[name]
    ref = HC.reference_of(cell)
    enc, o = _encode(cell)
    ring = HC.ring_for(cell)[0]
    assert event in _cascaded_mates(o, ring, ref.picks[row].tolist())
    try:
        _households(enc, ring, N.CSA_ADDRESS_BATCH)
        rc, panels, attempts = _sample(enc, cell.k, BEGIN + row, 1)
        assert rc == N.CSA_OK
        _same(attempts, ref.attempts[row:row + 1], "attempts")
        _same(panels, ref.panels[row:row + 1], "panels")
    finally:
        enc.close()
